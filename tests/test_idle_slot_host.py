"""CPU test of the owner of a model's idle collision handle (csrc/host/idle_slot.h): compiles tests/idle_slot_check.cpp -- a
stand-alone program that drives take / give / drop with counted dummy handles (take from empty, exact, larger than asked, too
small, cap mismatch, stale generation; give into empty, smaller, equal, larger, stale generation; drop; destruction with one
idle) and checks after every operation which handle is idle and that every handle made is destroyed exactly once -- for the host
only, with AddressSanitizer and UBSan, and runs it.  No GPU needed."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_idle_slot_keeps_one_handle_and_destroys_each_once(tmp_path):
    exe = str(tmp_path / "idle_slot_check")
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17",
                    "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "idle_slot_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:]
    assert re.fullmatch(r"[1-9]\d* checks, 0 failed", r.stdout.strip().splitlines()[-1])
