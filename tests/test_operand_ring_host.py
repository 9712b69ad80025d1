"""CPU test of the dense loop's operand-set bookkeeping (csrc/operand_ring.h): compiles tests/operand_ring_check.cpp -- a
stand-alone program that drives the ring as csrc/host/fit_loop.hip DenseLoop does, through scripted sequences of round forms (multi-round
launches with R = 1, 3 and 8, single self-served, key / rest and serial rounds, admission and compaction exports between them,
several fits on one ring) beside a model of the two streams, and checks after every step that no set is written while an
unawaited GEMM reads it, that every evaluation gets exactly one GEMM in order, that cur is the latest export, and that retired
frames leave their last column in every set read later -- for the host only, with AddressSanitizer and UBSan, and runs it.
No GPU needed."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_operand_ring_follows_the_scripted_forms(tmp_path):
    exe = str(tmp_path / "operand_ring_check")
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17",
                    "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "operand_ring_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-2000:]
    assert re.fullmatch(r"[1-9]\d* checks, 0 failed", r.stdout.strip().splitlines()[-1])
