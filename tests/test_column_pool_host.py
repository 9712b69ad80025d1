"""CPU test of the dense loop's column pool (csrc/column_pool.h): compiles tests/column_pool_check.cpp -- a stand-alone program
that drives the pool with scripted stage-flag snapshots as csrc/host/fit_loop.hip DenseLoop::poll does (5 frames through 2 columns, 32
resident, 70 / 32, 48 / 32, 40 / 16, a random finishing order at 200 / 64) and checks map, running list, admission order and
the compaction rule after every poll -- for the host only, with AddressSanitizer and UBSan, and runs it.  No GPU needed."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_column_pool_follows_the_scripted_polls(tmp_path):
    exe = str(tmp_path / "column_pool_check")
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17",
                    "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "column_pool_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:]
    assert re.fullmatch(r"[1-9]\d* checks, 0 failed", r.stdout.strip().splitlines()[-1])
