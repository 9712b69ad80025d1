"""CPU test of the model's host tables (csrc/model_tables.h): compiles tests/model_tables_check.cpp -- a stand-alone program
that builds the tables of a tiny descriptor and checks each against its definition, the row-overflow fallback and every
refusal -- for the host only, with AddressSanitizer and UBSan, and runs it.  Product and lab form (the lab form also builds
the k-major `dirs`).  No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.parametrize("defines", [[], ["-DSFX_LAB"]], ids=["product", "lab"])
def test_model_tables_against_their_definitions(defines, tmp_path):
    exe = str(tmp_path / "model_tables_check")
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17", *defines,
                    "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "model_tables_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:]
    assert " 0 failed" in r.stdout
