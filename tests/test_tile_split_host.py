"""CPU test of the dense GEMM's tile lists (csrc/model_tables.h tile_key / tile_rest): compiles tests/tile_split_check.cpp -- a
stand-alone program that builds the tables of tiny descriptors and checks that the two lists partition the tiles, ascend, and
split them exactly by `holds an exported vertex` (V not a multiple of 16, an empty key list, every tile a key tile) -- for the
host only, with AddressSanitizer and UBSan, and runs it.  Product and lab form.  No GPU needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.parametrize("defines", [[], ["-DSFX_LAB"]], ids=["product", "lab"])
def test_tile_lists_partition_the_tiles_by_consumer(defines, tmp_path):
    exe = str(tmp_path / "tile_split_check")
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17", *defines,
                    "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "tile_split_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:]
    assert " 0 failed" in r.stdout
