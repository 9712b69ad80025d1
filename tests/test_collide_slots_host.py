"""CPU test of the interpenetration term's slot layout (csrc/collide_slots.h): compiles tests/collide_slots_check.cpp -- a stand-alone
program that includes that header ALONE and runs its pen_public_stats on the stats rows of a binary file -- for the host only, with
AddressSanitizer and UBSan, once per stride of the row (16: every build; 32: -DPEN_COUNT), runs it, and compares what it wrote with
the same fold written in numpy over the slot numbers the layout has had since the term was built (they are part of what
sfx_pen_stats reports: renumbering them must be a decision, not an accident).  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PAIRS, DROPPED, OVERFLOW, WALKS_CUT, ONE_SIDED = 0, 1, 2, 13, 15


def rows(stride):
    """Hand-written rows: all slots zero; a clean mesh; one-sided pairs > 0; overflow and cut walks; every slot of the row a
    different number (a fold that read a wrong slot would show); large counts."""
    r = np.zeros((6, stride), np.int32)
    r[1, [PAIRS, 3, 14]] = 412, 16384, 9031
    r[2, [PAIRS, DROPPED, ONE_SIDED, 14]] = 5000, 37, 12, 20000
    r[3, [OVERFLOW, WALKS_CUT, 3]] = 262144, 3, 16384
    r[4] = 1000 + 7 * np.arange(stride)
    r[5, [PAIRS, DROPPED, OVERFLOW, WALKS_CUT, ONE_SIDED]] = 2 ** 30, 2 ** 29, 2 ** 31 - 1, 2 ** 20, 2 ** 29
    r[5, 4:13] = 123456          # (the clock window below the two counts: never part of the fold)
    return r


def numpy_fold(r):
    return np.stack([r[:, PAIRS] - r[:, ONE_SIDED], r[:, DROPPED] + r[:, ONE_SIDED], r[:, OVERFLOW], r[:, WALKS_CUT]], 1)


@pytest.mark.parametrize("stride", [16, 32])
def test_public_stats_fold_matches_numpy(stride, tmp_path):
    exe = str(tmp_path / "collide_slots_check")
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17",
                    "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] +
                   (["-DPEN_COUNT"] if stride == 32 else []) +
                   [os.path.join(ROOT, "tests", "collide_slots_check.cpp"), "-o", exe], check=True)
    r = rows(stride)
    np.concatenate([[stride, len(r)], r.ravel()]).astype("<i4").tofile(str(tmp_path / "in.bin"))
    p = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:]
    got = np.fromfile(str(tmp_path / "out.bin"), "<i4").reshape(-1, 4)
    want = numpy_fold(r)
    assert got.shape == want.shape and np.array_equal(got, want), (got, want)
    assert np.array_equal(got[0], [0, 0, 0, 0])                       # all slots zero
    assert np.array_equal(got[2], [5000 - 12, 37 + 12, 0, 0])         # one-sided pairs leave the pairs and count as dropped
    # the program's own account of the layout: the slots above, the clock window [4, 15), 16 work counters of which 6 are public
    m = re.search(r"rows of (\d+); pairs (\d+) dropped (\d+) overflow (\d+) walks_cut (\d+) one_sided (\d+); clock window (\d+) \+ (\d+); "
                  r"work slots (\d+), public (\d+), debug from (\d+)", p.stdout)
    assert m and [int(v) for v in m.groups()] == [stride, PAIRS, DROPPED, OVERFLOW, WALKS_CUT, ONE_SIDED, 4, 11, 16, 6, 8], p.stdout
