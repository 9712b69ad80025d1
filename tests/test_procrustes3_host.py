"""CPU test of the 3x3 Procrustes solve (csrc/procrustes3.h, the solve of sfx_eval_align): compiles tests/procrustes3_check.cpp --
a stand-alone program that reads float64 K matrices, writes the header's R for each and itself checks R^T R = I, det R = +1,
R K symmetric and tr(R K) >= tr(Q K) over 1 000 random rotations -- for the host only, with AddressSanitizer and UBSan, runs it,
and compares every R with numpy's V Z U^T (evaluation.ProcrustesAlignment, utils.py:575-581) to 1e-12.  The matrices: the two
golden sets, their z-mirrored versions (det K < 0: the reflection branch), rank-2 K (three points; four coplanar points), K
scaled by 1e-12 and by 1e+12, and a K with two equal singular values, where the properties alone are asked for.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
G = np.load(os.path.join(ROOT, "tests", "golden", "evaluation.npz"))


def cross_covariance(est, gt):
    """K = X1 X2^T of evaluation.ProcrustesAlignment for point sets [N, 3]."""
    X1, X2 = (est - est.mean(0)).T, (gt - gt.mean(0)).T
    return X1 @ X2.T


def numpy_rotation(K):
    U, _, Vh = np.linalg.svd(K)
    Z = np.eye(3)
    Z[-1, -1] *= np.sign(np.linalg.det(U @ Vh))
    return Vh.T @ Z @ U.T


def matrices():
    rng = np.random.RandomState(7)
    mirror = np.array([1.0, 1.0, -1.0])
    out = []
    for tag in ("j", "v"):
        est, gt = G[tag + "_est"].astype(np.float64), G[tag + "_gt"].astype(np.float64)
        out.append((tag, cross_covariance(est, gt), True))
        out.append((tag + " mirrored", cross_covariance(est * mirror, gt), True))
    three = rng.normal(size=(3, 3)) + 2.0
    out.append(("three points", cross_covariance(1.3 * three @ numpy_rotation(rng.normal(size=(3, 3))).T + 0.01 * rng.normal(size=(3, 3)), three), True))
    flat = rng.normal(size=(4, 3))
    flat[:, 2] = 0.0                                                    # four points of the plane z = 0, both sets
    out.append(("four coplanar", cross_covariance(flat + 0.05 * rng.normal(size=(4, 3)) * [1, 1, 0], flat), True))
    K = out[2][1]
    out.append(("scaled 1e-12", K * 1e-12, True))
    out.append(("scaled 1e+12", K * 1e+12, True))
    U, V = numpy_rotation(rng.normal(size=(3, 3))), numpy_rotation(rng.normal(size=(3, 3)))
    out.append(("equal singular values", U @ np.diag([2.0, 2.0, 1.0]) @ V.T, False))
    return out


def test_rotation_matches_numpy_and_is_the_optimal_proper_rotation(tmp_path):
    exe = str(tmp_path / "procrustes3_check")
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17",
                    "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "procrustes3_check.cpp"), "-o", exe], check=True)
    cases = matrices()
    Ks = np.stack([K for _, K, _ in cases])
    # the preconditions the cases are named after
    dets = [np.linalg.det(K) for K in Ks]
    assert dets[0] > 0 and dets[2] > 0
    assert dets[1] == pytest.approx(-2.1e3, rel=0.05) and dets[3] == pytest.approx(-1.5e8, rel=0.05), dets[:4]
    for i in (4, 5):
        s = np.linalg.svd(Ks[i], compute_uv=False)
        assert s[2] <= 1e-15 * s[0] < 1e-3 * s[1], (cases[i][0], s)       # rank 2 exactly (up to the rounding of the sums)
    Ks.astype("<f8").tofile(str(tmp_path / "K.bin"))
    r = subprocess.run([exe, str(tmp_path / "K.bin"), str(tmp_path / "R.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:]
    assert re.fullmatch(r"[1-9]\d* checks, 0 failed", r.stdout.strip().splitlines()[-1])
    out = np.fromfile(str(tmp_path / "R.bin"), "<f8").reshape(len(cases), 12)
    for (name, K, unique), row in zip(cases, out):
        R, sv = row[:9].reshape(3, 3), row[9:]
        assert np.allclose(sv, np.linalg.svd(K, compute_uv=False), rtol=1e-12, atol=1e-15 * np.abs(K).max()), (name, sv)
        assert abs(np.linalg.det(R) - 1.0) <= 1e-13, name
        if unique:
            err = np.abs(R - numpy_rotation(K)).max()
            print("%-24s max |R - numpy| = %.2e" % (name, err))
            assert err <= 1e-12, (name, err)
