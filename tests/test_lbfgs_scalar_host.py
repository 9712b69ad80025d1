"""CPU test of the optimiser's scalar layer (csrc/lbfgs_scalar.h) against its specification: compiles tests/lbfgs_scalar_check.cpp --
a stand-alone program that runs the header's cubic_interpolate, flipped_orientation and fresh_state on the records of a binary
file -- for the host only, with AddressSanitizer and UBSan, runs it once, and compares what it wrote with
oracle.lbfgs_machine.cubic_interpolate (value and type tag bit for bit, or NaN on both sides), oracle.fit_frame.flipped_orientation
(1 float32 ulp of the largest component: both sides compute in double and round once, another libm may move that rounding by one
step) and the initial state of oracle.lbfgs_machine.StageMachine.  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

from oracle import lbfgs_machine as LM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "cubic_overflow.npz"))
N_RANDOM = 20000
PPTPPT = 0b100100           # function values and abscissae Python floats, directional derivatives tensors (tools/make_goldens.py)


def cubic_cases():
    """Rows of 10: x1 f1 g1 x2 f2 g2 lo hi, the tag mask, has_bounds.  A value tagged as a tensor is a float32 already.
    First the golden's rows under the tagging the golden was made with and with every scalar a Python float (what its float64
    column computes: there a tensor rounds nothing); then seeded cases with random tags, with and without bounds, some with
    abscissae a few float32 steps apart and some with a function value near 1e25 (d1 ** 2 overflows in float32)."""
    rows = []
    for tags in (PPTPPT, 0):
        for x1, f1, g1, x2, f2, g2 in GOLD["rows"]:
            rows.append([x1, f1, g1, x2, f2, g2, 0.0, 0.0, tags, 0])
    rng = np.random.RandomState(11)
    for _ in range(N_RANDOM):
        x1 = rng.uniform(0.0, 2.0)
        x2 = x1 * (1.0 + 2e-7 * rng.randn()) if rng.rand() < 0.03 else x1 + rng.uniform(-2.0, 2.0)
        fs, gs = 10.0 ** rng.randint(0, 6), 10.0 ** rng.randint(0, 6)
        f1, f2, g1, g2 = fs * rng.randn(), fs * rng.randn(), gs * rng.randn(), gs * rng.randn()
        if rng.rand() < 0.02:
            f2 = 1e25 * rng.uniform(0.1, 3.0)
        lo = min(x1, x2) + rng.uniform(-0.5, 0.5)
        hi = lo + rng.uniform(0.0, 3.0)
        rows.append([x1, f1, g1, x2, f2, g2, lo, hi, rng.randint(0, 256), rng.randint(0, 2)])
    rows = np.array(rows, np.float64)
    for k in range(8):
        t = (rows[:, 8].astype(int) >> k) & 1 == 1
        rows[t, k] = rows[t, k].astype(np.float32)
    return rows


def flip_cases():
    rng = np.random.RandomState(12)
    v = rng.randn(5000, 3)
    v *= (rng.uniform(0.0, 3.1, size=(5000, 1)) / np.linalg.norm(v, axis=1, keepdims=True))
    special = [np.zeros(3)] + [s * np.eye(3)[a] for s in (1e-13, np.pi) for a in range(3)]
    return np.concatenate([v, np.array(special)]).astype(np.float32)


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """(cubic rows, [value, tag] of each, flip rows, flipped orientation of each, fresh_state fields) from ONE run of the program."""
    tmp = tmp_path_factory.mktemp("lbfgs_scalar")
    exe = str(tmp / "lbfgs_scalar_check")
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17",
                    "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "lbfgs_scalar_check.cpp"), "-o", exe], check=True)
    cub, flip = cubic_cases(), flip_cases()
    np.concatenate([[len(cub), len(flip)], cub.ravel(), flip.astype(np.float64).ravel()]).astype("<f8").tofile(str(tmp / "in.bin"))
    r = subprocess.run([exe, str(tmp / "in.bin"), str(tmp / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:]
    assert r.stdout.strip().endswith("sizeof(OptScal) = 360")
    out = np.fromfile(str(tmp / "out.bin"), "<f8")
    assert out.size == 2 * len(cub) + 3 * len(flip) + 10
    a, b = 2 * len(cub), 2 * len(cub) + 3 * len(flip)
    return cub, out[:a].reshape(-1, 2), flip, out[a:b].reshape(-1, 3), out[b:]


def oracle_cubic(row):
    sc = [LM.T(row[k]) if (int(row[8]) >> k) & 1 else LM.P(row[k]) for k in range(8)]
    return LM.cubic_interpolate(*sc[:6], bounds=(sc[6], sc[7]) if row[9] else None)


def test_cubic_interpolate_is_the_specifications_bit_for_bit(answers):
    cub, got = answers[0], answers[1]
    assert len(cub) >= 2 * len(GOLD["rows"]) + 10000
    old, LM.Sc.dt = LM.Sc.dt, np.float32
    try:
        want = [oracle_cubic(row) for row in cub]
    finally:
        LM.Sc.dt = old
    both_nan = 0
    for i, (row, w, (v, t)) in enumerate(zip(cub, want, got)):
        if np.isnan(w.v) or np.isnan(v):
            assert np.isnan(w.v) and np.isnan(v), (i, row, w, v)
            both_nan += 1
            continue
        wv = np.float64(w.v)           # (a float32 widens exactly)
        assert wv.tobytes() == np.float64(v).tobytes() and int(t) == int(w.t), (i, row, w, v, t)
    share = both_nan / len(cub)
    print("%d cases, NaN on both sides in %d (%.2f %%)" % (len(cub), both_nan, 100 * share))
    assert share <= 0.05, "the cases are meant to be finite in all but a few per cent"
    # the golden itself: its float32 column under its own tagging (the three overflow rows are NaN), its float64 column with
    # Python floats throughout
    n = len(GOLD["rows"])
    assert np.isnan(GOLD["f32"][:3]).all() and np.isnan(got[:3, 0]).all() and np.isfinite(got[3:n, 0]).all()
    assert np.all(got[n:2 * n, 1] == 0)
    for v, w in zip(got[3:n, 0], GOLD["f32"][3:]):
        assert v == np.float32(w) or abs(v - w) <= 1e-6 * abs(w), (v, w)          # (the bound of test_oracle_vs_golden.py)
    for v, w in zip(got[n:2 * n, 0], GOLD["f64"]):
        assert v == w or abs(v - w) <= 1e-6 * abs(w), (v, w)


def test_flipped_orientation_matches_the_specification(answers):
    from oracle.fit_frame import flipped_orientation
    flip, got = answers[2], answers[3]
    worst = 0.0
    for i, (r, g) in enumerate(zip(flip, got)):
        want = np.asarray(flipped_orientation(r.astype(np.float64))).astype(np.float32)
        ulp = np.spacing(np.abs(want).max()) if np.abs(want).max() > 0 else np.float32(0)
        err = np.abs(g - want.astype(np.float64)).max()
        worst = max(worst, err / ulp if ulp > 0 else err)
        assert err <= ulp, (i, r, g, want)
    print("%d rotation vectors, largest difference %.2f float32 ulp of the largest component" % (len(flip), worst))


def test_fresh_state_is_the_machines_initial_state(answers):
    m = LM.StageMachine(np.zeros(4, np.float32))
    phase, outer, n_iter_total, func_evals, evals, hd_v, hd_t, hist_n, cache_valid, has_prev_outer = answers[4]
    assert (phase, outer, n_iter_total, func_evals, evals) == (m.phase, m.outer, m.n_iter_total, m.func_evals, m.evals)
    assert (hd_v, bool(hd_t)) == (float(m.H_diag.v), m.H_diag.t)
    assert hist_n == len(m.Y) and bool(cache_valid) == (m.cache is not None) and bool(has_prev_outer) == (m.prev_loss_outer is not None)
