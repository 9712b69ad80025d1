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


# ---- the line search's transitions on seeded states (lbfgs_scalar_check.cpp: TR_IN numbers in, TR_OUT out per case)
TR_IN, TR_OUT = 38, 36
SCALARS = ("t", "t_prev", "f_prev", "gtd_prev", "ls_f0", "ls_gtd0", "d_norm", "br0", "br1", "bf0", "bf1", "bgtd0", "bgtd1")
INTS = ("ls_iter", "ls_evals", "ls_done", "insuf", "low", "high")
N_PER_KIND = 2500
BRACKET, ZOOM, TRIAL = 0, 1, 2


def transition_cases():
    """Rows of TR_IN: kind, the 13 scalars as (value, tag), the six integers, f_in, gtd_new, max_ls, max_iter, tol_change.  States
    a line search can be in and a good many it cannot (any scalar may be a Python float or a tensor): both sides follow the same
    rounding rule whatever the tags.  Sizes and signs are drawn so that every branch of the three transitions is met often
    (the counts are asserted on the specification's side in the test).  4 % of the zoom-phase evaluations return a NaN loss, which
    becomes a bracket end that every comparison rejects; the bracket phase gets none: a NaN that meets the curvature condition
    there makes a one-point bracket on which the reference itself has no defined end (opt_ext_common.NAN_CONFIG)."""
    old, LM.Sc.dt = LM.Sc.dt, np.float32
    try:
        return _transition_cases()
    finally:
        LM.Sc.dt = old


def _transition_cases():
    rng = np.random.RandomState(13)
    f32 = lambda v: float(np.float32(v))
    rows = []
    for kind in (BRACKET, ZOOM, TRIAL):
        for _ in range(N_PER_KIND):
            gs, fs = 10.0 ** rng.randint(-1, 3), 10.0 ** rng.randint(-1, 3)
            v = dict.fromkeys(SCALARS, 0.0)
            v["t_prev"] = 0.0 if rng.rand() < 0.5 else rng.uniform(0.0, 1.0)
            v["t"] = v["t_prev"] + rng.uniform(0.01, 2.0)
            v["ls_f0"] = fs * rng.randn()
            v["ls_gtd0"] = -gs * (abs(rng.randn()) + 1e-3)
            v["gtd_prev"] = -gs * abs(rng.randn())
            v["d_norm"] = 10.0 ** rng.uniform(-12, 1)
            v["br0"] = rng.uniform(0.0, 2.0)
            v["br1"] = v["br0"] * (1.0 + 1e-7 * rng.randn()) if rng.rand() < 0.08 else v["br0"] + rng.uniform(0.05, 1.0) * rng.choice([-1, 1])
            v["bf0"], v["bf1"] = v["ls_f0"] - fs * rng.uniform(0, 1), v["ls_f0"] - fs * rng.uniform(0, 1)
            v["bgtd0"], v["bgtd1"] = gs * rng.randn(), gs * rng.randn()
            armijo_line = v["ls_f0"] + 1e-4 * v["t"] * v["ls_gtd0"]
            gtd_new = 1.5 * gs * rng.randn()
            if kind == BRACKET:
                f_in = armijo_line + fs * abs(rng.randn()) * (-1 if rng.rand() < 0.7 else 1)
                v["f_prev"] = f_in + fs * rng.randn() if rng.rand() < 0.3 else v["ls_f0"] + fs
            else:
                v["t"] = v["br0"] + rng.uniform(0, 1) * (v["br1"] - v["br0"])
                f_in = min(v["bf0"], v["bf1"]) + 0.3 * fs * rng.randn()
                v["f_prev"] = v["ls_f0"]
            if kind == ZOOM and rng.rand() < 0.04:
                f_in = np.nan
            tag = {k: int(rng.rand() < (0.9 if ("gtd" in k or k == "d_norm") else 0.5 if k in ("t", "t_prev", "br0", "br1") else 0.1))
                   for k in SCALARS}
            for k in SCALARS:
                if tag[k]:
                    v[k] = f32(v[k])
            low = 0 if LM.le(LM.Sc(v["bf0"], tag["bf0"]), LM.Sc(v["bf1"], tag["bf1"])) else 1
            ints = dict(ls_iter=int(rng.choice([0, 1, 2, 3, 7, 19, 25, 29], p=[.2, .2, .2, .1, .1, .05, .1, .05])),
                        ls_evals=int(rng.randint(0, 30)), ls_done=int(kind == TRIAL and rng.rand() < 0.1),
                        insuf=int(kind == TRIAL and rng.rand() < 0.5), low=low, high=1 - low)
            row = [kind]
            for k in SCALARS:
                row += [v[k], tag[k]]
            row += [ints[k] for k in INTS]
            row += [f32(f_in), f32(gtd_new), 25, int(rng.choice([20, 30, 7])), float(rng.choice([1e-9, 0.0, 1e-3]))]
            assert len(row) == TR_IN
            rows.append(row)
    return np.array(rows, np.float64)


class OneTransition(LM.StageMachine):
    """The specification put into a given state of a line search on a one-variable problem (d = 1, so g . d is g itself), which
    stops after ONE transition: `after` says what it would have gone on with.  The stored gradients are marked by their values
    (ls_g0 101, g_prev 102, the bracket's 201 and 202), so where each one went shows afterwards."""

    def __init__(self, row):
        LM.StageMachine.__init__(self, np.zeros(1, np.float32), max_ls=int(row[35]), max_iter=int(row[36]), tol_change=row[37])
        s = {k: LM.Sc(row[1 + 2 * i], bool(row[2 + 2 * i])) for i, k in enumerate(SCALARS)}
        self.t, self.t_prev, self.f_prev, self.gtd_prev = s["t"], s["t_prev"], s["f_prev"], s["gtd_prev"]
        self.ls_f0, self.ls_gtd0, self.d_norm = s["ls_f0"], s["ls_gtd0"], s["d_norm"]
        self.br, self.bf, self.bgtd = [s["br0"], s["br1"]], [s["bf0"], s["bf1"]], [s["bgtd0"], s["bgtd1"]]
        self.ls_iter, self.ls_evals, self.ls_done, self.insuf, self.low, self.high = (int(x) for x in row[27:33])
        self.ls_g0, self.g_prev = np.float32([101.0]), np.float32([102.0])
        self.bg = [np.float32([201.0]), np.float32([202.0])]
        self.d, self.x_init = np.ones(1, np.float32), np.zeros(1, np.float32)
        self.phase, self.after, self.stop_before_trial = LM.PH_BRACKET, None, True

    def _zoom_next(self):
        if self.stop_before_trial:
            self.after = "zoom_next"
        else:
            LM.StageMachine._zoom_next(self)

    def _finish_ls(self):
        self.after = "finish_ls"

    def state(self):
        sc = [self.t, self.t_prev, self.f_prev, self.gtd_prev, self.ls_f0, self.ls_gtd0, self.d_norm, self.br[0], self.br[-1],
              self.bf[0], self.bf[-1], self.bgtd[0], self.bgtd[-1]]
        return sc, [self.ls_iter, self.ls_evals, int(self.ls_done), int(self.insuf), self.low, self.high]


def spec_transition(row):
    """(branches of the specification taken, what the transition hands the vector layer, phase, scalars, integers) for one case."""
    m = OneTransition(row)
    kind, f_in, g_new = int(row[0]), LM.P(np.float32(row[33])), np.float32([row[34]])
    gtd = LM.T(g_new[0])
    taken = []
    if kind == BRACKET:
        if m.ls_iter == m.max_ls:
            taken.append("bracket: max_ls exhausted")
        elif m._armijo_fail(f_in, m.t) or (m.ls_iter > 1 and LM.ge(f_in, m.f_prev)):
            taken.append("bracket -> zoom by Armijo")
        elif m._curv_ok(gtd):
            taken.append("bracket -> zoom, one-point bracket")
        elif LM.ge(gtd, LM.P(0)):
            taken.append("bracket -> zoom by slope >= 0")
        else:
            taken.append("bracket extension")
        m._on_bracket(f_in, g_new)
        g0 = {101.0: 1, 102.0: 2}.get(float(m.bg[0][0]), 3) if m.after else 0
        assert (m.after is None) == (taken[0] == "bracket extension") and m.after in (None, "zoom_next")
        ret = [g0, 0, 0]
    elif kind == ZOOM:
        lo, hi = m.low, m.high
        if m._armijo_fail(f_in, m.t) or LM.ge(f_in, m.bf[lo]):
            taken.append("zoom replaces high end")
        elif m._curv_ok(gtd):
            taken.append("zoom done by curvature")
        elif LM.ge(LM.mul(gtd, LM.sub(m.br[hi], m.br[lo])), LM.P(0)):
            taken.append("zoom: low end moved to the high end first")
        else:
            taken.append("zoom replaces low end")
        m.phase = LM.PH_ZOOM
        m._on_zoom(f_in, g_new)
        marks = [float(b[0]) for b in m.bg]
        end = [i for i in (0, 1) if marks[i] not in (201.0, 202.0)]
        assert len(end) == 1 and np.float32(marks[end[0]]) == g_new[0]
        end = end[0]
        copy_first = int(marks[1 - end] == 201.0 + end)
        assert copy_first == (taken[0] == "zoom: low end moved to the high end first")
        if m.after == "finish_ls":
            taken.append("zoom bracket collapse")
        ret = [end, copy_first, int(m.after == "finish_ls")]
    else:
        m.stop_before_trial = False
        if not (m.ls_done or not (m.ls_iter < m.max_iter)):
            t = LM.cubic_interpolate(m.br[0], m.bf[0], m.bgtd[0], m.br[1], m.bf[1], m.bgtd[1])
            bmax = m.br[1] if LM.gt(m.br[1], m.br[0]) else m.br[0]
            bmin = m.br[1] if LM.lt(m.br[1], m.br[0]) else m.br[0]
            eps = LM.mul(LM.P(0.1), LM.sub(bmax, bmin))
            if LM.lt(LM.pmin(LM.sub(bmax, t), LM.sub(t, bmin)), eps):
                if m.insuf or LM.ge(t, bmax) or LM.le(t, bmin):
                    near_max = LM.lt(LM.sabs(LM.sub(t, bmax)), LM.sabs(LM.sub(t, bmin)))
                    taken.append("zoom trial clamped to bmax - eps" if near_max else "zoom trial clamped to bmin + eps")
                else:
                    taken.append("zoom trial sets insuf")
        m._zoom_next()
        ret = [int(m.after is None), 0, 0]
    sc, ints = m.state()
    return taken, ret, m.phase, sc, ints


BRANCHES = ("bracket -> zoom by Armijo", "bracket -> zoom, one-point bracket", "bracket -> zoom by slope >= 0", "bracket extension",
            "zoom replaces high end", "zoom done by curvature", "zoom replaces low end", "zoom bracket collapse",
            "zoom trial clamped to bmin + eps", "zoom trial clamped to bmax - eps", "zoom trial sets insuf",
            "zoom: low end moved to the high end first", "bracket: max_ls exhausted")


def test_line_search_transitions_are_the_specifications_bit_for_bit(answers):
    """ls_bracket_eval, ls_zoom_eval and ls_zoom_trial, called directly on seeded states, against StageMachine put into the same
    state and stopped after the one transition: every scalar the transition can write (value and tag, bit for bit, or NaN on
    both sides), low / high / ls_done / insuf / ls_iter / ls_evals, the phase, and what the vector layer is told to do with the
    gradients.  The whole-machine replays (test_opt_wide_host.py) never reach two of the thirteen branches; here each is taken
    at least 50 times, counted on the specification's side, and at most 5 % of the cases carry a NaN on both sides."""
    trans, got = answers[5], answers[6]
    old = LM.Sc.dt
    count = dict.fromkeys(BRANCHES, 0)
    both_nan = 0
    try:
        LM.Sc.dt = np.float32
        for i, (row, g) in enumerate(zip(trans, got)):
            taken, ret, phase, sc, ints = spec_transition(row)
            for b in taken:
                count[b] += 1
            assert [int(x) for x in g[:3]] == ret and int(g[3]) == phase, (i, row, taken, g[:4], ret, phase)
            nan_here = False
            for k, (name, w) in enumerate(zip(SCALARS, sc)):
                v, t = g[4 + 2 * k], g[5 + 2 * k]
                if np.isnan(w.v) or np.isnan(v):
                    assert np.isnan(w.v) and np.isnan(v) and int(t) == int(w.t), (i, name, taken, w, v, t)
                    nan_here = True
                    continue
                assert np.float64(w.v).tobytes() == np.float64(v).tobytes() and int(t) == int(w.t), (i, name, taken, w, v, t)
            assert [int(x) for x in g[30:36]] == ints, (i, taken, g[30:36], ints)
            both_nan += nan_here
    finally:
        LM.Sc.dt = old
    for b in BRANCHES:
        print("%-45s %d" % (b, count[b]))
    share = both_nan / len(trans)
    print("%d cases, NaN on both sides in %d (%.2f %%)" % (len(trans), both_nan, 100 * share))
    assert all(count[b] >= 50 for b in BRANCHES), count
    assert share <= 0.05, "the cases are meant to be finite in all but a few per cent"


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """(cubic rows, [value, tag] of each, flip rows, flipped orientation of each, fresh_state fields, transition rows, the program's
    answer to each) from ONE run of the program."""
    tmp = tmp_path_factory.mktemp("lbfgs_scalar")
    exe = str(tmp / "lbfgs_scalar_check")
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17",
                    "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "lbfgs_scalar_check.cpp"), "-o", exe], check=True)
    cub, flip, trans = cubic_cases(), flip_cases(), transition_cases()
    np.concatenate([[len(cub), len(flip)], cub.ravel(), flip.astype(np.float64).ravel()]).astype("<f8").tofile(str(tmp / "in.bin"))
    trans.astype("<f8").tofile(str(tmp / "trans_in.bin"))
    r = subprocess.run([exe, str(tmp / "in.bin"), str(tmp / "out.bin"), str(tmp / "trans_in.bin"), str(tmp / "trans_out.bin")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:]
    assert r.stdout.strip().endswith("sizeof(OptScal) = 360")
    out = np.fromfile(str(tmp / "out.bin"), "<f8")
    assert out.size == 2 * len(cub) + 3 * len(flip) + 10
    a, b = 2 * len(cub), 2 * len(cub) + 3 * len(flip)
    tout = np.fromfile(str(tmp / "trans_out.bin"), "<f8")
    assert tout.size == TR_OUT * len(trans)
    return cub, out[:a].reshape(-1, 2), flip, out[a:b].reshape(-1, 3), out[b:], trans, tout.reshape(-1, TR_OUT)


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
