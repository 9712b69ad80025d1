"""The numpy oracle of the chamfer term's contract (include/sfx.h, sfx_chamfer_forward / sfx_chamfer_backward; csrc/chamfer.hip,
csrc/chamfer_math.h), the point sets the tests run it on and the yardstick of their float comparisons.  Plain numpy: nothing of
the package, nothing of the reference tree.

Exact parts (bit for bit): the nearest index and its squared distance -- float32, ((dx dx + dy dy) + dz dz) from the coordinate
differences, the lowest index of a tie -- and, in rows_exact, the gradient rows in the device's own float64 order (gather term,
then the row's list in ascending query index, cut into segments by seg_len).
Float parts: loss and gradients by the formulas of the contract in a dtype of the caller's choice at GIVEN indices; a test
evaluates them in float64 (the reference) and in float32 (the yardstick): bound = max(10 x |f32 - f64|, 2^-22 x max|f64|)."""
import functools

import numpy as np

SERIAL_MAX = 32         # CH_SERIAL_MAX, CH_SEGMENTS of csrc/chamfer_math.h
SEGMENTS = 64
SHAPES = ((1, 1), (2, 3), (511, 1023), (512, 1024), (513, 1025), (1025, 2049), (2049, 513))     # 512 queries / 1024 targets per tile


# ---- point sets -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def normal_clouds(B, Na, Nb, seed=0):
    rng = np.random.RandomState(1000 * seed + 7 * Na + Nb + B)
    return rng.normal(size=(B, Na, 3)).astype(np.float32), rng.normal(size=(B, Nb, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def body_clouds(B, Na, Nb, seed=0):
    """Body-scale: a ~ N(0, diag(.25, .5, .12)) metres, b a resampling of a's points plus 5 mm of noise."""
    rng = np.random.RandomState(2000 * seed + 7 * Na + Nb + B)
    a = (rng.normal(size=(B, Na, 3)) * [0.25, 0.5, 0.12]).astype(np.float32)
    pick = rng.randint(0, Na, size=(B, Nb))
    b = (np.take_along_axis(a, pick[..., None].repeat(3, -1), 1) + 0.005 * rng.normal(size=(B, Nb, 3))).astype(np.float32)
    return a, b


@functools.lru_cache(maxsize=None)
def lattice_clouds(Na=600, Nb=1500):
    """Integer coordinates in -3 .. 3: float32 is exact and most queries have a tied minimum."""
    rng = np.random.RandomState(5)
    return rng.randint(-3, 4, size=(1, Na, 3)).astype(np.float32), rng.randint(-3, 4, size=(1, Nb, 3)).astype(np.float32)


# Rows of a 70-row destination set (one full wave and six rows of the next) and the entries each collects, per mesh: in the first
# wave two lists past SERIAL_MAX (33: 33 segments of 1; 130: segments of 3, the last one short) beside one of exactly SERIAL_MAX,
# shorter ones and empty rows; in the second wave one long list among rows that are empty or collect a single entry.  The two
# meshes put their long lists on different lanes (mesh 1: the first and the last lane of the first wave, the last row of all).
LONG_LIST_ROWS = ({5: 33, 20: 130, 41: 32, 66: 33, 64: 1, 69: 1, 7: 1, 30: 3, 50: 20, 12: 31},
                  {0: 130, 63: 33, 17: 32, 69: 33, 65: 1, 1: 1, 40: 4, 33: 25, 8: 26})
LONG_LIST_NROWS = 70


@functools.lru_cache(maxsize=None)
def long_list_clouds():
    """(a [2, 70, 3], b [2, 285, 3], counts [2, 70]): a on a 10 cm grid with 5 mm of jitter, b 5 mm about the rows of
    LONG_LIST_ROWS in a shuffled order, so b's nearest points in a are those rows, counts[m, r] queries each."""
    rng = np.random.RandomState(21)
    r = np.arange(LONG_LIST_NROWS)
    a = (np.stack([0.1 * (r % 10), 0.1 * (r // 10), 0.0 * r], 1) + 0.005 * rng.normal(size=(2, LONG_LIST_NROWS, 3))).astype(np.float32)
    counts = np.array([[rows.get(int(k), 0) for k in r] for rows in LONG_LIST_ROWS])
    pick = np.stack([rng.permutation(np.repeat(r, c)) for c in counts])
    b = (np.take_along_axis(a, pick[..., None].repeat(3, -1), 1) + 0.005 * rng.normal(size=pick.shape + (3,))).astype(np.float32)
    return a, b, counts


def masks_and_weights(B, Na, Nb, seed=3):
    rng = np.random.RandomState(seed + Na + Nb)
    ma, mb = rng.rand(B, Na) > 0.3, rng.rand(B, Nb) > 0.3
    ma[:, 0] = True; mb[:, 0] = True
    wa, wb = rng.uniform(0.2, 2.0, size=(B, Na)).astype(np.float32), rng.uniform(0.2, 2.0, size=(B, Nb)).astype(np.float32)
    return ma, mb, wa, wb


# ---- exact: nearest index and squared distance ----------------------------------------------------------------------------------
def dist2(q, t):
    """[Nq, Nt] squared distances in the dtype of the inputs, in the contract's association."""
    d = q[:, None, :] - t[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def nearest(q, t, mq=None, mt=None):
    """One mesh, one direction: (idx int32 [Nq], s [Nq]) in the dtype of q.  -1 / 0 at a masked query and when no target is valid;
    -1 / NaN where valid targets exist and none is nearer than +inf."""
    mq = np.ones(len(q), bool) if mq is None else np.asarray(mq, bool)
    mt = np.ones(len(t), bool) if mt is None else np.asarray(mt, bool)
    idx, s = np.full(len(q), -1, np.int32), np.zeros(len(q), q.dtype)
    if not mt.any():
        return idx, s
    with np.errstate(invalid="ignore", over="ignore"):
        d = dist2(q, t)
    d[:, ~mt] = np.inf
    d[np.isnan(d)] = np.inf                       # (every comparison with a NaN is false: never nearer)
    j = np.argmin(d, 1)                           # the first of equal minima
    m = d[np.arange(len(q)), j]
    found = m < np.inf
    idx[:] = np.where(found, j, -1)
    s[:] = np.where(found, m, np.nan)
    idx[~mq] = -1
    s[~mq] = 0
    return idx, s


def nearest_batch(a, b, ma=None, mb=None):
    """idx_ab [B, Na], idx_ba [B, Nb], dist2_ab, dist2_ba for a batch."""
    out = [[], [], [], []]
    for k in range(len(a)):
        ia, sa = nearest(a[k], b[k], None if ma is None else ma[k], None if mb is None else mb[k])
        ib, sb = nearest(b[k], a[k], None if mb is None else mb[k], None if ma is None else ma[k])
        for o, v in zip(out, (ia, ib, sa, sb)):
            o.append(v)
    return [np.stack(o) for o in out]


# ---- the formulas of the contract in a chosen dtype, at given indices ----------------------------------------------------------
def rho_fn(s, rho):
    r2 = s.dtype.type(rho) * s.dtype.type(rho)
    return s if rho == 0 else r2 * s / (s + r2)


def drho_fn(s, rho):
    r2 = s.dtype.type(rho) * s.dtype.type(rho)
    return np.ones_like(s) if rho == 0 else (r2 * r2) / ((s + r2) * (s + r2))


def direction(q, t, idx, w, g, rho, dtype):
    """One mesh, one direction in `dtype`: (loss, d / d q [Nq, 3], d / d t [Nt, 3]) at the given indices (-1: no term)."""
    q, t = q.astype(dtype), t.astype(dtype)
    ok = idx >= 0
    j = np.where(ok, idx, 0)
    diff = q - t[j]
    s = (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]
    w = np.ones(len(q), dtype) if w is None else w.astype(dtype)
    val = np.where(ok, w * rho_fn(s, rho), 0).astype(dtype)
    gq = (np.where(ok, dtype(g) * w * drho_fn(s, rho) * 2, 0).astype(dtype)[:, None] * diff).astype(dtype)
    gt = np.zeros((len(t), 3), dtype)
    np.add.at(gt, j[ok], -gq[ok])
    return val.sum(dtype=dtype), gq, gt


def term(a, b, idx_ab, idx_ba, wa, wb, g, rho, dtype):
    """One mesh: (loss [2], da [Na, 3], db [Nb, 3]) in `dtype`; g [2] the upstream of the two directions."""
    l0, da0, db0 = direction(a, b, idx_ab, wa, g[0], rho, dtype)
    l1, db1, da1 = direction(b, a, idx_ba, wb, g[1], rho, dtype)
    return np.array([l0, l1], dtype), da0 + da1, db0 + db1


def bound(f32, f64):
    """The yardstick of a float comparison: 10 x the float32 formulas' own error, at least 2^-22 of the largest magnitude."""
    f64 = np.asarray(f64, np.float64)
    return max(10.0 * float(np.abs(np.asarray(f32, np.float64) - f64).max()), 2.0 ** -22 * float(np.abs(f64).max()))


# ---- exact: the gradient rows in the device's order ------------------------------------------------------------------------------
def seg_len(n):
    return n if n <= SERIAL_MAX else (n + SEGMENTS - 1) // SEGMENTS


def _coef(g, w, s32, rho):
    r2 = np.float64(np.float32(rho)) * np.float64(np.float32(rho))
    s = np.float64(s32)
    d = (r2 * r2) / ((s + r2) * (s + r2)) if rho > 0 else np.float64(1.0)
    return ((np.float64(np.float32(g)) * np.float64(w)) * d) * 2.0


def _s32(p, q):
    d = p - q                                      # float32
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def rows_exact(X, Y, idx_own, idx_in, wx, wy, g_own, g_in, rho, sequential=False):
    """float32 [Nd, 3]: the rows of destination set X (one mesh) as sfx_chamfer_backward forms them.  idx_own [Nd]: X's nearest
    targets in Y (the gather term), idx_in [Nq]: Y's nearest targets in X (the scatter terms).  sequential: one segment whatever
    the length -- the plain ascending sum."""
    Nd, Nq = len(X), len(Y)
    order = np.argsort(np.where((idx_in >= 0) & (idx_in < Nd), idx_in, Nd), kind="stable")
    keys = np.where((idx_in >= 0) & (idx_in < Nd), idx_in, Nd)[order]
    starts = np.searchsorted(keys, np.arange(Nd + 1))
    out = np.zeros((Nd, 3), np.float32)
    X64, Y64 = X.astype(np.float64), Y.astype(np.float64)
    for r in range(Nd):
        row = np.zeros(3)
        t = idx_own[r]
        if 0 <= t < Nq:
            row = _coef(g_own, 1.0 if wx is None else wx[r], _s32(X[r], Y[t]), rho) * (X64[r] - Y64[t])
        lst = order[starts[r]:starts[r + 1]]
        if len(lst):
            step = len(lst) if sequential else seg_len(len(lst))
            for k0 in range(0, len(lst), step):
                p = np.zeros(3)
                for q in lst[k0:k0 + step]:
                    p = p + -(_coef(g_in, 1.0 if wy is None else wy[q], _s32(Y[q], X[r]), rho) * (Y64[q] - X64[r]))
                row = row + p
        out[r] = row.astype(np.float32)
    return out
