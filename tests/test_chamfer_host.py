"""CPU tests of the chamfer term's surface (sfx_chamfer_forward / sfx_chamfer_backward, engine.chamfer_eval / chamfer_backward,
pointcloud.ChamferLoss): the declarations and their bindings, the unit's flags, what is refused before any launch, and the
header csrc/chamfer_math.h itself -- tests/chamfer_math_check.cpp, a stand-alone program compiled for the host only with
AddressSanitizer and UBSan, evaluates the header on cases written here and numpy checks what it wrote.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import chamfer_common as CC
from smplifyx_amd import _capi, engine, pointcloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smplify-x-partial_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ENTRY_POINTS = ("sfx_chamfer_forward", "sfx_chamfer_backward")


def _t(*shape):
    return torch.zeros(*shape, dtype=torch.float32)


def _declaration(hdr, name):
    m = re.search(r"\bint\s+%s\s*\((.*?)\);" % name, hdr, flags=re.S)
    return re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)


def test_header_declares_both_entries_once_and_states_the_contract():
    hdr = open(os.path.join(ROOT, "include", "sfx.h")).read()
    for name in ENTRY_POINTS:
        assert len(re.findall(r"\bint\s+%s\s*\(" % name, hdr)) == 1, name
        assert name in _capi.SYMBOLS, name
    # the section sits after sfx_eval_nearest (tests/test_evaluation_device_host.py slices the text before it)
    assert hdr.index("int  sfx_eval_nearest") < hdr.index("int  sfx_chamfer_forward") < hdr.index("int  sfx_chamfer_backward")
    doc = hdr[hdr.index("int  sfx_eval_nearest"):hdr.index("int  sfx_chamfer_forward")].rsplit("/*", 1)[-1]
    for phrase in ("ties go to the lowest index", "((dx dx + dy dy) + dz dz)", "No float atomics", "no fused multiply-add",
                   "utils.py:92-95", "point-to-vertex"):
        assert phrase in doc, phrase
    assert re.search(r"#define SFX_CHAMFER_MAX_POINTS \(1 << 26\)", hdr) and engine.CHAMFER_MAX_POINTS == 1 << 26


def test_bindings_take_the_arguments_the_header_declares():
    hdr = open(os.path.join(ROOT, "include", "sfx.h")).read()
    lib = _capi.load()
    for name in ENTRY_POINTS:
        assert len(_capi.SYMBOLS[name][1]) == len(_declaration(hdr, name).split(",")), name
        assert hasattr(lib, name)


def test_scratch_formulas_mirror_the_header():
    hdr = open(os.path.join(ROOT, "include", "sfx.h")).read()
    for macro, fn in (("SFX_CHAMFER_FORWARD_SCRATCH_BYTES", engine.chamfer_forward_scratch_bytes),
                      ("SFX_CHAMFER_BACKWARD_SCRATCH_BYTES", engine.chamfer_backward_scratch_bytes)):
        body = re.search(r"#define %s\(B, Na, Nb\)\s+(.*)" % macro, hdr).group(1)
        expr = re.sub(r"\(int64_t\)", "", body)
        for B, Na, Nb in ((1, 1, 1), (3, 513, 1025), (256, 10475, 10475), (16, 10475, 50000)):
            assert eval(expr, dict(B=B, Na=Na, Nb=Nb)) == fn(B, Na, Nb), (macro, B, Na, Nb)


def test_units_list_names_chamfer_once_without_contraction_and_the_math_has_a_header_of_its_own():
    lines = [l.split() for l in open(os.path.join(CSRC, "units.txt")) if l.strip() and not l.startswith("#")]
    mine = [l for l in lines if l[0] == "chamfer"]
    assert len(mine) == 1 and "-ffp-contract=off" in mine[0][1:]
    assert os.path.exists(os.path.join(CSRC, "chamfer.hip"))
    math = open(os.path.join(CSRC, "chamfer_math.h")).read()
    assert "hip_runtime" not in math and not re.search(r"\bhip[A-Z]\w+\(", math)       # no HIP runtime call in it
    unit = open(os.path.join(CSRC, "chamfer.hip")).read()
    assert '#include "chamfer_math.h"' in unit
    code = re.sub(r"//.*", "", unit)
    assert not re.search(r"atomicAdd\(\s*&?\s*\(?\s*(float|double)", code) and "atomicAdd_f" not in code and "unsafeAtomic" not in code
    assert (CC.SERIAL_MAX, CC.SEGMENTS) == tuple(int(re.search(r"#define %s (\d+)" % n, math).group(1)) for n in ("CH_SERIAL_MAX", "CH_SEGMENTS"))


def test_chamfer_eval_refuses_before_any_launch():
    a, b = _t(2, 5, 3), _t(2, 7, 3)
    with pytest.raises(ValueError, match="no CPU fallback"):
        engine.chamfer_eval(a, b)
    with pytest.raises(TypeError, match="torch tensor"):
        engine.chamfer_eval(a.numpy(), b)
    with pytest.raises(TypeError, match="torch tensor"):
        engine.chamfer_eval(a, b.numpy())
    with pytest.raises(ValueError, match=r"b: shape \(3, 7, 3\)"):
        engine.chamfer_eval(a, _t(3, 7, 3))
    with pytest.raises(ValueError, match=r"a: shape \(2, 5, 2\)"):
        engine.chamfer_eval(_t(2, 5, 2), b)
    with pytest.raises(ValueError, match=r"mask_b: shape \(2, 5\)"):
        engine.chamfer_eval(a, b, mask_b=torch.ones(2, 5, dtype=torch.bool))
    with pytest.raises(ValueError, match="torch.bool or torch.uint8"):
        engine.chamfer_eval(a, b, mask_a=torch.ones(2, 5))
    with pytest.raises(ValueError, match=r"weight_a: shape \(2, 7\)"):
        engine.chamfer_eval(a, b, weight_a=_t(2, 7))
    with pytest.raises(TypeError, match="weight_b: a torch tensor"):
        engine.chamfer_eval(a, b, weight_b=np.ones((2, 7), np.float32))
    for rho in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="rho"):
            engine.chamfer_eval(a, b, rho=rho)


def test_chamfer_backward_refuses_before_any_launch():
    a, b = _t(2, 5, 3), _t(2, 7, 3)
    fwd = dict(idx_ab=torch.zeros(2, 5, dtype=torch.int32), idx_ba=torch.zeros(2, 7, dtype=torch.int32))
    g = _t(2, 2)
    with pytest.raises(ValueError, match="no CPU fallback"):
        engine.chamfer_backward(a, b, fwd, g)
    with pytest.raises(TypeError, match="torch tensor"):
        engine.chamfer_backward(a.numpy(), b, fwd, g)
    with pytest.raises(ValueError, match=r"b: shape \(2, 7\)"):
        engine.chamfer_backward(a, _t(2, 7), fwd, g)
    with pytest.raises(ValueError, match="want"):
        engine.chamfer_backward(a, b, fwd, g, want=("c",))
    with pytest.raises(ValueError, match="want"):
        engine.chamfer_backward(a, b, fwd, g, want=())
    with pytest.raises(ValueError, match="rho"):
        engine.chamfer_backward(a, b, fwd, g, rho=-1.0)
    with pytest.raises(ValueError, match="torch.bool or torch.uint8"):
        engine.chamfer_backward(a, b, fwd, g, mask_b=torch.ones(2, 7))


def test_chamfer_loss_refuses_before_any_launch():
    with pytest.raises(ValueError, match="reduction"):
        pointcloud.ChamferLoss(reduction="median")
    for rho in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="rho"):
            pointcloud.ChamferLoss(rho=rho)
    loss = pointcloud.ChamferLoss(rho=0.05)
    v, p = _t(2, 5, 3), _t(2, 7, 3)
    with pytest.raises(ValueError, match="no CPU fallback"):
        loss(v, p)
    with pytest.raises(ValueError, match="no CPU fallback"):
        loss(v.double(), p.double())
    with pytest.raises(TypeError, match="vertices: a torch tensor"):
        loss(v.numpy(), p)
    with pytest.raises(TypeError, match="points: a torch tensor"):
        loss(v, p.numpy())
    with pytest.raises(ValueError, match=r"shape \(2, 5\)"):
        loss(_t(2, 5), p)
    with pytest.raises(ValueError, match=r"mask_b: shape \(2, 5\)"):
        loss(v, p, point_mask=torch.ones(2, 5, dtype=torch.bool))
    with pytest.raises(ValueError, match="torch.bool or torch.uint8"):
        loss(v, p, vertex_mask=torch.ones(2, 5))
    assert "float32" in pointcloud.ChamferLoss.__doc__ and "point-to-point" in pointcloud.__doc__


# ---- the header itself ---------------------------------------------------------------------------------------------------------
def _index_cases():
    rng = np.random.RandomState(11)
    cases = [(rng.randint(0, 40, size=300).astype(np.int32), 40),                 # ordinary
             (np.r_[rng.randint(0, 9, size=50), [3] * 0].astype(np.int32), 12),   # buckets 9 .. 11 empty
             (np.full(200, 4, np.int32), 7),                                      # one bucket holds everything
             (np.array([-1, 2, 5, -1, 2, 9, 0, 7, -3], np.int32), 6),             # -1 and indices that name no target
             (np.full(5, -1, np.int32), 3),                                       # nothing at all
             (np.zeros(0, np.int32), 4)]                                          # no query
    return cases


def test_header_against_numpy(tmp_path):
    exe = str(tmp_path / "chamfer_math_check")
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
                    "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "chamfer_math_check.cpp"), "-o", exe], check=True)
    rng = np.random.RandomState(3)
    pairs = np.concatenate([rng.normal(size=(4000, 6)), rng.normal(size=(500, 6)) * 1e-3 + 1.0, rng.randint(-3, 4, size=(500, 6)),
                            [[0, 0, 0, 0, 0, 0], [1e19, 0, 0, -1e19, 0, 0], [1e-23, 1e-23, 0, 0, 0, 0]]]).astype(np.float32)
    h = 1e-4
    s0 = np.r_[np.exp(rng.uniform(np.log(1e-6), np.log(10.0), size=300)), 0.0].astype(np.float32).astype(np.float64)
    rhos = np.r_[0.0, 0.01, 0.05, 1.0, 100.0].astype(np.float32).astype(np.float64)
    S, R = [x.reshape(-1) for x in np.meshgrid(s0, rhos, indexing="ij")]
    W = rng.uniform(0.0, 2.0, size=S.size).astype(np.float32).astype(np.float64)
    Gu = rng.normal(size=S.size).astype(np.float32).astype(np.float64)
    rho_cases = np.stack([S, R, W, Gu], 1)
    lens = np.r_[np.arange(1, 200), 2049, 4096, 4097, 50000, 1 << 26].astype(np.int32)
    idx_cases = _index_cases()
    with open(str(tmp_path / "cases.bin"), "wb") as f:
        np.array([len(pairs), len(rho_cases), len(lens), len(idx_cases)], "<i4").tofile(f)
        pairs.astype("<f4").tofile(f)
        rho_cases.astype("<f8").tofile(f)
        lens.astype("<i4").tofile(f)
        for idx, nt in idx_cases:
            np.array([len(idx), nt], "<i4").tofile(f)
            idx.astype("<i4").tofile(f)
    r = subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:]
    assert re.fullmatch(r"[1-9]\d* checks, 0 failed", r.stdout.strip().splitlines()[-1])
    raw = open(str(tmp_path / "out.bin"), "rb").read()
    pos = 0

    def take(dtype, n):
        nonlocal pos
        out = np.frombuffer(raw, dtype, n, pos)
        pos += out.nbytes
        return out

    # squared distances: float32 numpy in the same association, bit for bit
    s = take("<f4", len(pairs))
    with np.errstate(over="ignore"):
        d = pairs[:, :3] - pairs[:, 3:]
        want = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert want.dtype == np.float32 and np.array_equal(s.view(np.uint32), want.view(np.uint32))
    assert np.isinf(s[-2]) and s[-1] == 0.0 and s[-3] == 0.0                         # overflow, underflow
    # rho, rho', the per-point value and the gradient factor: float64 numpy
    out = take("<f8", len(rho_cases) * 4).reshape(-1, 4)
    r2 = R * R
    with np.errstate(invalid="ignore", divide="ignore"):
        rho_np = np.where(R > 0, r2 * S / (S + r2), S)
        drho_np = np.where(R > 0, r2 * r2 / ((S + r2) * (S + r2)), 1.0)
    rel = lambda x, y: np.abs(x - y).max() / np.abs(y).max()
    assert np.allclose(out[:, 0], rho_np, rtol=1e-15, atol=0) and np.allclose(out[:, 1], drho_np, rtol=1e-15, atol=0)
    assert np.array_equal(out[:, 2], (W * rho_np).astype(np.float32).astype(np.float64))          # rounded once
    assert np.allclose(out[:, 3], Gu * W * drho_np * 2.0, rtol=1e-15, atol=0)
    print("rho %.1e  rho' %.1e (largest relative difference to numpy)" % (rel(out[:, 0], rho_np), rel(out[:, 1], drho_np)))
    # rho' against a central difference of rho in float64, step = h (s + rho^2).  With rho' = k^2 / (s + k)^2 and
    # rho''' = 6 k^2 / (s + k)^4 (k = rho^2) the truncation error is h^2 rho' exactly to leading order, and the rounding of the
    # two rho values (each <= k, 2^-52 relative) adds at most 2^-52 k / step: relative to rho' that is 2^-52 (s + k) / (k h)
    for rho in rhos[1:]:
        k2 = float(rho) ** 2
        step = h * (s0 + k2)
        f = lambda x: k2 * x / (x + k2)
        cd = (f(s0 + step) - f(s0 - step)) / (2 * step)
        got = out[R == rho, 1]
        tol = 2.0 * h * h + 8.0 * 2.0 ** -52 * (s0 + k2) / (k2 * h)
        assert np.all(np.abs(got - cd) <= tol * np.abs(cd)), (rho, (np.abs(got - cd) / np.abs(cd) / tol).max())
    # the segment rule
    seg = take("<i4", len(lens))
    assert seg.tolist() == [CC.seg_len(int(n)) for n in lens]
    # the inverted index: bucket contents and order against a stable argsort
    for idx, nt in idx_cases:
        off, lst, placed = take("<i4", nt + 1), take("<i4", len(idx)), take("<i4", len(idx))
        ok = (idx >= 0) & (idx < nt)
        order = np.argsort(np.where(ok, idx, nt), kind="stable")[:ok.sum()]
        assert off.tolist() == np.r_[0, np.cumsum(np.bincount(idx[ok], minlength=nt))].tolist()
        assert lst[:ok.sum()].tolist() == order.tolist() and np.all(lst[ok.sum():] == -1)
        assert np.array_equal(placed, lst)
    counts = [np.bincount(i[(i >= 0) & (i < nt)], minlength=nt) for i, nt in idx_cases]
    assert (counts[1] == 0).any() and counts[2].max() == 200 and (counts[2] > 0).sum() == 1       # an empty bucket; one holding all
    assert pos == len(raw)
