"""GPU tests on a model with DENSE skinning weights (run with -m gpu): helpers.dense_weights_model gives whole 16-vertex tiles
8, 9, 12 and 55 nonzero weights per vertex and every vertex a keypoint can read 12, where synthetic.make_synthetic_model has at
most 3.  That runs what no test on the synthetic model reaches: the full-row fallbacks of a vertex with more than SFX_NW = 8
weights (wj[0] == -1: closure_body.h items, collide_eval.h, k_adj_prep), the skinning epilogue of the dense GEMM at up to 14
joint groups per tile, k_adj_finish over long per-joint vertex lists, and the ROW OVERFLOW of csrc/model_tables.h (the dynamic
contour's per-joint lists do not fit their blocks: dynp_js absent, closure_body.h walks dj_*).

  a. forward, all vertices: DeviceModel.lbs_forward against the oracle in float64 and float32 (bounds of test_gpu_parity:
     1e-5 m / 5e-6 m, full pose 1e-6), 24 frames that cover LUT rows 0, 1..38, 39, 40..77 and 78, oracle/lbs_numpy on two of them
  b. every launch shape of the dense GEMM against the 16-frame kernel that (a) anchors, bit for bit
  c. v_posed, the vertices and the self-served blend offsets of a dense-mode batch at 33 and 81 columns
  d. the closure, rows and dense, at LUT rows 0, 1..38 and 40..78 (bounds of helpers: 4e-6 / 6e-6 / per block)

Observed on MI355X (the session summary prints every comparison next to its bound):
  a. vertices <= 5.4e-7 m against the float32 oracle and <= 6.0e-7 m against float64 (largest in the 55-weight tiles; the
     model's own tiles 2.1e-7 / 2.3e-7, the last tile 1.4e-7), joints 3.0e-7 / 8.4e-8 m, full pose 2.4e-7; the float32 oracle's
     own error against float64 at these frames: vertices 6.2e-7 m, joints 3.2e-7 m
  b. every shape equal to the 16-frame kernel in every bit
  c. v_posed <= 7.2e-8 m; vertices and self-served offsets equal in every bit
  d. loss <= 1.6e-7, gradient <= 2.0e-7 (rows) / 1.8e-7 (dense).  With the blocks of the rows after an overflowing one left at
     zero (before this file came with its fix to csrc/model_tables.h) the last stage gave, rows and dense alike: LUT row 17 loss
     2.9e-2, gradient 1.7e-1; LUT row 62 loss 9.9e-2, gradient 9.1e-2; LUT row 0 and the stages without face keypoints as above.
"""
import numpy as np
import pytest
import torch

import helpers as H
import test_gpu_parity as T
from oracle import lbs_numpy

pytestmark = pytest.mark.gpu

FWD_NAMES = ("global_orient", "pose_embedding", "betas", "expression", "jaw_pose", "leye_pose", "reye_pose", "left_hand_pose",
             "right_hand_pose")
NECK_Y = 3 * (12 - 1) + 1           # body_pose index of the neck's (joint 12) rotation about y


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def dense_model(synth_model):
    return H.dense_weights_model(synth_model)


@pytest.fixture(scope="module")
def cfg_halpe():
    cfg = H.load_cfg("fit_smplx_combined_halpe.yaml")
    assert cfg["use_hands"] and cfg["use_face"] and cfg["use_face_contour"]
    return cfg


@pytest.fixture(scope="module")
def dm_halpe(gpu, dense_model, cfg_halpe):
    dm = T._dm(dense_model, cfg_halpe)
    yield dm
    dm.close()


# ---- the head yaw the dynamic contour's LUT row is rounded from (oracle/body_model.py dynamic_lmk_rows), in fp64 numpy
def yaw_degrees(global_orient, body_pose):
    full = np.concatenate([np.asarray(global_orient, np.float64).ravel(), np.asarray(body_pose, np.float64).ravel()])
    rel = np.eye(3)
    for j in lbs_numpy.NECK_CHAIN:
        rel = lbs_numpy.rodrigues(full[3 * j:3 * j + 3]) @ rel
    return -np.degrees(np.arctan2(-rel[2, 0], np.hypot(rel[0, 0], rel[1, 0])))


def lut_row_of(deg):
    y = int(np.round(min(deg, 39.0)))
    return 78 if y < -39 else (39 - y if y < 0 else y)


def set_yaw(P, i, deg):
    """Turn frame i's neck about y until its head yaw is `deg` degrees (the other rotations of the chain stay as drawn)."""
    from scipy.optimize import brentq

    def f(a):
        p = P["pose_embedding"][i].astype(np.float64)
        p[NECK_Y] = a
        return yaw_degrees(P["global_orient"][i], p) - deg
    grid = np.linspace(-2.5, 2.5, 201)
    val = np.array([f(a) for a in grid])
    k = np.flatnonzero(np.sign(val[:-1]) != np.sign(val[1:]))
    assert k.size, ("the neck alone cannot turn frame %d to %g degrees" % (i, deg), val.min() + deg, val.max() + deg)
    k = k[np.argmin(np.abs(grid[k]))]           # the smallest turn that does
    P["pose_embedding"][i, NECK_Y] = np.float32(brentq(f, grid[k], grid[k + 1], xtol=1e-10))


def lut_rows(P):
    """LUT row of every frame of P: oracle.body_model.dynamic_lmk_rows in float64 and in float32 and the numpy restatement
    above agree exactly, and no frame sits within 0.001 degrees of a rounding boundary -- the device rounds the same yaw."""
    from oracle.body_model import dynamic_lmk_rows
    B = P["global_orient"].shape[0]
    fp = np.concatenate([P["global_orient"], P["pose_embedding"]], 1)
    deg = np.array([yaw_degrees(P["global_orient"][i], P["pose_embedding"][i]) for i in range(B)])
    rows = np.array([lut_row_of(d) for d in deg])
    for dtype in (torch.float64, torch.float32):
        assert np.array_equal(dynamic_lmk_rows(torch.tensor(fp, dtype=dtype), dtype).numpy(), rows), dtype
    frac = np.abs(deg - np.floor(deg) - 0.5)
    assert np.all((frac > 1e-3) | (np.abs(deg) > 40.0)), deg
    return rows


# ------------------------------------------------------------------------------------------------------------------------
# a. forward, all vertices
_FWD = {}


def forward_frames():
    """24 distinct frames: 0 the exact-zero pose; 1, 2 with body angles scaled by 3 (up to about 2.7 rad); 3 .. 6 turned to head
    yaws 17.3, 55, -17.3 and -55 degrees (LUT rows 17, 39, 56, 78); the rest as helpers.random_params draws them."""
    if "P" not in _FWD:
        rng = np.random.RandomState(3)
        P = H.random_params(rng, 24)
        for k in ("global_orient", "pose_embedding", "jaw_pose", "leye_pose", "reye_pose"):
            P[k][0] = 0
        P["pose_embedding"][1:3] *= 3.0
        for i, deg in ((3, 17.3), (4, 55.0), (5, -17.3), (6, -55.0)):
            set_yaw(P, i, deg)
        _FWD["P"] = P
    return _FWD["P"]


def test_forward_all_vertices_against_fp64(gpu, dense_model, cfg_halpe, dm_halpe):
    """24 frames (two 16-frame slices: k_lbs_dense16c) of the full halpe cfg against the oracle in both precisions and
    oracle/lbs_numpy, every vertex, reported per tile class; figures in the module docstring."""
    P = forward_frames()
    B = P["betas"].shape[0]
    assert B == 24 and abs(P["pose_embedding"][1:3]).max() > 2.0
    rows = lut_rows(P)
    got = set(int(r) for r in rows)
    assert 0 in got and 39 in got and 78 in got and any(1 <= r <= 38 for r in got) and any(40 <= r <= 77 for r in got), sorted(got)
    assert rows[0] == 0 and list(rows[3:7]) == [17, 39, 56, 78], rows
    t = lambda a: torch.tensor(a, device=gpu)
    verts, joints, fp = dm_halpe.lbs_forward(*[t(P[n]) for n in FWD_NAMES])
    verts, joints, fp = verts.cpu().numpy(), joints.cpu().numpy(), fp.cpu().numpy()
    assert joints.shape == (B, 136, 3) and verts.shape == (B, dm_halpe.V, 3)
    v32, j32, f32 = T._oracle_forward(dense_model, cfg_halpe, P, torch.float32)
    v64, j64, f64 = T._oracle_forward(dense_model, cfg_halpe, P, torch.float64)
    label = "dense-weights forward"
    print("%s: the float32 oracle's own error against float64: verts %.2e m, joints %.2e m" %
          (label, np.abs(v32 - v64).max(), np.abs(j32 - j64).max()))
    H.check_bound(label, "full pose vs fp32 oracle", np.abs(fp - f32).max(), 1e-6)
    H.check_bound(label, "joints vs fp32 oracle [m]", np.abs(joints - j32).max(), 5e-6)
    H.check_bound(label, "joints vs fp64 oracle [m]", np.abs(joints - j64).max(), 1e-5)
    # per tile class (helpers.dense_tile_classes: 0 and 5 the model's own rows, 1 .. 4 = 8, 9, 12, 55 weights) and the last,
    # partial tile; the keypoint vertices (12 weights, in tiles of every class) once more by themselves
    V = dm_halpe.V
    vcls = np.repeat(H.dense_tile_classes(V), H.DENSE_TILE)[:V]
    e32, e64 = np.abs(verts - v32).max((0, 2)), np.abs(verts - v64).max((0, 2))
    groups = [("class %d" % c, vcls == c) for c in range(H.DENSE_TILE_CLASSES)]
    groups += [("last tile", np.arange(V) >= V - V % H.DENSE_TILE), ("keypoint vertices", np.isin(np.arange(V), H.keypoint_vertices(dense_model)))]
    assert np.all(np.any([m for _, m in groups[:H.DENSE_TILE_CLASSES]], 0)) and (V % H.DENSE_TILE) == 11
    for name, m in groups:
        assert m.any()
        H.check_bound(label, "verts vs fp32 oracle [m], %s" % name, e32[m].max(), 5e-6)
        H.check_bound(label, "verts vs fp64 oracle [m], %s" % name, e64[m].max(), 1e-5)
    # the second, independent statement of the forward: oracle/lbs_numpy.py (fp64, explicit loops) on a scaled and a turned frame
    for i in (1, 5):
        o = lbs_numpy.forward(dense_model, {("body_pose" if k == "pose_embedding" else k): v[i] for k, v in P.items()},
                              joint_map=H.joint_map_for(cfg_halpe))
        assert o["lut_row"] == rows[i]
        assert np.abs(o["vertices"] - v64[i]).max() < 1e-12 and np.abs(o["joints"] - j64[i]).max() < 1e-12
        H.check_bound(label, "verts vs lbs_numpy [m]", np.abs(verts[i] - o["vertices"]).max(), 1e-5)
        H.check_bound(label, "joints vs lbs_numpy [m]", np.abs(joints[i] - o["joints"]).max(), 1e-5)


# ------------------------------------------------------------------------------------------------------------------------
# b. every launch shape, bit for bit
LAUNCH_B = (1, 16, 17, 32, 33, 64, 65, 80, 81, 96, 97, 128, 129, 144, 145, 160)
_SHAPES = {}


def _shape_frames(gpu, dm):
    """160 distinct random points and their vertices / joints through k_lbs_dense16c in chunks of 16 frames (computed once)."""
    if not _SHAPES:
        P = H.random_params(np.random.RandomState(17), 160)
        ins = [torch.tensor(P[n], device=gpu) for n in FWD_NAMES]
        chunks = [dm.lbs_forward(*[x[i:i + 16] for x in ins], return_full_pose=False)[:2] for i in range(0, 160, 16)]
        _SHAPES.update(ins=ins, verts=torch.cat([c[0] for c in chunks]), joints=torch.cat([c[1] for c in chunks]))
    return _SHAPES


@pytest.mark.parametrize("B", LAUNCH_B)
def test_every_launch_shape_equals_the_16_frame_kernel_bitwise(gpu, dm_halpe, B):
    """launch_lbs_dense16's rule (csrc/lbs_dense.hip) over the slices of 16 frames: 1 .. 2 slices k_lbs_dense16c; 3 .. 4 <4> with
    one frame block; 5 <5>; 6 <3> with two blocks; 7 .. 8 <4> with two; 9 <3> with three; 10 <4> with three, the last one short.
    The kernels are documented as interchangeable bit for bit: every frame of lbs_forward(frames[:B]) equals the same frame
    pushed through in chunks of 16, on all vertices and joints -- no tolerance."""
    S = _shape_frames(gpu, dm_halpe)
    verts, joints, _ = dm_halpe.lbs_forward(*[x[:B] for x in S["ins"]], return_full_pose=False)
    assert torch.isfinite(verts).all() and verts.shape == (B, dm_halpe.V, 3)
    if B > 1:
        assert not torch.equal(verts[0], verts[B - 1])
    bad = (verts != S["verts"][:B]).any(2)
    assert torch.equal(verts, S["verts"][:B]), (B, int(bad.sum()), bad.nonzero()[:4].tolist(),
                                               float((verts - S["verts"][:B]).abs().max()))
    assert torch.equal(joints, S["joints"][:B]), (B, float((joints - S["joints"][:B]).abs().max()))


# ------------------------------------------------------------------------------------------------------------------------
# c. v_posed and the exported offsets of a dense-mode batch
def _oracle_vposed(model, cfg, P):
    """v_posed [B][V][3] of the float64 oracle (the buffers and the Rodrigues formula of oracle/body_model.py, every frame at once)."""
    from oracle.body_model import batch_rodrigues
    bm = H.oracle_model(model, cfg, torch.float64)
    d = lambda a: torch.tensor(a, dtype=torch.float64)
    B = P["betas"].shape[0]
    lh = d(P["left_hand_pose"]) @ bm.left_hand_components
    rh = d(P["right_hand_pose"]) @ bm.right_hand_components
    full = torch.cat([d(P["global_orient"]), d(P["pose_embedding"]), d(P["jaw_pose"]), d(P["leye_pose"]), d(P["reye_pose"]), lh, rh], 1)
    full = full + bm.pose_mean
    v_shaped = bm.v_template + torch.einsum("bl,mkl->bmk", torch.cat([d(P["betas"]), d(P["expression"])], 1), bm.shapedirs)
    R = batch_rodrigues(full.view(-1, 3)).view(B, -1, 3, 3)
    feat = (R[:, 1:] - torch.eye(3, dtype=torch.float64)).reshape(B, -1)
    return (v_shaped + torch.matmul(feat, bm.posedirs).view(B, -1, 3)).numpy()


@pytest.mark.parametrize("B", [33, 81])
def test_vposed_and_exported_offsets_of_a_dense_batch(gpu, synth_model, dense_model, B):
    """33 columns: k_lbs_dense16<4>, one frame block; 81: <3>, two blocks -- inside the 65 .. 192 columns at which the fit loop
    uses the self-served offsets.  Body-only halpe cfg (n_uniq <= 16: one tile of exported vertices), the interpenetration
    buffers attached so that the GEMM writes v_posed of every vertex."""
    from smplifyx_amd import synthetic
    cfg = H.load_cfg("fit_smplx_combined_halpe.yaml", use_hands=False, use_face=False, interpenetration=True)
    parts = synthetic.make_synthetic_parts(dense_model)
    dm = T._dm(dense_model, cfg)
    dm.set_parts(parts["segm"], parts["parents"], cfg["ign_part_pairs"])
    assert 0 < dm.n_uniq <= 16, dm.n_uniq
    frames = T.synth_frames(synth_model, cfg, 3)
    fb = H.engine_batch_from_frames(dm, cfg, frames, [i % 3 for i in range(B)], lbs_mode="dense")
    rng = np.random.RandomState(100 + B)
    P = H.random_params(rng, B, scale=0.5)
    P["pose_embedding"] = (0.3 * rng.normal(size=(B, 63))).astype(np.float32)
    fb.set_params(regression_pose=frames["reg_pose"][[i % 3 for i in range(B)]],
                  cam_translation=np.tile(np.array([[0.0, 0.0, 3.0]], np.float32), (B, 1)), **P)
    fb.closure(0)
    vp = fb.debug_read("vposed").reshape(B, -1, 3)
    verts = fb.debug_read("verts").reshape(B, -1, 3)
    gemm, own = fb.debug_read("uvp"), fb.debug_read("uvp_self")
    fb.close()
    label = "dense-weights batch B=%d" % B
    ref = _oracle_vposed(dense_model, cfg, P)
    H.check_bound(label, "v_posed vs fp64 oracle [m]", np.abs(vp - ref).max(), 5e-6)
    o = lbs_numpy.forward(dense_model, {("body_pose" if k == "pose_embedding" else k): v[B - 1] for k, v in P.items()},
                          joint_map=H.joint_map_for(cfg), use_face_contour=cfg["use_face_contour"])
    assert np.abs(o["v_posed"] - ref[B - 1]).max() < 1e-12
    t = lambda a: torch.tensor(a, device=gpu)
    v_fwd = dm.lbs_forward(*[t(P[n]) for n in FWD_NAMES], return_full_pose=False)[0].cpu().numpy()
    assert np.isfinite(verts).all() and not np.array_equal(verts[0], verts[1])
    assert np.array_equal(verts, v_fwd), (B, np.abs(verts - v_fwd).max())
    assert gemm.shape == own.shape == (B, dm.n_uniq * 3) and np.abs(gemm).max() > 0 and not np.array_equal(gemm[0], gemm[1])
    assert np.array_equal(own, gemm), (B, np.abs(own - gemm).max())
    dm.close()


# ------------------------------------------------------------------------------------------------------------------------
# d. the closure at LUT rows 0, 1 .. 38 and 40 .. 78
YAWS = (0.2, 17.3, -23.3)           # degrees: LUT rows 0, 17 and 62


def _turn_heads(P, est):
    for i, deg in enumerate(YAWS):
        set_yaw(P, i, deg)
    rows = lut_rows(P)
    assert rows[0] == 0 and 1 <= rows[1] <= 38 and 40 <= rows[2] <= 78, rows


@pytest.mark.parametrize("mode", ["rows", "dense"])
def test_closure_on_dense_weights_matches_oracle(gpu, synth_model, dense_model, cfg_halpe, mode):
    """Hands + face + contour on the dense-weights model: every keypoint vertex has 12 weights (the full-row fallback of the
    items, forward and adjoint), and LUT row 0's dynamic vertices carry 612 > nd * SFX_NW = 408 weights -- the row overflow of
    csrc/model_tables.h: no dynp_js, the adjoint walks dj_*, and the forward part of the block of whatever row the head pose
    selects must be there.  Camera stage, first and last body stage (the last one has the face keypoints live).
    Before the blocks of the rows after an overflowing one were filled, the frames at LUT rows 17 and 62 read vertex 0 with
    weight 0 for every contour landmark (figures in the module docstring)."""
    from smplifyx_amd import engine
    last = len(engine.stage_weights_from_cfg(cfg_halpe)[0]) - 1
    assert last >= 1
    T.closure_probe(dense_model, cfg_halpe, mode, "dense-weights-%s" % mode, B=3, seed=11, stages=[-1, 0, last],
                    model_tag="dense-weights", frames=T.synth_frames(synth_model, cfg_halpe, 3), points="far-turned", adjust=_turn_heads)
