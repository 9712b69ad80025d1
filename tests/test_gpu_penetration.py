"""Interpenetration term (csrc/collide.hip) against the oracle (oracle/penetration.py) --
candidate pairs, loss and vertex gradient -- on small meshes and on the synthetic SMPL-X mesh."""
import numpy as np
import pytest
import torch

import helpers as H
from oracle import penetration as OP

# bounds of the stand-alone operator: ~10 x the maxima observed on MI355X in round 6 (loss 2.1e-7, vertex gradient 5.1e-5 over 29 checks;
# the session summary prints them: helpers.check_bound)
from smplifyx_amd import engine

pytestmark = pytest.mark.gpu


def _sphere(n_lat, n_lon, center, radius):
    """Closed triangulated sphere: vertices [V,3], faces [F,3]."""
    vs = [[0, 0, 1.0]]
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        for j in range(n_lon):
            ph = 2 * np.pi * j / n_lon
            vs.append([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
    vs.append([0, 0, -1.0])
    vs = np.asarray(vs) * radius + np.asarray(center)
    fs = []
    ring = lambda i, j: 1 + (i - 1) * n_lon + (j % n_lon)
    for j in range(n_lon):
        fs.append([0, ring(1, j), ring(1, j + 1)])
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            fs.append([ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)])
            fs.append([ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)])
    last = len(vs) - 1
    for j in range(n_lon):
        fs.append([last, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)])
    return vs, np.asarray(fs, np.int64)


def _two_spheres(offset):
    v0, f0 = _sphere(10, 16, [0, 0, 0], 0.10)
    v1, f1 = _sphere(9, 14, [offset, 0.01, 0.02], 0.08)
    verts = np.concatenate([v0, v1])
    faces = np.concatenate([f0, f1 + len(v0)])
    segm = np.concatenate([np.zeros(len(f0), np.int64), 2 * np.ones(len(f1), np.int64)])
    parents = np.concatenate([-np.ones(len(f0), np.int64), np.ones(len(f1), np.int64)])   # part 2's parent is part 1
    return verts, faces, segm, parents


def _pairs_from_gpu(pen, B):
    """ordered partner lists -> set of unordered pairs per frame (debug read-back through torch)."""
    return pen.stats(B)


@pytest.mark.parametrize("sigma,outside", [(0.5, True), (0.5, False), (1e-3, True), (1e-4, True)])     # 1e-4: the cfgs' df_cone_height
def test_two_spheres_loss_and_gradient(sigma, outside):
    verts, faces, segm, parents = _two_spheres(0.13)
    B = 3
    rng = np.random.RandomState(0)
    vb = np.stack([verts + 0.004 * rng.normal(size=verts.shape) * (b > 0) + [0.01 * b, 0, 0] for b in range(B)])
    pen = engine.Penetration(len(verts), faces, segm, parents, max_collisions=64, max_batch=B)
    loss, dv = pen.eval(torch.tensor(vb, dtype=torch.float32, device="cuda"), sigma, outside)
    st = pen.stats(B)
    assert np.all(st["dropped"] == 0) and np.all(st["entry_overflow"] == 0)
    loss, dv = loss.cpu().numpy(), dv.cpu().numpy()
    for b in range(B):
        v32 = vb[b].astype(np.float32).astype(np.float64)
        lo, go, pairs = OP.penetration(v32, faces, segm, parents, None, sigma=sigma, penalize_outside=outside)
        assert st["pairs"][b] == 2 * len(pairs), (b, st["pairs"][b], len(pairs))
        assert len(pairs) > 50
        H.check_bound("operator", "loss", abs(loss[b] - lo) / max(abs(lo), 1e-30), 5e-6)
        H.check_bound("operator", "vertex gradient", np.linalg.norm(dv[b] - go) / max(np.linalg.norm(go), 1e-30), 6e-4)


@pytest.mark.parametrize("sigma,outside", [(0.5, True), (0.5, False), (1e-4, True)])
def test_point2plane_loss_and_gradient(sigma, outside):
    """DistanceFieldPenetrationLoss(point2plane=True) (cmd_parser.py:239; oracle/penetration.py assumption A6): every
    Psi^2 of a pair weighted by (n_f . n_g)^2, gradient through Psi and through both normals -- against fp64 autograd of
    the oracle; the flag changes the value (it is not the default form rescaled) and switching it off again restores the
    default form bit for bit."""
    verts, faces, segm, parents = _two_spheres(0.13)
    B = 3
    rng = np.random.RandomState(1)
    vb = np.stack([verts + 0.004 * rng.normal(size=verts.shape) * (b > 0) + [0.01 * b, 0, 0] for b in range(B)])
    t = torch.tensor(vb, dtype=torch.float32, device="cuda")
    pen = engine.Penetration(len(verts), faces, segm, parents, max_collisions=64, max_batch=B)
    l0, d0 = pen.eval(t, sigma, outside)
    l0, d0 = l0.cpu().numpy(), d0.cpu().numpy()
    loss, dv = pen.eval(t, sigma, outside, point2plane=True)
    st = pen.stats(B)
    assert np.all(st["dropped"] == 0) and np.all(st["entry_overflow"] == 0)
    loss, dv = loss.cpu().numpy(), dv.cpu().numpy()
    for b in range(B):
        v32 = vb[b].astype(np.float32).astype(np.float64)
        lo, go, pairs = OP.penetration(v32, faces, segm, parents, None, sigma=sigma, penalize_outside=outside, point2plane=True)
        assert st["pairs"][b] == 2 * len(pairs) and len(pairs) > 50
        H.check_bound("operator", "loss", abs(loss[b] - lo) / max(abs(lo), 1e-30), 5e-6)
        H.check_bound("operator", "vertex gradient", np.linalg.norm(dv[b] - go) / max(np.linalg.norm(go), 1e-30), 6e-4)
        assert 0 < loss[b] < 0.98 * l0[b], (loss[b], l0[b])               # (n_f . n_g)^2 < 1 on most pairs of two spheres
        # not the default gradient rescaled: the normals carry gradient of their own
        cosang = float((dv[b] * d0[b]).sum() / (np.linalg.norm(dv[b]) * np.linalg.norm(d0[b])))
        assert cosang < 0.9999, cosang
    l1, d1 = pen.eval(t, sigma, outside)
    assert np.array_equal(l1.cpu().numpy(), l0) and np.array_equal(d1.cpu().numpy(), d0)


def test_part_filter_and_separated_meshes():
    verts, faces, segm, parents = _two_spheres(0.13)
    t = torch.tensor(verts[None], dtype=torch.float32, device="cuda")
    # same part everywhere -> nothing collides; parent/child parts -> nothing; ignored pair -> nothing
    for sg, pr, ign in ((np.zeros_like(segm), -np.ones_like(parents), None),
                        (segm, np.where(segm == 2, 0, -1), None),
                        (segm, parents, ["0,2"])):
        pen = engine.Penetration(len(verts), faces, sg, pr, ign, max_collisions=64, max_batch=1)
        loss, dv = pen.eval(t, 0.5)
        assert float(loss[0]) == 0.0 and float(dv.abs().max()) == 0.0 and pen.stats(1)["pairs"][0] == 0
    # far apart: no candidates at all
    v2, f2, s2, p2 = _two_spheres(0.5)
    pen = engine.Penetration(len(v2), f2, s2, p2, max_collisions=64, max_batch=1)
    loss, dv = pen.eval(torch.tensor(v2[None], dtype=torch.float32, device="cuda"), 0.5)
    assert float(loss[0]) == 0.0 and pen.stats(1)["pairs"][0] == 0
    # without labels every non-adjacent overlapping pair counts (self-collisions of one sphere included)
    pen = engine.Penetration(len(verts), faces, max_collisions=128, max_batch=1)
    pen.eval(t, 0.5)
    pairs = OP.candidate_pairs(verts.astype(np.float32), faces)
    assert pen.stats(1)["pairs"][0] == 2 * len(pairs) > 0


def test_mis_shaped_vertices_are_refused_before_any_launch():
    """eval / eval_pairs hand the library a pointer and V: vertices of another count, another dtype or on the host are a
    ValueError (a TypeError when no tensor at all), not a read past the buffer -- also under `python -O`, which is why these are
    no asserts.  The checks come before the first call into the library, so nothing is launched here."""
    verts, faces, segm, parents = _two_spheres(0.13)
    V = len(verts)
    pen = engine.Penetration(V, faces, segm, parents, max_collisions=64, max_batch=1)
    good = torch.tensor(verts[None], dtype=torch.float32, device="cuda")
    pairs = torch.zeros(1, 4, 2, dtype=torch.int32, device="cuda")
    for bad, msg in ((good[:, :V - 1], "shape"), (good.double(), "float32"), (good.cpu(), "no CPU fallback"), (good[0], "shape")):
        with pytest.raises(ValueError, match="verts.*" + msg):
            pen.eval(bad, 0.5)
        with pytest.raises(ValueError, match="verts.*" + msg):
            pen.eval_pairs(bad, pairs, 0.5)
    with pytest.raises(TypeError, match="verts"):
        pen.eval(verts[None].astype(np.float32), 0.5)
    for bad, msg in ((pairs.long(), "int32"), (pairs.cpu(), "no CPU fallback"), (pairs[:, :, :1], "shape"),
                     (torch.zeros(2, 4, 2, dtype=torch.int32, device="cuda"), "shape")):
        with pytest.raises(ValueError, match="pairs.*" + msg):
            pen.eval_pairs(good, bad, 0.5)
    pen.close()


def test_max_collisions_cap_keeps_the_lowest_ids():
    """A triangle with more than max_collisions partners keeps the max_collisions LOWEST triangle ids -- a rule on ids,
    not on which pair a wavefront happened to find first --, a pair counts only if both triangles kept each other, and
    the gradient is the exact gradient of the loss over the kept pairs.  Against the oracle's statement of the same
    rule (pairs, loss, gradient), at the cfgs' cone height, and bit for bit whatever else is in the batch."""
    verts, faces, segm, parents = _two_spheres(0.13)
    v32 = verts.astype(np.float32)
    pairs = OP.candidate_pairs(v32.astype(np.float64), faces, segm, parents)
    cnt = np.bincount(pairs.reshape(-1), minlength=len(faces))
    cap = int((cnt.max() + 1) // 2)               # binds for many triangles, and every list still fits the 2 x cap buffer
    assert (cnt > cap).sum() >= 10 and cnt.max() <= 2 * cap
    opairs, n_cut = OP.ordered_pairs_capped(pairs, cap)
    assert n_cut > 0 and len(opairs) == 2 * len(pairs) - n_cut
    sym = set(map(tuple, opairs.tolist()))
    assert all((g, f) in sym for f, g in sym)                       # kept by both sides
    for sigma in (1e-4, 0.5):
        vt = torch.tensor(v32.astype(np.float64), dtype=torch.float64, requires_grad=True)
        lo = OP.penetration_loss_ordered(vt, faces, opairs, sigma)
        lo.backward()
        go = vt.grad.numpy()
        pen = engine.Penetration(len(verts), faces, segm, parents, max_collisions=cap, max_batch=3)
        rng = np.random.RandomState(3)
        others = np.stack([v32 + 0.003 * rng.normal(size=v32.shape).astype(np.float32) for _ in range(2)])
        res = []
        for batch in (v32[None], np.concatenate([others[:1], v32[None], others[1:]])):
            loss, dv = pen.eval(torch.tensor(batch, device="cuda"), sigma)
            i = 0 if batch.shape[0] == 1 else 1
            st = pen.stats(batch.shape[0])
            assert st["pairs"][i] == len(opairs) and st["dropped"][i] == n_cut, (st, len(opairs), n_cut)
            res.append((float(loss[i]), dv[i].cpu().numpy()))
        assert res[0][0] == res[1][0] and np.array_equal(res[0][1], res[1][1])          # batch composition
        H.check_bound("operator", "loss", abs(res[0][0] - float(lo)) / max(abs(float(lo)), 1e-30), 5e-6)
        H.check_bound("operator", "vertex gradient", np.linalg.norm(res[0][1] - go) / max(np.linalg.norm(go), 1e-30), 6e-4)


def test_lists_beyond_twice_the_cap_are_derived_from_the_grid_again():
    """A triangle with MORE than 2 x max_collisions partners (its list holds only the first 2 x cap arrivals) gets its kept
    partners from a second look at the grid (collide.hip pen_rewalk): the cap lowest ids, like every other triangle -- pairs,
    cut partners, loss and gradient against the oracle's statement of the rule, identical from run to run and whatever else
    is in the batch, and nothing is reported as order dependent."""
    verts, faces, segm, parents = _two_spheres(0.13)
    v32 = verts.astype(np.float32)
    pairs = OP.candidate_pairs(v32.astype(np.float64), faces, segm, parents)
    cnt = np.bincount(pairs.reshape(-1), minlength=len(faces))
    cap = max(2, int(cnt.max()) // 5)
    assert (cnt > 2 * cap).sum() >= 10, (cnt.max(), cap)          # many lists overflow what is held while they are collected
    opairs, n_cut = OP.ordered_pairs_capped(pairs, cap)
    assert n_cut > 0
    for sigma in (1e-4, 0.5):
        vt = torch.tensor(v32.astype(np.float64), dtype=torch.float64, requires_grad=True)
        lo = OP.penetration_loss_ordered(vt, faces, opairs, sigma)
        lo.backward()
        go = vt.grad.numpy()
        pen = engine.Penetration(len(verts), faces, segm, parents, max_collisions=cap, max_batch=3)
        rng = np.random.RandomState(5)
        others = np.stack([v32 + 0.003 * rng.normal(size=v32.shape).astype(np.float32) for _ in range(2)])
        res = []
        for batch in (v32[None], np.concatenate([others[:1], v32[None], others[1:]]), v32[None]):
            loss, dv = pen.eval(torch.tensor(batch, device="cuda"), sigma)
            i = 0 if batch.shape[0] == 1 else 1
            st = pen.stats(batch.shape[0])
            assert st["pairs"][i] == len(opairs) and st["dropped"][i] == n_cut, (st, len(opairs), n_cut)
            res.append((float(loss[i]), dv[i].cpu().numpy()))
        for r in res[1:]:
            assert res[0][0] == r[0] and np.array_equal(res[0][1], r[1])               # batch composition, run to run
        H.check_bound("operator", "loss", abs(res[0][0] - float(lo)) / max(abs(float(lo)), 1e-30), 5e-6)
        H.check_bound("operator", "vertex gradient", np.linalg.norm(res[0][1] - go) / max(np.linalg.norm(go), 1e-30), 6e-4)


def test_max_collisions_cap_is_reported():
    verts, faces, segm, parents = _two_spheres(0.13)
    pen = engine.Penetration(len(verts), faces, segm, parents, max_collisions=2, max_batch=1)
    pen.eval(torch.tensor(verts[None], dtype=torch.float32, device="cuda"), 0.5)
    st = pen.stats(1)
    assert st["dropped"][0] > 0 and st["pairs"][0] <= 2 * len(faces)


def test_synthetic_smplx_mesh(synth_model):
    """The 20908-face synthetic SMPL-X mesh with synthetic part labels and the cfg's ignored pairs
    (cfg_files/fit_smplx_combined_halpe.yaml): pair count, loss and gradient vs the oracle."""
    from smplifyx_amd import synthetic
    parts = synthetic.make_synthetic_parts(synth_model)
    ign = ["9,16", "9,17", "6,16", "6,17", "1,2", "12,22"]
    v = np.asarray(synth_model["v_template"], np.float32)
    f = np.asarray(synth_model["f"]).astype(np.int64)
    pen = engine.Penetration(len(v), f, parts["segm"], parts["parents"], ign, max_collisions=128, max_batch=2)
    vb = np.stack([v, v * np.array([1.0, 1.0, 0.9], np.float32)])
    loss, dv = pen.eval(torch.tensor(vb, device="cuda"), 0.01)
    st = pen.stats(2)
    assert np.all(st["dropped"] == 0) and np.all(st["entry_overflow"] == 0)
    lo, go, pairs = OP.penetration(v.astype(np.float64), f, parts["segm"], parts["parents"], ign, sigma=0.01)
    assert st["pairs"][0] == 2 * len(pairs)
    assert abs(float(loss[0]) - lo) <= 5e-4 * abs(lo)
    g = dv[0].cpu().numpy()
    assert np.linalg.norm(g - go) <= 5e-3 * np.linalg.norm(go)
    # frame 1 (a different pose of the same mesh) is independent of frame 0
    loss1, dv1 = pen.eval(torch.tensor(vb[1:], device="cuda"), 0.01)
    assert float(loss1[0]) == float(loss[1]) and torch.equal(dv1[0], dv[1])


@pytest.mark.parametrize("point2plane", [False, True])
def test_closure_with_interpenetration_matches_oracle(synth_model, point2plane):
    """cfg_files/fit_smplx_combined_halpe.yaml with its interpenetration term (coll_loss_weights
    [0, 0.1, 1.0], max_collisions 128, ign_part_pairs) inside the fitting closure, dense path:
    total loss and gradient with respect to the 182 optimisation variables vs oracle autograd
    (oracle SMPL-X forward -> brute-force pairs -> cone field).  df_cone_height is raised from the
    cfg's 1e-4 to 1e-2 for the tight comparison (at 1e-4 the field's quadratic branch has a 2.5e7
    coefficient and fp32 vs fp64 agree to ~1e-2 only -- checked loosely at the end)."""
    import helpers as H
    import test_gpu_parity as T
    from smplifyx_amd import synthetic
    cfg = H.load_cfg("fit_smplx_combined_halpe.yaml", use_hands=False, use_face=False, interpenetration=True)
    assert cfg["interpenetration"] and cfg["coll_loss_weights"] == [0.0, 0.1, 1.0] and cfg["max_collisions"] == 128
    cfg["df_cone_height"] = 1e-2
    cfg["point2plane"] = point2plane  # cmd_parser.py:239 (the shipped cfgs: False); True: oracle/penetration.py assumption A6
    cfg["max_collisions"] = 1024      # the synthetic triangle soup: curled fingers give some triangles > 128 partners;
                                      # which partners a cap keeps is implementation defined, so the comparison avoids it
    parts = synthetic.make_synthetic_parts(synth_model)
    dm = T._dm(synth_model, cfg)
    dm.set_parts(parts["segm"], parts["parents"], cfg["ign_part_pairs"])
    B = 2
    K = len(H.joint_map_for(cfg))
    frames = synthetic.make_frames(B, H.oracle_joints_fn(synth_model, cfg), K, focal=5000.0)
    fb = H.engine_batch_from_frames(dm, cfg, frames, range(B), lbs_mode="dense")
    rng = np.random.RandomState(21)
    P = H.random_params(rng, B, scale=0.2)
    # near the rest pose: the synthetic mesh is a volumetric triangle soup around the bones, and a
    # bent limb sweeps hundreds of thousands of pairs (more than max_collisions per triangle)
    P["pose_embedding"] = (0.03 * rng.normal(size=(B, 63))).astype(np.float32)
    P["global_orient"] = frames["reg_global"] + 0.1 * rng.normal(size=(B, 3)).astype(np.float32)
    P["cam_translation"] = (frames["cam_t"] + 0.3 * rng.normal(size=(B, 3))).astype(np.float32)
    est = (frames["cam_t"][:, 2] + 1.0).astype(np.float32)
    kp = frames["keypoints"]
    jw = np.tile(H.base_joint_weights(cfg, K), (B, 1))
    fb.set_frames(kp, jw, np.zeros((B, K), np.float32), frames["focal"],
                  np.tile([frames["W"] * 0.5, frames["H"] * 0.5], (B, 1)), 1000.0 / frames["H"], est_tz=est)
    fb.set_params(regression_pose=frames["reg_pose"], **P)
    P["est_tz"] = est
    faces = np.asarray(synth_model["f"]).astype(np.int64)

    def oracle(i, stage, with_pen):
        import helpers
        ff_make = helpers.oracle_frame_fit
        def patched(model, c, fr, idx, dtype=torch.float64):
            ff = ff_make(model, c, fr, idx, dtype=dtype)
            if with_pen:
                ff.set_penetration(faces, parts["segm"], parts["parents"], cfg["ign_part_pairs"])
            return ff
        helpers.oracle_frame_fit = patched
        try:
            return T._oracle_closure(synth_model, cfg, frames, i, P, stage)
        finally:
            helpers.oracle_frame_fit = ff_make

    # stage 0: coll weight 0 -> the term is off; stages 1, 2: on
    l0, g0 = fb.closure(0)
    lo, go = oracle(0, 0, False)
    assert abs(l0[0] - lo) <= 2e-5 * abs(lo)
    for stage in (1, 2):
        loss, grad = fb.closure(stage)
        st = fb.penetration_stats()
        assert np.all(st["dropped"] == 0) and np.all(st["entry_overflow"] == 0) and np.all(st["vertices"] > 0), st
        i = stage - 1
        lo, go = oracle(i, stage, True)
        lo_np, _ = oracle(i, stage, False)
        assert lo - lo_np > 1e-3 * lo                                  # the term matters in this pose
        # (looser than the keypoint terms' 1e-5 / 1e-4: the cone field amplifies the 1e-7 m between two fp32 skinnings, LAB_NOTES §4.6)
        H.check_closure("pen-body-dense", stage, loss[i], lo, grad[i], go, loss_tol=1e-4, grad_tol=2e-3)
        assert np.all(grad[i][13:13 + 63] == 0)                        # dead body_pose parameter
    fb.close()


def test_interpenetration_at_the_cfg_values(synth_model):
    """cfg_files/fit_smplx_combined_halpe.yaml's own df_cone_height 1e-4 and max_collisions 128 inside the closure
    (dense path), on the surface-like synthetic mesh (the bench's `pen` workload; the random triangle soup of the other
    tests puts thousands of partners on a triangle).

    At sigma = 1e-4 the field measures heights in units of 0.1 mm: moving the vertices by 1e-7 m (the difference between
    the fp32 GEMM's vertices and the oracle's fp64 ones) changes the term's VERTEX gradient by 1.3 % and, after the
    cancellation inside J^T, its parameter gradient by tens of per cent (measured with the oracle alone:
    tools/pen_sens.py) -- the term is that ill conditioned in any fp32 implementation.  So it is compared where it is well
    defined: on the device's OWN vertices (read back) -- pair set, cut partners, loss and vertex gradient against the
    oracle in fp64 with the tolerances of the stand-alone operator tests; J^T is covered by
    test_dense_skinning_adjoint_matches_torch_reference; the closure's total has to agree with the oracle's to the
    accuracy the term's loss has (eps / sigma = 1e-3 relative of the term)."""
    import helpers as H
    import test_gpu_parity as T
    from smplifyx_amd import synthetic
    model = synthetic.make_synthetic_model(0, surface=True)
    cfg = H.load_cfg("fit_smplx_combined_halpe.yaml", use_hands=False, use_face=False, interpenetration=True)
    assert cfg["df_cone_height"] == 1e-4 and cfg["max_collisions"] == 128 and cfg["coll_loss_weights"] == [0.0, 0.1, 1.0]
    parts = synthetic.make_synthetic_parts(model)
    dm = T._dm(model, cfg)
    dm.set_parts(parts["segm"], parts["parents"], cfg["ign_part_pairs"])
    B = 2
    K = len(H.joint_map_for(cfg))
    frames = synthetic.make_frames(B, H.oracle_joints_fn(model, cfg), K, focal=5000.0)
    fb = H.engine_batch_from_frames(dm, cfg, frames, range(B), lbs_mode="dense")
    rng = np.random.RandomState(21)
    P = H.random_params(rng, B, scale=0.2)
    P["pose_embedding"] = (frames["reg_pose"] + 0.05 * rng.normal(size=(B, 63))).astype(np.float32)
    P["global_orient"] = frames["reg_global"] + 0.1 * rng.normal(size=(B, 3)).astype(np.float32)
    P["cam_translation"] = (frames["cam_t"] + 0.3 * rng.normal(size=(B, 3))).astype(np.float32)
    est = (frames["cam_t"][:, 2] + 1.0).astype(np.float32)
    jw = np.tile(H.base_joint_weights(cfg, K), (B, 1))
    fb.set_frames(frames["keypoints"], jw, np.zeros((B, K), np.float32), frames["focal"],
                  np.tile([frames["W"] * 0.5, frames["H"] * 0.5], (B, 1)), 1000.0 / frames["H"], est_tz=est)
    fb.set_params(regression_pose=frames["reg_pose"], **P)
    P["est_tz"] = est
    faces = np.asarray(model["f"]).astype(np.int64)

    def oracle(i, stage, with_pen):
        import helpers
        ff_make = helpers.oracle_frame_fit
        def patched(model_, c, fr, idx, dtype=torch.float64):
            ff = ff_make(model_, c, fr, idx, dtype=dtype)
            if with_pen:
                ff.set_penetration(faces, parts["segm"], parts["parents"], cfg["ign_part_pairs"])
            return ff
        helpers.oracle_frame_fit = patched
        try:
            return T._oracle_closure(model, cfg, frames, i, P, stage)
        finally:
            helpers.oracle_frame_fit = ff_make

    for stage in (1, 2):
        loss, grad = fb.closure(stage)
        st = fb.penetration_stats()
        assert np.all(st["entry_overflow"] == 0)
        vd = fb.debug_read("verts").reshape(B, -1, 3).astype(np.float64)
        pl = fb.debug_read("pen_loss")[:, 0]
        pg = fb.debug_read("pen_dverts").reshape(B, -1, 3)
        for i in range(B):
            pairs = OP.candidate_pairs(vd[i], faces, parts["segm"], parts["parents"], cfg["ign_part_pairs"])
            cnt = np.bincount(pairs.reshape(-1), minlength=len(faces))
            assert cnt.max() <= 256, cnt.max()         # (every list fits the collection buffer: the cut is then a rule on ids)
            opairs, n_cut = OP.ordered_pairs_capped(pairs, 128)
            assert len(opairs) > 500
            assert st["pairs"][i] == len(opairs) and st["dropped"][i] == n_cut, (stage, i, st, len(opairs), n_cut)
            vt = torch.tensor(vd[i], dtype=torch.float64, requires_grad=True)
            lo_v = OP.penetration_loss_ordered(vt, faces, opairs, 1e-4)
            lo_v.backward()
            H.check_bound("operator", "loss", abs(pl[i] - float(lo_v)) / max(abs(float(lo_v)), 1e-30), 5e-6)
            gv = vt.grad.numpy()
            H.check_bound("operator", "vertex gradient", np.linalg.norm(pg[i] - gv) / max(np.linalg.norm(gv), 1e-30), 6e-4)
        i = stage - 1
        lo, go = oracle(i, stage, True)
        lo_np, go_np = oracle(i, stage, False)
        pen_part = lo - lo_np
        assert pen_part > 1e-4 * lo, (pen_part, lo)
        assert abs(loss[i] - lo) <= 5e-3 * pen_part + 2e-5 * abs(lo_np), (stage, loss[i], lo, lo_np)
        assert np.all(np.isfinite(grad)) and np.all(grad[i][13:13 + 63] == 0)
    fb.close()


def test_dense_skinning_adjoint_matches_torch_reference(synth_model):
    _dense_skinning_adjoint(synth_model, False)


def test_dense_skinning_adjoint_matches_torch_reference_dense_weights(synth_model):
    """The same on helpers.dense_weights_model (the first test keeps the name it had, and so has no parameter): the vertices
    with more than SFX_NW weights take the full-row branch of collide_eval.h's adjoint (wj[0] == -1) and k_adj_finish walks
    per-joint vertex lists several times the base model's.  No partner is dropped and no grid cell overflows at this pose,
    and at least 1000 vertices with more than 8 weights carry a gradient (observed on MI355X: 129 488 .. 183 118 ordered pairs
    per frame, 6 060 .. 6 528 vertices with a gradient, 3 181 .. 3 437 of them with more than 8 weights)."""
    import helpers as H
    _dense_skinning_adjoint(H.dense_weights_model(synth_model), True)


def _dense_skinning_adjoint(synth_model, dense):
    """The adjoint of the dense skinning in isolation (d v_posed = T^T g written by k_pen_gather -> fp32-MFMA split-K GEMM
    k_lbs_dense_adj -> k_adj_finish: partial sums and d A): from the evaluation's own vertex gradient g, skinning transforms A,
    v_posed and the model constants, a plain torch fp64 restatement of
        d feat[k] = sum_{v,c} dirs[k][3v+c] (T_v^T g_v)[c],   T_v = sum_j W[v][j] A_j
        d A_j     = sum_v W[v][j] g_v (x) [v_posed_v; 1]
    must agree with what the kernels wrote.  Tolerance 2e-5 relative (fp32 accumulation over 31 425 terms)."""
    import helpers as H
    import test_gpu_parity as T
    from smplifyx_amd import synthetic
    cfg = H.load_cfg("fit_smplx_combined_halpe.yaml", use_hands=False, use_face=False, interpenetration=True)
    cfg["df_cone_height"] = 1e-2
    cfg["max_collisions"] = 1024
    parts = synthetic.make_synthetic_parts(synth_model)
    dm = T._dm(synth_model, cfg)
    dm.set_parts(parts["segm"], parts["parents"], cfg["ign_part_pairs"])
    B = 3
    K = len(H.joint_map_for(cfg))
    frames = synthetic.make_frames(B, H.oracle_joints_fn(synth_model, cfg), K, focal=5000.0)
    fb = H.engine_batch_from_frames(dm, cfg, frames, range(B), lbs_mode="dense")
    rng = np.random.RandomState(5)
    P = H.random_params(rng, B, scale=0.2)
    P["pose_embedding"] = (0.05 * rng.normal(size=(B, 63))).astype(np.float32)
    fb.set_params(regression_pose=frames["reg_pose"], **P)
    fb.closure(2)
    g = fb.debug_read("pen_dverts").reshape(B, -1, 3).astype(np.float64)
    A = fb.debug_read("A").reshape(B, 3, 4, 55).astype(np.float64)            # [b][row][col][joint]
    vp = fb.debug_read("vposed").reshape(B, -1, 3).astype(np.float64)
    dfeat = fb.debug_read("pen_dfeat")
    dA = fb.debug_read("pen_dA").reshape(B, 55, 3, 4)
    assert np.abs(g).max() > 0
    W = np.asarray(synth_model["weights"], np.float64)                         # [V][55]
    st = fb.penetration_stats()
    many = ((W != 0).sum(1) > 8)[None] & np.any(g != 0, axis=2)
    print("pairs %s dropped %s entry_overflow %s; vertices with a gradient %s, of them with more than 8 weights %s" %
          (st["pairs"], st["dropped"], st["entry_overflow"], np.any(g != 0, axis=2).sum(1), many.sum(1)))
    if dense:
        assert np.all(st["dropped"] == 0) and np.all(st["entry_overflow"] == 0), st
        assert many.any(0).sum() >= 1000, many.sum(1)
    V = W.shape[0]
    nb, ne = cfg["num_betas"], cfg["num_expression_coeffs"]
    sd = np.asarray(synth_model["shapedirs"], np.float64)
    dirs = np.concatenate([sd[:, :, :nb], sd[:, :, 300:300 + ne] if sd.shape[2] > 300 else sd[:, :, nb:nb + ne],
                           np.asarray(synth_model["posedirs"], np.float64).reshape(V, 3, -1)], axis=2)      # [V][3][506]
    for b in range(B):
        T_v = np.einsum("vj,rcj->vrc", W, A[b])                                # [V][3][4]
        dvp = np.einsum("vrc,vr->vc", T_v[:, :, :3], g[b])
        ref_feat = np.einsum("vck,vc->k", dirs, dvp)
        err = np.linalg.norm(dfeat[b, :ref_feat.size] - ref_feat) / np.linalg.norm(ref_feat)
        assert err < 2e-5, (b, err)
        assert np.all(dfeat[b, ref_feat.size:] == 0)
        hom = np.concatenate([vp[b], np.ones((V, 1))], 1)
        ref_dA = np.einsum("vj,vr,vc->jrc", W, g[b], hom)
        errA = np.linalg.norm(dA[b] - ref_dA) / np.linalg.norm(ref_dA)
        assert errA < 2e-5, (b, errA)
    fb.close()


def test_dense_skinning_adjoint_does_not_depend_on_the_launch_shape():
    """A column's d feat must not depend on how many other columns are active: k_lbs_dense_adj splits the reduction over
    r into ranges of 512 per wavefront when the launch has three or more 64-frame tiles and of 256 otherwise -- both
    launches form the same chunk / pair / group sums (lbs_adjoint.hip), so the same frames give the same bits in a batch of
    3 (one tile, 256) and of 200 (four tiles, 512).  Also d A, the loss and the closure's gradient."""
    import helpers as H
    import test_gpu_parity as T
    from smplifyx_amd import synthetic
    model = synthetic.make_synthetic_model(0, surface=True)
    cfg = H.load_cfg("fit_smplx_combined_halpe.yaml", use_hands=False, use_face=False, interpenetration=True)
    parts = synthetic.make_synthetic_parts(model)
    dm = T._dm(model, cfg)
    dm.set_parts(parts["segm"], parts["parents"], cfg["ign_part_pairs"])
    K = len(H.joint_map_for(cfg))
    n = 3
    frames = synthetic.make_frames(n, H.oracle_joints_fn(model, cfg), K, focal=5000.0)
    rng = np.random.RandomState(5)
    P = H.random_params(rng, n, scale=0.2)
    P["pose_embedding"] = (0.05 * rng.normal(size=(n, 63))).astype(np.float32)
    got = {}
    for B in (n, 200):
        idx = [i % n for i in range(B)]
        fb = H.engine_batch_from_frames(dm, cfg, frames, idx, lbs_mode="dense")
        fb.set_params(regression_pose=frames["reg_pose"][idx], **{k: v[idx] for k, v in P.items()})
        loss, grad = fb.closure(2)
        got[B] = (fb.debug_read("pen_dfeat")[:n].copy(), fb.debug_read("pen_dA")[:n].copy(), loss[:n].copy(), grad[:n].copy(),
                  fb.debug_read("pen_dfeat"))
        fb.close()
    assert np.abs(got[n][0]).max() > 0
    for q in range(4):
        assert np.array_equal(got[n][q], got[200][q]), q
    assert np.array_equal(got[200][4][:n], got[200][4][n:2 * n])          # and not on the column index either


def test_fit_frames_with_interpenetration_runs(synth_model):
    """driver.fit_frames on cfg_files/fit_smplx_combined_halpe.yaml with interpenetration=True: the whole
    schedule runs on device with the penetration step between the dense LBS and the loss/adjoint
    pass; the stages with weight 0 are untouched, the others end on a higher loss (the synthetic
    triangle soup always interpenetrates)."""
    import helpers as H
    import test_gpu_parity as T
    from smplifyx_amd import driver, synthetic
    cfg = H.load_cfg("fit_smplx_combined_halpe.yaml", use_hands=False, use_face=False, interpenetration=True)
    cfg.update(use_camera_prior=False, maxiters=4, df_cone_height=1e-2)
    parts = synthetic.make_synthetic_parts(synth_model)
    dm = T._dm(synth_model, cfg)
    dm.set_parts(parts["segm"], parts["parents"], cfg["ign_part_pairs"])
    K = len(H.joint_map_for(cfg))
    frames = synthetic.make_frames(2, H.oracle_joints_fn(synth_model, cfg), K, focal=5000.0)
    jw = H.base_joint_weights(cfg, K)
    res = driver.fit_frames(dm, cfg, frames["keypoints"], jw, 600, 800, 5000.0, reg_pose=frames["reg_pose"],
                            reg_global=frames["reg_global"], lbs_mode="dense")
    cfg0 = dict(cfg); cfg0["interpenetration"] = False
    ref = driver.fit_frames(dm, cfg0, frames["keypoints"], jw, 600, 800, 5000.0, reg_pose=frames["reg_pose"],
                            reg_global=frames["reg_global"], lbs_mode="dense")
    assert np.all(np.isfinite(res["stage_loss"])) and np.all(np.isfinite(res["pose_embedding"]))
    # camera stage and body stage 0 (coll weight 0) do not see the term (the two runs use closure
    # variants with different fp32 summation orders: equal to rounding); the later stages do
    assert np.allclose(res["stage_loss"][:, :2], ref["stage_loss"][:, :2], rtol=1e-4)
    assert np.all(res["stage_loss"][:, 2:] > ref["stage_loss"][:, 2:] * 1.001)
    with pytest.raises(ValueError, match="dense"):
        driver.fit_frames(dm, cfg, frames["keypoints"], jw, 600, 800, 5000.0, reg_pose=frames["reg_pose"],
                          reg_global=frames["reg_global"], lbs_mode="rows")


def test_pooled_batch_with_interpenetration():
    """A job of more frames than GEMM columns (slots < B) WITH the interpenetration term: the collision buffers hold one mesh
    per column of the pool, so (i) the fit through the pool equals the resident fit bit for bit, (ii) a stand-alone closure
    on the pooled batch (one column per frame: more meshes than the buffers hold) walks the columns in chunks and returns
    the same loss and gradient as a resident batch -- it used to ignore the operator's "batch exceeds the capacity" and
    build the gradient from stale buffers --, (iii) the diagnostics cover every frame.  On the surface-like synthetic mesh:
    the triangle soup overflows the partner lists (more than 2 x max_collisions partners), where arrival order decides."""
    import helpers as H
    import test_gpu_parity as T
    from smplifyx_amd import driver, engine, synthetic
    model = synthetic.make_synthetic_model(0, surface=True)
    cfg = H.load_cfg("fit_smplx_combined_halpe.yaml", use_hands=False, use_face=False, interpenetration=True)
    cfg.update(use_camera_prior=False, maxiters=3)
    parts = synthetic.make_synthetic_parts(model)
    dm = T._dm(model, cfg)
    dm.set_parts(parts["segm"], parts["parents"], cfg["ign_part_pairs"])
    K = len(H.joint_map_for(cfg))
    B, slots = 70, 32
    frames = synthetic.make_frames(B, H.oracle_joints_fn(model, cfg), K, focal=5000.0)
    jw = H.base_joint_weights(cfg, K)
    kw = dict(reg_pose=frames["reg_pose"], reg_global=frames["reg_global"], lbs_mode="dense")
    res_pool = driver.fit_frames(dm, cfg, frames["keypoints"], jw, 600, 800, 5000.0, slots=slots, **kw)
    res_all = driver.fit_frames(dm, cfg, frames["keypoints"], jw, 600, 800, 5000.0, **kw)
    res_again = driver.fit_frames(dm, cfg, frames["keypoints"], jw, 600, 800, 5000.0, **kw)
    # A triangle that meets more than 2 x max_collisions partners in some trial pose keeps the ones that ARRIVE first (LAB_NOTES §4.6):
    # such a frame is not reproducible run to run, whatever the batch, and the engine says which ones they are
    # (result key 'pen_order_dependent', sticky per frame over the fit).  Every other frame must come out of the pool, and out
    # of a second resident run, with the same bits.
    keys = ("stage_loss", "pose_embedding", "betas", "cam_translation", "global_orient", "stage_evals")
    same = lambda a, b_: np.array([all(np.array_equal(a[k][i], b_[k][i], equal_nan=True) for k in keys) for i in range(B)])
    clean = ~(res_all["pen_order_dependent"] | res_pool["pen_order_dependent"] | res_again["pen_order_dependent"])
    assert clean.all(), np.flatnonzero(~clean)            # (round 4: overflowing partner lists are derived from the grid again; only a cut bucket walk is flagged)
    assert same(res_again, res_all)[clean].all(), np.flatnonzero(~same(res_again, res_all) & clean)
    assert same(res_pool, res_all)[clean].all(), np.flatnonzero(~same(res_pool, res_all) & clean)
    assert np.all(res_all["stage_evals"][:, 2:] > 0)
    # stand-alone closure of the last stage (collision weight 1.0) on a pooled batch vs a resident one, same parameters
    out = {}
    for name, s_ in (("pool", slots), ("all", 0)):
        fb, _ = driver._make_batch(dm, cfg, frames["keypoints"], jw, 600, 800, 5000.0, frames["reg_pose"], frames["reg_global"],
                                   None, None, "dense", True, slots=s_)
        loss, grad = fb.closure(fb.n_stages - 1)
        st = fb.penetration_stats()
        out[name] = (loss, grad, st)
        fb.close()
    assert np.array_equal(out["pool"][0], out["all"][0]) and np.array_equal(out["pool"][1], out["all"][1])
    assert np.array_equal(out["pool"][2]["pairs"], out["all"][2]["pairs"]) and out["all"][2]["pairs"].shape == (B,)
    assert (out["all"][2]["pairs"] > 0).sum() > B // 2          # the tubes of neighbouring bones run through each other: the term was evaluated


@H.requires_lab()
def test_chunked_pair_tests_equal_the_unchunked_walk(tmp_path):
    """k_pen_walk / k_pen_walk2 (round 4: a block's walk through its bucket in chunks of 64 steps, the chunks beyond the first as
    one flat list over all meshes) against the walk that runs every bucket to its end on the block's own wavefront
    (SFX_PEN_WALK_CHUNKS_OFF=1), and the flat pair evaluation against the per-mesh grid (SFX_PEN_FLAT_OFF=1): same pairs, same
    loss, same gradient, bit for bit.  The mesh is built to make the chunks matter: 1 500 small triangles of two parts inside ONE
    grid cell (a bucket of 1 500 entries: 24 chunks per block) next to a sparse cloud of large ones, three meshes with
    different content in one call (the flat lists cross mesh boundaries).  max_collisions 1024 so that no partner list overflows."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r'''
import json, sys, numpy as np, torch
sys.path.insert(0, %r)
from smplifyx_amd import engine
rng = np.random.RandomState(0)
def mesh(n_dense, n_sparse, seed):
    r = np.random.RandomState(seed)
    c = np.concatenate([0.2 * r.rand(n_dense, 3), 4.0 * r.rand(n_sparse, 3) + 1.0])        # one crowded cell + a sparse cloud of
    sg = np.concatenate([np.full(n_dense, 0.01), np.full(n_sparse, 0.15)])                # large triangles (they set the cell size)
    tri = c[:, None, :] + sg[:, None, None] * r.randn(len(c), 3, 3)
    return tri.reshape(-1, 3).astype(np.float32)
nd, ns = 1500, 1000
F = nd + ns
faces = np.arange(F * 3).reshape(F, 3)
segm = (np.arange(F) %% 2).astype(np.int64); parents = np.full(F, -1, np.int64)
verts = np.stack([mesh(nd, ns, s) for s in (1, 2, 3)])
verts[1, : nd * 3 // 2] += 10.0           # the second mesh: half of the crowd moved away
pen = engine.Penetration(F * 3, faces, segm=segm, parents=parents, max_collisions=1024, max_batch=3)
loss, dv = pen.eval(torch.tensor(verts, device="cuda"), 0.01, True)
st = pen.stats(3)
print(json.dumps({"loss": [float(x).hex() for x in loss.cpu().numpy()], "pairs": st["pairs"].tolist(), "dropped": st["dropped"].tolist(),
                  "cut": st["walks_cut"].tolist(), "grad_sum": float(np.abs(dv.cpu().numpy().astype(np.float64)).sum()).hex(),
                  "grad_hash": hash(dv.cpu().numpy().tobytes()) & 0xffffffff}))
''' % root
    outs = {}
    for name, env_extra in (("chunked", {}), ("unchunked", {"SFX_PEN_WALK_CHUNKS_OFF": "1", "SFX_PEN_FLAT_OFF": "1"})):
        env = dict(os.environ, PYTHONHASHSEED="0", **env_extra)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[name] = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    a, b = outs["chunked"], outs["unchunked"]
    assert a["pairs"][0] > 3000 and a["pairs"][1] < a["pairs"][0] and a["dropped"] == [0, 0, 0] and a["cut"] == [0, 0, 0], a
    assert a == b, (a, b)


@H.requires_lab()
def test_phase_clocks_columns_are_the_documented_slots():
    """The read-out of sfx_pen_phase_clocks as csrc/collide_slots.h documents it (PenClockCol): only k_pen_narrow stamps -- the
    ends of its phases D-G in columns 3-6 -- columns 0-2 and 7-8 have no writer, column 9 is the count of cut walks sfx_pen_stats
    reports and column 10 the grid entries the work counters sum.  Two overlapping spheres (offset 0.13, as in
    test_two_spheres_loss_and_gradient: a few hundred pairs per mesh, which form 1 keeps in its per-column workgroup), B = 2."""
    verts, faces, segm, parents = _two_spheres(0.13)
    B = 2
    vb = np.stack([verts + [0.01 * b, 0, 0] for b in range(B)]).astype(np.float32)
    prev = engine.pen_form(1)
    try:
        pen = engine.Penetration(len(verts), faces, segm, parents, max_collisions=64, max_batch=B)
        engine.pen_work_reset()
        pen.eval(torch.tensor(vb, device="cuda"), 0.5, True)
        pc, st, work = pen.phase_clocks(B), pen.stats(B), engine.pen_work_get()
        pen.close()
    finally:
        engine.pen_form(prev)
    print("phase clocks (us | counts):", pc.tolist(), "pairs", st["pairs"].tolist(), "entries", work["entries"])
    assert pc.shape == (B, 11) and np.all(st["pairs"] > 100)
    assert np.all(pc[:, [0, 1, 2, 7, 8]] == 0)
    assert np.all(np.diff(pc[:, 3:7], axis=1) >= 0) and np.all(pc[:, 6] > 0)
    assert np.array_equal(pc[:, 9], st["walks_cut"])
    assert pc[:, 10].sum() == work["entries"] and work["entries"] > 0


def test_operator_matches_the_reference_lines_golden():
    """The device operator against numbers the REFERENCE's own lines produced: tests/golden/objective_pen.npz holds
    SMPLifyLoss.forward's total with the collision weight at 0 and at 0.1 (fitting.py:437-455 over the CPU stand-ins of the absent
    package) and d total / d vertices; their difference is 0.1 x the term on that mesh."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "objective_pen.npz"))
    verts, faces = g["verts"].astype(np.float32), g["faces"].astype(np.int64)
    ref_loss = (float(g["w01_total"]) - float(g["w0_total"])) / 0.1
    ref_grad = g["w01_d_vertices"][0] / 0.1
    pen = engine.Penetration(len(verts), faces, g["w01_segm"].astype(np.int64), g["parents"].astype(np.int64), ["0,1"],
                             max_collisions=128, max_batch=1)
    loss, dv = pen.eval(torch.tensor(verts[None], device="cuda"), 0.01)
    st = pen.stats(1)
    assert st["dropped"][0] == 0 and st["pairs"][0] > 200
    # (the golden's vertices are fp64; the device rounds them to fp32: 1e-7 relative on the coordinates, amplified by 1 / sigma = 100)
    H.check_bound("operator-vs-reference-lines", "loss", abs(float(loss[0]) - ref_loss) / ref_loss, 2e-4)
    H.check_bound("operator-vs-reference-lines", "vertex gradient",
                  np.linalg.norm(dv[0].cpu().numpy() - ref_grad) / np.linalg.norm(ref_grad), 2e-3)
    # nothing between parts that never collide: one part for every triangle
    pen1 = engine.Penetration(len(verts), faces, np.zeros(len(faces), np.int64), g["parents"].astype(np.int64), None, max_collisions=128, max_batch=1)
    l1, d1 = pen1.eval(torch.tensor(verts[None], device="cuda"), 0.01)
    assert float(l1[0]) == 0.0 and float(d1.abs().sum()) == 0.0 and np.abs(g["nopairs_d_vertices"]).sum() == 0
    pen.close(); pen1.close()
