"""GPU tests of the wide device optimiser: sfx_opt_wide_* (csrc/opt_wide.hip, csrc/lbfgs_wide.h), engine.WideOptimizer,
optimizers.lbfgs_ls.LBFGS(wide=True).step and FittingMonitor.run_fitting over it -- problems of up to 32768 variables, one
workgroup of 1024 threads each.

Reference, error measure, yardstick and bound: tests/opt_ext_common.py, unchanged (lock-step replay: oracle/lbfgs_machine.
StageMachine in float32 is fed the very evaluations the device consumed; bound = 10 x the error of two arithmetic variants of the
machine, floor 1e-6).  tests/test_opt_wide_host.py asserts on the CPU that the variants stay in lock-step for every configuration
used here, and runs the same state machine header on the CPU.  Every test is tens to a few hundred launches of B workgroups."""
import gc

import numpy as np
import pytest
import torch

import helpers as H
import opt_drive_common as O
import opt_ext_common as X
import opt_wide_common as W
from oracle.lbfgs_machine import StageMachine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")
    return torch.device("cuda:0")


CLS, LABEL = "WideOptimizer", "opt-wide"      # the handle under test: its class in smplifyx_amd.engine, the label of its check_bound lines


def _opt(B, N, **hyper):
    return O.opt(CLS, B, N, **hyper)


_bits, _drive, _family, _check_replay = O.bits, O.drive, O.family, O.check_replay


def _variant_bound(x0, hyper, xs, fs, gs):
    """Where no CPU closure of the loss exists to run the variants on: the two variants fed the same recorded evaluations, error
    against the machine while both still run; bound = 10 x the larger, floor 1e-6 (as test_gpu_opt_ext.py's per-sample test)."""
    yard = 0.0
    for name, v in X.variants(x0, **hyper):
        m = StageMachine(x0, dtype=np.float32, **hyper)
        for k in range(len(xs)):
            if v.done or m.done:
                break
            yard = max(yard, float(np.abs(v.x_trial.astype(np.float64) - m.x_trial).max() / np.abs(m.x_trial).max()))
            v.feed(fs[k], gs[k]); m.feed(fs[k], gs[k])
    return max(X.FLOOR, 10 * yard)


# ---------------------------------------------------------------- 1. the reference's own trajectories
@pytest.mark.parametrize("N", W.GOLDEN_NS)
def test_golden_trajectories(gpu, N):
    """Fed the evaluations of the reference's float32 runs (tests/golden/lbfgs_wide.npz), the device finishes after exactly the
    golden's number of evaluations, returns its result exactly (one of the fed losses) and proposes each next point within the bound."""
    g = W.gold()
    xs, fs, gs = W.golden_evals(N)
    bound = W.golden_bound(N)
    opt = _opt(1, N, **W.GOLDEN_HYPER)
    feed = lambda xt, k: (torch.tensor(fs[k:k + 1], device=gpu), torch.tensor(gs[k], device=gpu).reshape(1, N))
    x0 = np.asarray(g["%d_x0" % N], np.float32).reshape(1, N)
    dxs, _, _, n_done = _drive(opt, x0, feed, limit=len(xs) + 1)
    r = opt.result()
    assert n_done == len(xs) and r["evals"][0] == len(xs) and r["status"][0] == 1
    assert np.float32(r["result"][0]) == np.float32(float(g["%d_res" % N]))
    err = max(float(np.abs(dxs[k, 0].astype(np.float64) - xs[k]).max() / np.abs(xs[k]).max()) for k in range(len(xs)))
    print("N = %d: %d evaluations, worst relative trial-point difference %.2e (bound %.2e)" % (N, len(xs), err, bound))
    H.check_bound("opt-wide golden", "N=%d trial points" % N, err, bound)
    xf = r["x"].cpu().numpy()[0].astype(np.float64)
    gf = g["%d_xf" % N].astype(np.float64)
    H.check_bound("opt-wide golden", "N=%d final point" % N, np.abs(xf - gf).max() / np.abs(gf).max(), bound)
    opt.close()


# ---------------------------------------------------------------- 2. replay on the family
def _family_run(N, hname):
    return O.family_run(CLS, N, hname)


@pytest.mark.parametrize("N,hname", W.WIDE_CONFIGS)
def test_replay_on_the_family(gpu, N, hname):
    """B = 5 problems per configuration (what each size is there for: opt_wide_common.WIDE_CONFIGS)."""
    x0, xs, fs, gs, r, trace, n_done = _family_run(N, hname)
    bound = X.bound(N, hname)
    worst = 0.0
    for b in range(X.NB):
        res = dict(evals=r["evals"][b], status=r["status"][b], result=r["result"][b])
        worst = max(worst, _check_replay("opt-wide family", "N=%d %s trial points" % (N, hname), X.HYPER[hname], x0[b],
                                         xs[:, b], fs[:, b], gs[:, b], res, trace[b], bound))
        n = int(r["evals"][b])
        assert np.array_equal(_bits(r["grad"][b]), _bits(gs[n - 1, b])), "the gradient of the last consumed evaluation"
    assert n_done == r["evals"].max()
    print("N = %d, %s: evaluations %s, worst relative trial-point difference %.2e (bound %.2e)" % (N, hname, r["evals"], worst, bound))


# ---------------------------------------------------------------- 3. batch independence
def test_batch_independence_bit_for_bit(gpu):
    """Each problem of the batch, run alone on the evaluations it consumed in the batch, proposes the same trial points and ends
    with the same result, bit for bit; a finished problem's row of x_trial never moves again; ten more `tell`s after the last
    one has finished change nothing."""
    N, hname = W.INDEPENDENCE_CONFIG
    hyper = X.HYPER[hname]
    x0, xs, fs, gs, r, _, n_done = _family_run(N, hname)
    ev = r["evals"]
    assert len(set(ev.tolist())) >= 2, ("the problems must finish at different evaluations", ev)
    for b in range(X.NB):
        n = int(ev[b])
        assert (_bits(xs[n:, b]) == _bits(r["x"][b])).all(), "the row of a finished problem holds its accepted point"
        alone = _opt(1, N, **hyper)
        feed = lambda xt, k: (torch.tensor(fs[k, b:b + 1], device=gpu), torch.tensor(gs[k, b:b + 1], device=gpu))
        axs, _, _, a_done = _drive(alone, x0[b:b + 1], feed)
        ra = alone.result()
        assert a_done == n and ra["evals"][0] == n
        assert np.array_equal(_bits(axs[:, 0]), _bits(xs[:n, b])), ("trial points", b)
        assert np.array_equal(_bits(ra["result"]), _bits(r["result"][b:b + 1]))
        assert np.array_equal(_bits(ra["x"].cpu().numpy()[0]), _bits(r["x"][b]))
        alone.close()
    # over-running: ten evaluations nobody needs
    opt = _opt(X.NB, N, **hyper)
    oxs, _, _, o_done = _drive(opt, x0, _family(), extra=10)
    assert o_done == n_done and len(oxs) == n_done + 10
    assert np.array_equal(_bits(oxs[:n_done]), _bits(xs)), "the batch run is reproducible"
    assert (_bits(oxs[n_done:]) == _bits(r["x"])).all()
    assert opt.active() == 0
    ro = opt.result()
    assert np.array_equal(ro["evals"], ev) and np.array_equal(_bits(ro["result"]), _bits(r["result"]))
    assert np.array_equal(_bits(ro["x"].cpu().numpy()), _bits(r["x"])) and np.array_equal(_bits(ro["grad"].cpu().numpy()), _bits(r["grad"]))
    opt.close()


# ---------------------------------------------------------------- 4. step mode
def test_step_mode_equals_fit_mode(gpu):
    """opt_drive_common.step_mode_equals_fit_mode at N = 4097."""
    O.step_mode_equals_fit_mode(CLS, 4097)


# ---------------------------------------------------------------- 5. a non-finite evaluation
def test_a_nan_loss_ends_one_problem_only(gpu):
    """opt_drive_common.nan_loss_ends_one_problem_only: opt_ext_common.NAN_CONFIG through the wide handle."""
    assert X.NAN_CONFIG in W.WIDE_CONFIGS
    O.nan_loss_ends_one_problem_only(CLS, LABEL + " family")


# ---------------------------------------------------------------- 6. the Python surface
def _lbfgs(params, **kw):
    from smplifyx_amd.optimizers.lbfgs_ls import LBFGS
    return LBFGS(params, line_search_fn="strong_Wolfe", **kw)


def _recording_closure(params, B, b0=0):
    """A closure on GPU tensors over the family (problems b0 .. b0 + B - 1 of the flattened parameters) that records what it saw."""
    rec = []

    def closure():
        for p in params:
            p.grad = None
        x = torch.cat([p.reshape(B, -1) for p in params], 1)
        a = ((torch.arange(x.shape[1], device=x.device) % 10 + 1) ** 2).to(torch.float32)
        c = (0.3 + 0.05 * torch.arange(b0, b0 + B, device=x.device, dtype=torch.float32)).reshape(B, 1)
        loss = 0.5 * (a * (x - c) ** 2).sum(1) + 0.1 * torch.sin(3 * x).sum(1)
        loss.sum().backward()
        rec.append((x.detach().cpu().numpy().copy(), loss.detach().cpu().numpy().copy(),
                    torch.cat([p.grad.reshape(B, -1) for p in params], 1).cpu().numpy().copy()))
        return loss if B > 1 else loss.reshape(())
    return closure, rec


def _replay_surface(what, rec, b, hyper, result):
    xs, fs, gs = (np.stack([r[i][b] for r in rec]) for i in range(3))
    bound = _variant_bound(xs[0], hyper, xs, fs, gs)
    m = StageMachine(xs[0], dtype=np.float32, **hyper)
    err, lock = X.replay(m, xs, fs, gs)
    assert lock, (what, b, len(xs), m.done)
    if result is not None:
        assert X.same_result(result, m.result), (what, result, m.result)
    print("%s, problem %d: %d evaluations, trial points off by %.2e (bound %.2e)" % (what, b, len(xs), err, bound))
    H.check_bound("opt-wide surface", what, err, bound)
    return m


def _groups(lens):
    return [(int(o), int(n), True) for o, n in zip(np.cumsum([0] + list(lens[:-1])), lens)]


STEP = dict(maxiters=1, ftol=0.0, gtol=0.0, lr=1.0, max_iter=20)      # ONE LBFGS.step = run_fitting with maxiters = 1, its own tests off


def test_lbfgs_wide_step_and_run_fitting(gpu):
    """LBFGS([x1000], wide=True).step: returns the entry loss, leaves the accepted point in x and the last gradient in x.grad, and the
    evaluations its closure saw replay through the machine; the same for FittingMonitor.run_fitting over such an optimiser."""
    from smplifyx_amd import engine, fitting
    N = 1000
    x0 = torch.tensor(X.family_x0(N, 0), device=gpu)
    x = x0.clone().requires_grad_(True)
    closure, rec = _recording_closure([x], 1)
    opt = _lbfgs([x], lr=1.0, max_iter=20, wide=True)
    loss = opt.step(closure)
    assert isinstance(opt._ext, engine.WideOptimizer)
    assert torch.is_tensor(loss) and loss.dim() == 0 and float(loss) == float(rec[0][1][0])
    assert np.array_equal(_bits(x.grad.cpu().numpy()), _bits(rec[-1][2][0])), "x.grad holds the last evaluation's gradient"
    m = _replay_surface("LBFGS(wide).step N=1000", rec, 0, STEP, None)
    assert np.float32(m.records[-2][1]) == np.float32(float(loss))
    assert any(np.array_equal(_bits(x.detach().cpu().numpy()), _bits(r[0][0])) for r in rec), "the accepted point is one of the evaluated points"
    # run_fitting: the host loop over optimizer.step
    with torch.no_grad():
        x.copy_(x0)
    x.grad = None
    del rec[:]
    mon = fitting.FittingMonitor(maxiters=6, ftol=1e-9, gtol=1e-9)
    with mon:
        res = mon.run_fitting(_lbfgs([x], lr=1.0, max_iter=20, wide=True), closure, [x], None, 0, use_vposer=False)
    assert res is not None
    _replay_surface("run_fitting over LBFGS(wide) N=1000", rec, 0, dict(maxiters=6, ftol=1e-9, gtol=1e-9, lr=1.0, max_iter=20), res)


def test_lbfgs_wide_many_tensors_and_per_sample(gpu):
    """20 tensors of 50 (more than the narrow path's 12 tensors); per_sample=True on [4, 300]; and wide=True within the narrow
    limits ([65]) is the narrow path: the same bits as wide=False."""
    from smplifyx_amd import engine
    x0 = X.family_x0(1000, 1)
    ps = [torch.tensor(x0[50 * i:50 * i + 50], device=gpu).requires_grad_(True) for i in range(20)]
    closure, rec = _recording_closure(ps, 1)
    opt = _lbfgs(ps, lr=1.0, max_iter=20, wide=True)
    loss = opt.step(closure)
    assert isinstance(opt._ext, engine.WideOptimizer) and float(loss) == float(rec[0][1][0])
    _replay_surface("LBFGS(wide).step 20 tensors of 50", rec, 0, dict(STEP, groups=_groups([50] * 20)), None)
    # per sample
    B, n = 4, 300
    xb = torch.tensor(np.stack([X.family_x0(n, b) for b in range(B)]), device=gpu).requires_grad_(True)
    closure, rec = _recording_closure([xb], B)
    opt = _lbfgs([xb], lr=1.0, max_iter=20, wide=True, per_sample=True)
    entry = opt.step(closure)
    assert tuple(entry.shape) == (B,) and np.array_equal(_bits(entry.cpu().numpy()), _bits(rec[0][1]))
    evals = opt._ext.result()["evals"]
    for b in range(B):
        _replay_surface("LBFGS(wide, per_sample).step [4, 300]", [r for r in rec[:int(evals[b])]], b, STEP, None)
    # within the narrow limits
    outs = []
    for wide in (False, True):
        x = torch.tensor(X.family_x0(65, 2), device=gpu).requires_grad_(True)
        closure, rec = _recording_closure([x], 1)
        opt = _lbfgs([x], lr=1.0, max_iter=20, wide=wide)
        loss = opt.step(closure)
        assert type(opt._ext) is engine.BatchOptimizer
        outs.append((x.detach().cpu().numpy().copy(), float(loss), np.stack([r[0][0] for r in rec])))
    assert np.array_equal(_bits(outs[0][0]), _bits(outs[1][0])) and outs[0][1] == outs[1][1] and np.array_equal(_bits(outs[0][2]), _bits(outs[1][2]))


# ---------------------------------------------------------------- 7. the user story
def test_one_shape_over_a_clip(gpu, synth_model):
    """4 frames of the synthetic differentiable SMPL-X: one betas [1, 10] shared by the clip, global_orient and body_pose per frame
    -- 274 variables in one problem --, a torch loss on the joints plus a frame-to-frame smoothness term, through run_fitting.
    The evaluations the closure saw replay through the machine in lock-step; the returned loss is below the first evaluation's."""
    from smplifyx_amd import fitting, smplx, utils as U
    cfg = H.load_cfg("fit_smplx_combined_halpe.yaml", use_hands=False, use_face=False)
    B = 4
    bm = smplx.create(synth_model, joint_mapper=U.JointMapper(H.joint_map_for(cfg)), num_betas=cfg["num_betas"],
                      num_expression_coeffs=cfg["num_expression_coeffs"], num_pca_comps=cfg["num_pca_comps"],
                      use_face_contour=cfg["use_face_contour"], batch_size=B, differentiable=True).to(gpu)
    rng = np.random.RandomState(7)
    P = H.random_params(rng, B, scale=0.3, npca=cfg["num_pca_comps"])
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=gpu)
    true_betas = 0.5 * rng.normal(size=(1, 10))
    with torch.no_grad():
        target = bm(return_verts=True, betas=t(np.repeat(true_betas, B, 0)), global_orient=t(P["global_orient"] + 0.1 * rng.normal(size=(B, 3))),
                    body_pose=t(P["pose_embedding"] + 0.1 * rng.normal(size=(B, 63)))).joints.clone()
    betas = torch.zeros(1, 10, device=gpu, requires_grad=True)
    orient = t(P["global_orient"]).requires_grad_(True)
    pose = t(P["pose_embedding"]).requires_grad_(True)
    params = [betas, orient, pose]
    assert sum(p.numel() for p in params) == 274
    rec = []

    def closure():
        for p in params:
            p.grad = None
        joints = bm(return_verts=True, betas=betas.expand(B, 10).contiguous(), global_orient=orient, body_pose=pose).joints
        loss = ((joints - target) ** 2).sum() + 0.1 * ((joints[1:] - joints[:-1]) ** 2).sum()
        loss.backward()
        rec.append((torch.cat([p.detach().reshape(1, -1) for p in params], 1).cpu().numpy(), loss.detach().reshape(1).cpu().numpy(),
                    torch.cat([p.grad.reshape(1, -1) for p in params], 1).cpu().numpy()))
        return loss
    mon = fitting.FittingMonitor(maxiters=5, ftol=1e-9, gtol=1e-9)
    with mon:
        res = mon.run_fitting(_lbfgs(params, lr=1.0, max_iter=15, wide=True), closure, params, None, 0, use_vposer=False)
    assert res is not None and res < float(rec[0][1][0]), (res, rec[0][1])
    hyper = dict(maxiters=5, ftol=1e-9, gtol=1e-9, lr=1.0, max_iter=15, groups=_groups([10, 12, 252]))
    _replay_surface("run_fitting, one shape over 4 frames (N = 274)", rec, 0, hyper, res)
    print("loss %.5f -> %.5f in %d evaluations" % (float(rec[0][1][0]), res, len(rec)))


# ---------------------------------------------------------------- 8. refusals and device memory
def test_refusals_and_device_memory(gpu):
    from smplifyx_amd import _capi
    for kw, msg in ((dict(B=1, N=32769), "N = 32769"), (dict(B=1, N=0), "N = 0"), (dict(B=0, N=4), "B = 0"),
                    (dict(B=1, N=257, groups=[1] * 257), "257 parameter groups"), (dict(B=1, N=6, groups=[2, 3]), "sum to 5"),
                    (dict(B=1, N=6, history_size=401), "history_size 401"), (dict(B=1, N=6, history_size=0), "history_size")):
        with pytest.raises(_capi.SfxError, match=msg):
            _opt(**kw)
    opt = _opt(2, 6)
    x = torch.zeros(2, 6, device=gpu)
    for bad, msg in ((x.cpu(), "CUDA tensor"), (x.double(), "float32"), (torch.zeros(6, 2, device=gpu).t(), "contiguous"),
                     (torch.zeros(2, 7, device=gpu), "shape")):
        with pytest.raises(ValueError, match=msg):
            opt.begin(bad)
    with pytest.raises(RuntimeError, match="before begin"):
        opt.tell(torch.zeros(2, device=gpu), x)
    opt.begin(x)
    with pytest.raises(ValueError, match="CUDA tensor"):
        opt.tell(torch.zeros(2), x)
    with pytest.raises(ValueError, match="float32"):
        opt.tell(torch.zeros(2, device=gpu), x.double())
    with pytest.raises(_capi.SfxError, match="resume"):
        opt.begin(x, mode="step", resume=True)
    opt.close()
    big = torch.zeros(32769, device=gpu, requires_grad=True)
    with pytest.raises(ValueError, match="32769 elements.*32768"):
        _lbfgs([big], wide=True).step(lambda: (big ** 2).sum())
    # 20 create / begin / destroy cycles of a handle of ~110 MB, measured as test_gpu_opt_ext.test_refusals_and_device_memory does
    B, N = 4, W.NMAX
    gc.collect()
    _opt(B, N).close()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    o = _opt(B, N)
    m = free0 - torch.cuda.mem_get_info()[0]
    o.close()
    assert m > 64 << 20, "the handle must be well above the allocator's granularity, got %d bytes" % m
    x0 = torch.zeros(B, N, device=gpu)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(20):
        o = _opt(B, N)
        o.begin(x0)
        o.close()
        with pytest.raises(_capi.SfxError):
            _opt(B, N + 1)
    torch.cuda.synchronize()
    after = torch.cuda.mem_get_info()[0]
    print("handle %.1f MB; free memory at the start / after 20 cycles: %.1f / %.1f MB" % (m / 2 ** 20, free0 / 2 ** 20, after / 2 ** 20))
    assert abs(free0 - after) <= m / 2, (m, free0, after)
