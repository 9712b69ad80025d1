"""GPU tests of the device optimiser for evaluations the caller supplies: sfx_opt_* (csrc/opt_ext.hip), engine.BatchOptimizer,
optimizers.lbfgs_ls.LBFGS.step with any callable and FittingMonitor.run_fitting over it.

Reference, error measure, yardstick and bound: tests/opt_ext_common.py (lock-step replay: oracle/lbfgs_machine.StageMachine in
float32 is fed the very evaluations the device consumed; bound = 10 x the error of two arithmetic variants of the machine,
floor 1e-6).  tests/test_opt_ext_host.py asserts on the CPU that the variants stay in lock-step for every configuration used
here.  Every test runs tens to a few hundred launches of one wavefront per problem."""
import gc

import numpy as np
import pytest
import torch

import helpers as H
import opt_drive_common as O
import opt_ext_common as X
from oracle.lbfgs_machine import StageMachine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the HIP path has no CPU fallback")
    return torch.device("cuda:0")


CLS, LABEL = "BatchOptimizer", "opt-ext"      # the handle under test: its class in smplifyx_amd.engine, the label of its check_bound lines


def _opt(B, N, **hyper):
    return O.opt(CLS, B, N, **hyper)


_bits, _drive, _family, _check_replay = O.bits, O.drive, O.family, O.check_replay


# ---------------------------------------------------------------- 1. the reference's own trajectories
@pytest.mark.parametrize("fname,N", X.GOLDEN_CASES)
def test_golden_trajectories(gpu, fname, N):
    """Fed the evaluations of the reference's float32 runs (tests/golden/lbfgs.npz), the device finishes after exactly the golden's
    number of evaluations, returns its result exactly (one of the fed losses) and proposes each next point within the bound."""
    g = X.gold()
    xs, fs, gs = X.golden_evals(g, fname, N)
    bound = X.golden_bound(g, fname, N)
    opt = _opt(1, N, **X.GOLDEN_HYPER)
    feed = lambda xt, k: (torch.tensor(fs[k:k + 1], device=gpu), torch.tensor(gs[k], device=gpu).reshape(1, N))
    x0 = np.asarray(g["%s_%d_f32_x0" % (fname, N)], np.float32).reshape(1, N)
    dxs, _, _, n_done = _drive(opt, x0, feed, limit=len(xs) + 1)
    r = opt.result()
    assert n_done == len(xs) and r["evals"][0] == len(xs) and r["status"][0] == 1
    assert np.float32(r["result"][0]) == np.float32(float(g["%s_%d_f32_res" % (fname, N)]))
    err = max(float(np.abs(dxs[k, 0].astype(np.float64) - xs[k]).max() / np.abs(xs[k]).max()) for k in range(len(xs)))
    print("%s_%d: %d evaluations, worst relative trial-point difference %.2e (bound %.2e)" % (fname, N, len(xs), err, bound))
    H.check_bound("opt-ext golden", "%s_%d trial points" % (fname, N), err, bound)
    xf = r["x"].cpu().numpy()[0].astype(np.float64)
    H.check_bound("opt-ext golden", "%s_%d final point" % (fname, N),
                  np.abs(xf - g["%s_%d_f32_xf" % (fname, N)]).max() / np.abs(g["%s_%d_f32_xf" % (fname, N)]).max(), bound)
    opt.close()


# ---------------------------------------------------------------- 2. replay on the family
def _family_run(N, hname):
    return O.family_run(CLS, N, hname)


@pytest.mark.parametrize("N,hname", X.GPU_CONFIGS)
def test_replay_on_the_family(gpu, N, hname):
    """B = 5 problems per configuration; N = 3 and 4 sit on either side of one lane's three elements, 64 / 65 and 191 / 192 on
    either side of a full wavefront row, history 9 wraps the ring with a partial block of 8."""
    x0, xs, fs, gs, r, trace, n_done = _family_run(N, hname)
    bound = X.bound(N, hname)
    worst = 0.0
    for b in range(X.NB):
        res = dict(evals=r["evals"][b], status=r["status"][b], result=r["result"][b])
        worst = max(worst, _check_replay("opt-ext family", "N=%d %s trial points" % (N, hname), X.HYPER[hname], x0[b],
                                         xs[:, b], fs[:, b], gs[:, b], res, trace[b], bound))
        n = int(r["evals"][b])
        assert np.array_equal(_bits(r["grad"][b]), _bits(gs[n - 1, b])), "the gradient of the last consumed evaluation"
    assert n_done == r["evals"].max()
    print("N = %d, %s: evaluations %s, worst relative trial-point difference %.2e (bound %.2e)" % (N, hname, r["evals"], worst, bound))


# ---------------------------------------------------------------- 3. batch independence
@pytest.mark.parametrize("N,hname,distinct", X.INDEPENDENCE_CONFIGS)
def test_batch_independence_bit_for_bit(gpu, N, hname, distinct):
    """Each problem of the batch, run alone on the evaluations it consumed in the batch, proposes the same trial points and ends
    with the same result, bit for bit; a finished problem's row of x_trial never moves again; ten more `tell`s after the last
    one has finished change nothing."""
    hyper = X.HYPER[hname]
    x0, xs, fs, gs, r, _, n_done = _family_run(N, hname)
    ev = r["evals"]
    assert len(set(ev.tolist())) >= distinct, ("the problems must finish at different evaluations", ev)
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
    """opt_drive_common.step_mode_equals_fit_mode at N = 65."""
    O.step_mode_equals_fit_mode(CLS, 65)


# ---------------------------------------------------------------- 5. a non-finite evaluation
def test_a_nan_loss_ends_one_problem_only(gpu):
    """opt_drive_common.nan_loss_ends_one_problem_only: the other four bit for bit the run of test_batch_independence_bit_for_bit."""
    O.nan_loss_ends_one_problem_only(CLS, LABEL + " family")


# ---------------------------------------------------------------- 6. refusals
def test_refusals_and_device_memory(gpu):
    from smplifyx_amd import _capi
    for kw, msg in ((dict(B=1, N=193), "N = 193"), (dict(B=1, N=0), "N = 0"), (dict(B=0, N=4), "B = 0"),
                    (dict(B=1, N=13, groups=[1] * 13), "13 parameter groups"), (dict(B=1, N=6, groups=[2, 3]), "sum to 5"),
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
    # 20 create / destroy cycles of a handle of ~14 MB, measured as test_a_refused_model_keeps_no_device_memory measures it
    gc.collect()
    _opt(64, 192).close()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    o = _opt(64, 192)
    m = free0 - torch.cuda.mem_get_info()[0]
    o.close()
    assert m > 8 << 20, "the handle must be well above the allocator's granularity, got %d bytes" % m
    for _ in range(20):
        o = _opt(64, 192)
        o.begin(torch.zeros(64, 192, device=gpu))
        o.close()
        with pytest.raises(_capi.SfxError):
            _opt(64, 193)
    torch.cuda.synchronize()
    after = torch.cuda.mem_get_info()[0]
    print("handle %.1f MB; free memory at the start / after 20 cycles: %.1f / %.1f MB" % (m / 2 ** 20, free0 / 2 ** 20, after / 2 ** 20))
    assert abs(free0 - after) <= m / 2, (m, free0, after)


# ---------------------------------------------------------------- 7. the Python surface
def _lbfgs(params, **kw):
    from smplifyx_amd.optimizers.lbfgs_ls import LBFGS
    return LBFGS(params, line_search_fn="strong_Wolfe", **kw)


def test_lbfgs_step_takes_any_closure(gpu):
    """quad_6 of the golden, with a closure written on a GPU tensor: step() returns the loss at entry, leaves the accepted point in
    x and the last gradient in x.grad; a second step resumes; run_fitting over it ends where the reference's run ended."""
    from smplifyx_amd import fitting
    g = X.gold()
    x0 = torch.tensor(g["quad_6_f32_x0"], dtype=torch.float32, device=gpu)
    x = x0.clone().requires_grad_(True)
    seen = []

    def closure():
        # an arbitrary closure on a GPU tensor: this one takes x to the host and evaluates there, in the arithmetic the golden's
        # evaluations were made with (sin on the GPU differs from the CPU's in the last bit, and near the minimum that bit
        # decides line searches: the comparison with the reference's final point is about the optimiser, not about sin)
        x.grad = None
        l = X.golden_fn("quad", x.cpu())
        l.backward()
        seen.append((x.detach().clone(), l.detach().clone(), x.grad.clone()))
        return l
    opt = _lbfgs([x], lr=1.0, max_iter=30)
    loss = opt.step(closure)
    assert torch.is_tensor(loss) and loss.dim() == 0 and loss.device == x.device
    assert torch.equal(seen[0][0], x0) and float(loss) == float(seen[0][1]), "the entry loss"
    assert torch.equal(x.grad, seen[-1][2]), "x.grad holds the last evaluation's gradient"
    assert float(X.golden_fn("quad", x.detach().cpu())) < float(loss)
    assert any(torch.equal(x.detach(), s[0]) for s in seen), "the accepted point is one of the evaluated points"
    n1, x1 = len(seen), x.detach().clone()
    loss2 = opt.step(closure)
    assert torch.equal(seen[n1][0], x1), "the second step starts at the accepted point"
    assert float(loss2) < float(loss)
    # the whole loop, as gen_lbfgs of tools/make_goldens.py ran the reference
    with torch.no_grad():
        x.copy_(x0)
    x.grad = None
    mon = fitting.FittingMonitor(maxiters=30, ftol=1e-9, gtol=1e-9)
    with mon:
        res = mon.run_fitting(_lbfgs([x], lr=1.0, max_iter=30), closure, [x], None, 0, use_vposer=False)
    xf = g["quad_6_f32_xf"]
    err = np.abs(x.detach().cpu().numpy().astype(np.float64) - xf).max() / np.abs(xf).max()
    print("run_fitting on quad_6: result %r (golden %r), final point off by %.2e (bound %.2e)" %
          (res, float(g["quad_6_f32_res"]), err, X.golden_bound(g, "quad", 6)))
    assert res is not None
    H.check_bound("opt-ext golden", "quad_6 run_fitting final point", err, X.golden_bound(g, "quad", 6))


def test_per_sample_on_a_differentiable_smplx_loss(gpu, synth_model):
    """LBFGS(per_sample=True), B = 4, on a loss written on smplx.create(differentiable=True): squared distance of the joints to
    targets made from perturbed parameters, over global_orient, body_pose and betas (76 variables per row).  Every row's loss
    strictly decreases; each row's recorded evaluations replay through the machine (one LBFGS.step = run_fitting with maxiters
    = 1 and its own tests off); poll_every = 4 leaves bit-identical parameters.
    Yardstick of this replay: the two variants fed the same recorded evaluations (there is no CPU closure of this loss to run
    them on), error while both still run; bound = 10 x the larger, floor 1e-6."""
    from smplifyx_amd import smplx, utils as U
    cfg = H.load_cfg("fit_smplx_combined_halpe.yaml", use_hands=False, use_face=False)
    B = 4
    bm = smplx.create(synth_model, joint_mapper=U.JointMapper(H.joint_map_for(cfg)), num_betas=cfg["num_betas"],
                      num_expression_coeffs=cfg["num_expression_coeffs"], num_pca_comps=cfg["num_pca_comps"],
                      use_face_contour=cfg["use_face_contour"], batch_size=B, differentiable=True).to(gpu)
    rng = np.random.RandomState(5)
    P = H.random_params(rng, B, scale=0.3, npca=cfg["num_pca_comps"])
    names = ("global_orient", "body_pose", "betas")
    start = dict(global_orient=P["global_orient"], body_pose=P["pose_embedding"], betas=P["betas"])
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=gpu)
    with torch.no_grad():
        target = bm(return_verts=True, **{n: t(start[n] + 0.15 * rng.normal(size=start[n].shape)) for n in names}).joints.clone()
    params = [getattr(bm, n) for n in names]

    def set_start():
        with torch.no_grad():
            for p, n in zip(params, names):
                p.copy_(t(start[n]).reshape(p.shape))
                p.grad = None
    rec = []

    def closure():
        for p in bm.parameters():
            p.grad = None
        loss = ((bm(return_verts=True).joints - target) ** 2).sum((1, 2))
        loss.sum().backward()
        rec.append((torch.cat([p.detach().reshape(B, -1) for p in params], 1).cpu().numpy(), loss.detach().cpu().numpy(),
                    torch.cat([p.grad.reshape(B, -1) for p in params], 1).cpu().numpy()))
        return loss
    lb = dict(lr=1.0, max_iter=20)
    set_start()
    opt = _lbfgs(params, per_sample=True, **lb)
    entry = opt.step(closure)
    assert tuple(entry.shape) == (B,) and entry.device == target.device
    evals = opt._ext.result()["evals"]
    final = [p.detach().clone() for p in params]
    xs, fs, gs = (np.stack([r[i] for r in rec]) for i in range(3))
    assert np.array_equal(_bits(entry.cpu().numpy()), _bits(fs[0]))
    with torch.no_grad():
        after = ((bm(return_verts=True).joints - target) ** 2).sum((1, 2))
    assert (after < entry).all(), (entry, after)
    hyper = dict(maxiters=1, ftol=0.0, gtol=0.0, lr=1.0, max_iter=20, groups=[(0, 3, True), (3, 63, True), (66, 10, True)])
    for b in range(B):
        n = int(evals[b])
        yard = 0.0
        for name, v in X.variants(xs[0, b], **hyper):
            m = StageMachine(xs[0, b], dtype=np.float32, **hyper)
            for k in range(n):
                if v.done or m.done:
                    break
                yard = max(yard, float(np.abs(v.x_trial.astype(np.float64) - m.x_trial).max() / np.abs(m.x_trial).max()))
                v.feed(fs[k, b], gs[k, b]); m.feed(fs[k, b], gs[k, b])
        bound = max(X.FLOOR, 10 * yard)
        m = StageMachine(xs[0, b], dtype=np.float32, **hyper)
        err, lock = X.replay(m, xs[:n, b], fs[:n, b], gs[:n, b])
        assert lock, (b, n, m.done)
        assert np.float32(m.records[-2][1]) == np.float32(entry[b].item())       # the (1, entry loss, ...) record of the step
        print("row %d: %d evaluations, entry loss %.4f -> %.4f, trial points off by %.2e (bound %.2e)" %
              (b, n, entry[b].item(), after[b].item(), err, bound))
        H.check_bound("opt-ext smplx", "per-sample trial points", err, bound)
    # polling every 4th evaluation: the same parameters, bit for bit
    set_start()
    n1 = len(rec)
    opt4 = _lbfgs(params, per_sample=True, poll_every=4, **lb)
    entry4 = opt4.step(closure)
    assert (len(rec) - n1) % 4 == 0 and len(rec) - n1 >= n1
    assert torch.equal(entry4, entry)
    for p, q in zip(params, final):
        assert torch.equal(p.detach(), q)
