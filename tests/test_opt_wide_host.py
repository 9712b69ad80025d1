"""CPU tests of the wide device optimiser (sfx_opt_wide_*, engine.WideOptimizer, LBFGS(wide=True): one workgroup per problem, up
to 32768 variables): the yardstick the GPU tests (test_gpu_opt_wide.py) rest on, the state machine of csrc/lbfgs_wide.h itself --
run on the CPU over a serial vector layer by tests/lbfgs_wide_check.cpp, under AddressSanitizer and UBSan --, the reference's
own trajectories at 193 and 1000 variables, and the refusals that need no device.

Reference, error measure and bound: tests/opt_ext_common.py, unchanged (lock-step replay against
oracle/lbfgs_machine.StageMachine; bound = 10 x the larger error of the machine's two arithmetic variants, floor 1e-6)."""
import os
import subprocess

import numpy as np
import pytest
import torch

import opt_ext_common as X
import opt_wide_common as W
from oracle.lbfgs_machine import StageMachine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


# ---------------------------------------------------------------- (a) the yardstick
@pytest.mark.parametrize("N,hname", W.WIDE_CONFIGS)
def test_variants_stay_in_lock_step(N, hname):
    """Both variants, on each of the 5 problems: the machine fed their evaluations wants every one of them and is done after the
    last; the same records; the same result (as test_opt_ext_host.py asserts for the narrow configurations)."""
    worst = 0.0
    for b in range(X.NB):
        for name, err, lock, recs, res, n in X.yardstick(N, hname, b):
            assert lock, (N, hname, b, name, "left lock-step", n)
            assert recs, (N, hname, b, name, "records differ")
            assert res, (N, hname, b, name, "results differ")
            assert n <= 150, (N, hname, b, n)
            worst = max(worst, err)
    print("N = %d, %s: worst relative trial-point difference of the variants %.2e -> bound %.2e" % (N, hname, worst, X.bound(N, hname)))
    assert X.bound(N, hname) == max(X.FLOOR, 10 * worst)
    assert worst < 1e-3, "a variant this far from the machine is not a rounding difference"


def test_the_independence_configuration_ends_at_different_evaluations():
    N, hname = W.INDEPENDENCE_CONFIG
    n = [X.yardstick(N, hname, b)[0][5] for b in range(X.NB)]
    assert len(set(n)) >= 2, n


# ---------------------------------------------------------------- (b) the header's machine on the CPU
def _header(N, hyper, fs, groups):
    h = dict(maxiters=30, ftol=1e-9, gtol=1e-9, lr=1.0, max_iter=None, max_eval=None, history=100, tol_grad=1e-5, tol_change=1e-9,
             reuse_entry_eval=False)
    h.update(hyper)
    max_iter = h["maxiters"] if h["max_iter"] is None else h["max_iter"]
    max_eval = max_iter * 5 // 4 if h["max_eval"] is None else h["max_eval"]
    return [N, len(fs), h["maxiters"], h["ftol"], h["gtol"], h["lr"], max_iter, max_eval, h["history"], h["tol_grad"], h["tol_change"],
            int(h["reuse_entry_eval"]), len(groups)] + list(groups) + [float(f) for f in fs]


@pytest.fixture(scope="module")
def machine_runs(tmp_path_factory):
    """{(N, hname, b, nan_at): (x0, hyper, fs, gs, program's answer)} from ONE run of the program: the machine's own run of every
    case on the CPU closure is recorded, the program is fed the recorded losses and gradients."""
    tmp = tmp_path_factory.mktemp("lbfgs_wide")
    exe = str(tmp / "lbfgs_wide_check")
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
                    "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "lbfgs_wide_check.cpp"), "-o", exe], check=True)
    cases = [(N, hname, b, None) for N, hname in W.CHECK_CONFIGS for b in range(X.NB)]
    cases.append(X.NAN_CONFIG + (X.NAN_PROBLEM, X.NAN_AT))
    hdr, vec, rec = [float(len(cases))], [], {}
    for N, hname, b, nan_at in cases:
        x0, hyper = X.family_x0(N, b), X.HYPER[hname]
        groups = [N] if b % 2 == 0 else [N - N // 3, N // 3]      # (the gtol test sees one tensor or two)
        hyper_g = dict(hyper, groups=[(int(o), n, True) for o, n in zip(np.cumsum([0] + groups[:-1]), groups)])
        xs, fs, gs = X.run_on_cpu_closure(StageMachine(x0, dtype=np.float32, **hyper_g), b, nan_at=nan_at)
        hdr += _header(N, hyper, fs, groups)
        vec += [x0] + gs
        rec[(N, hname, b, nan_at)] = [x0, hyper_g, fs, gs]
    np.asarray(hdr, "<f8").tofile(str(tmp / "in_hdr.bin"))
    np.concatenate(vec).astype("<f4").tofile(str(tmp / "in_vec.bin"))
    r = subprocess.run([exe] + [str(tmp / n) for n in ("in_hdr.bin", "in_vec.bin", "out_hdr.bin", "out_vec.bin")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:]
    oh, ov = np.fromfile(str(tmp / "out_hdr.bin"), "<f8"), np.fromfile(str(tmp / "out_vec.bin"), "<f4")
    h = p = 0
    for key in cases:
        N = key[0]
        k, status, result, evals, nrec = oh[h:h + 5]
        k, nrec = int(k), int(nrec)
        records = oh[h + 5:h + 5 + 4 * nrec].reshape(nrec, 4)
        h += 5 + 4 * nrec
        pts = ov[p:p + (k + 1) * N].reshape(k + 1, N)
        p += (k + 1) * N
        rec[key].append(dict(consumed=k, status=int(status), result=np.float32(result), evals=int(evals), records=records,
                             xs=pts[:k], x=pts[k]))
    assert h == oh.size and p == ov.size
    return rec


def _check_against_machine(key, run):
    x0, hyper, fs, gs, a = run
    N, hname = key[:2]
    assert a["consumed"] == len(fs) and a["evals"] == len(fs) and a["status"] == 1, (key, a["consumed"], len(fs), a["status"])
    m = StageMachine(x0, dtype=np.float32, **hyper)
    err, lock = X.replay(m, a["xs"], fs, gs)
    assert lock, (key, "left lock-step")
    assert X.same_records(a["records"], m.records), (key, a["records"][:, 0], [r[0] for r in m.records])
    assert X.same_result(a["result"], m.result), (key, a["result"], m.result)
    bound = X.bound(N, hname)
    assert err <= bound, (key, err, bound)
    xf = m.x.astype(np.float64)
    assert np.abs(a["x"] - xf).max() / np.abs(xf).max() <= bound, (key, "accepted point")
    return err, bound


@pytest.mark.parametrize("N,hname", W.CHECK_CONFIGS)
def test_the_headers_machine_replays_in_lock_step(machine_runs, N, hname):
    """csrc/lbfgs_wide.h over a serial vector layer, fed the evaluations of the machine's own run: it consumes every one of them and
    is done after the last, writes the same records, returns the same result and asks for the same points within the bound."""
    worst = 0.0
    for b in range(X.NB):
        err, bound = _check_against_machine((N, hname, b, None), machine_runs[(N, hname, b, None)])
        worst = max(worst, err)
    print("N = %d, %s: worst relative trial-point difference %.2e (bound %.2e)" % (N, hname, worst, bound))


def test_the_headers_machine_takes_a_nan_loss_as_the_machine_does(machine_runs):
    key = X.NAN_CONFIG + (X.NAN_PROBLEM, X.NAN_AT)
    fs = machine_runs[key][2]
    assert np.isnan(fs[X.NAN_AT]) and len(fs) > X.NAN_AT + 1
    err, bound = _check_against_machine(key, machine_runs[key])
    print("NaN at evaluation %d of %d: worst relative trial-point difference %.2e (bound %.2e)" % (X.NAN_AT, len(fs), err, bound))


# ---------------------------------------------------------------- (c) refusals without a device
def test_wide_optimizer_refuses_bad_shapes_before_the_device():
    from smplifyx_amd import _capi, engine
    for kw, msg in ((dict(B=1, N=32769), "N = 32769"), (dict(B=1, N=0), "N = 0"), (dict(B=0, N=4), "B = 0"),
                    (dict(B=1, N=257, groups=[1] * 257), "257 parameter groups"), (dict(B=1, N=6, groups=[2, 3]), "sum to 5"),
                    (dict(B=1, N=6, history_size=401), "history_size 401"), (dict(B=1, N=6, history_size=0), "history_size")):
        with pytest.raises(_capi.SfxError, match=msg):
            engine.WideOptimizer(**kw)
    with pytest.raises(TypeError, match="unknown hyper-parameter"):
        engine.WideOptimizer(1, 6, momentum=0.9)
    if not torch.cuda.is_available():
        with pytest.raises(_capi.SfxError, match="no HIP device"):
            engine.WideOptimizer(1, 6)


def _lbfgs(params, **kw):
    from smplifyx_amd.optimizers.lbfgs_ls import LBFGS
    return LBFGS(params, line_search_fn="strong_Wolfe", **kw)


def _closure_of(params):
    def closure():
        for p in params:
            p.grad = None
        l = sum((p ** 2).sum() for p in params)
        l.backward()
        return l
    return closure


def test_wide_step_refuses_cpu_tensors_and_more_than_32768_elements():
    x = torch.zeros(193, requires_grad=True)
    with pytest.raises(ValueError, match="parameter 0 is on cpu.*no CPU fallback"):
        _lbfgs([x], wide=True).step(_closure_of([x]))
    assert x.grad is None and torch.equal(x.detach(), torch.zeros(193)), "a refused step touches nothing"
    xs = [torch.zeros(2, requires_grad=True) for _ in range(13)]
    with pytest.raises(ValueError, match="parameter 0 is on cpu.*no CPU fallback"):
        _lbfgs(xs, wide=True).step(_closure_of(xs))
    big = torch.zeros(32769, requires_grad=True)
    with pytest.raises(ValueError, match="32769 elements.*32768"):
        _lbfgs([big], wide=True).step(_closure_of([big]))
    rows = [torch.zeros(2, 32768, requires_grad=True), torch.zeros(2, 1, requires_grad=True)]
    with pytest.raises(ValueError, match="32769 elements per sample.*32768"):
        _lbfgs(rows, wide=True, per_sample=True).step(_closure_of(rows))
    many = [torch.zeros(1, requires_grad=True) for _ in range(257)]
    with pytest.raises(ValueError, match="257 parameter tensors.*256"):
        _lbfgs(many, wide=True).step(_closure_of(many))
    # the default keeps its refusals, and says where to look
    with pytest.raises(ValueError, match="193 elements.*192.*wide=True"):
        _lbfgs([x]).step(_closure_of([x]))


# ---------------------------------------------------------------- (d) the reference's own trajectories
@pytest.mark.parametrize("N", W.GOLDEN_NS)
def test_machine_and_variants_follow_the_wide_golden(N):
    """tests/golden/lbfgs_wide.npz: fed the golden's evaluations, the machine and both variants finish after exactly its number of
    evaluations and return its result; the variants' distance from the golden's points sets the GPU test's bound."""
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "lbfgs_wide.npz")) < 400 << 10
    for name, err, lock, res in W.golden_yardstick(N):
        assert lock and res, (N, name, lock, res)
        assert err < 1e-3, (N, name, err)
    print("N = %d: %s -> bound %.2e" % (N, ["%s %.2e" % (e[0], e[1]) for e in W.golden_yardstick(N)], W.golden_bound(N)))
