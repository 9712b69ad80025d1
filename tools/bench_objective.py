"""Time per evaluation (forward + backward) of the differentiable SMPLifyLoss: the fused device objective
next to the SAME objective composed from torch ops on the same GPU tensors (oracle.objective's project / gmof and the terms of
smplify_terms, constants moved to the device; backward by autograd).  halpe cfg (K = 136, hands + face), embedding prior,
B = 1 and B = 256.  Three fused figures: the loss module's forward + backward (the whole Python surface), engine.objective_eval
alone (argument checks + one launch), and an upper bound on the kernel's own time: calls over 65536 frames enqueued back to
back, for the embedding and the mixture prior.  torch.cuda.Event after warm-up, median of REPS, the variants alternating in one process.

usage: python tools/bench_objective.py [--out profiles/objective_ext.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import objective as O                       # noqa: E402
from smplifyx_amd import engine, fitting, prior, smplx  # noqa: E402
from smplifyx_amd.camera import create_camera           # noqa: E402

REPS, WARM, ROUNDS = 50, 10, 3
W = dict(data_weight=1000.0 / 600, body_pose_weight=20.0, shape_weight=75.0, bending_prior_weight=63.4, hand_prior_weight=57.4,
         expr_prior_weight=10.0)
JAW_W = [100.0, 1000.0, 1000.0]
BLOCKS = ("joints", "translation", "body_pose", "embedding", "betas", "expression", "jaw_pose", "left_hand_pose", "right_hand_pose")


def make_inputs(B, K, dev, seed=0):
    rng = np.random.RandomState(seed)
    t = lambda a: torch.tensor(np.asarray(a, np.float32), device=dev)
    I = dict(joints=t(rng.uniform(-0.8, 0.8, size=(B, K, 3))), rotation=t(np.tile(np.eye(3), (B, 1, 1))),
             translation=t(np.concatenate([0.2 * rng.normal(size=(B, 2)), rng.uniform(3, 5, size=(B, 1))], 1)),
             focal_x=t(np.full(B, 5000.0)), focal_y=t(np.full(B, 5000.0)), center=t(np.tile([400.0, 300.0], (B, 1))),
             joints_conf=t(rng.uniform(0, 1, size=(B, K))), joint_weights=t(np.ones((B, K))),
             body_pose=t(0.3 * rng.normal(size=(B, 63))), embedding=t(rng.normal(size=(B, 32))), betas=t(rng.normal(size=(B, 10))),
             expression=t(rng.normal(size=(B, 10))), jaw_pose=t(0.1 * rng.normal(size=(B, 3))),
             left_hand_pose=t(0.3 * rng.normal(size=(B, 45))), right_hand_pose=t(0.3 * rng.normal(size=(B, 45))))
    with torch.no_grad():
        proj = O.project(I["joints"], I["rotation"], I["translation"], I["focal_x"], I["focal_y"], I["center"])
    I["gt_joints"] = proj + t(rng.uniform(5, 300, size=(B, K, 2)) * rng.choice([-1.0, 1.0], size=(B, K, 2)))
    return I


def torch_objective(L, I, consts):
    """SMPLifyLoss.forward (fitting.py:375-461, use_vposer, no interpenetration) from torch ops: oracle.objective's terms."""
    proj = O.project(L["joints"], I["rotation"], L["translation"], I["focal_x"], I["focal_y"], I["center"])
    weights = (I["joint_weights"] * I["joints_conf"]).unsqueeze(-1)
    total = torch.sum(weights ** 2 * O.gmof(I["gt_joints"] - proj, 100.0)) * W["data_weight"] ** 2
    total = total + L["embedding"].pow(2).sum() * W["body_pose_weight"] ** 2
    total = total + L["betas"].pow(2).sum() * W["shape_weight"] ** 2
    total = total + torch.sum(torch.exp(L["body_pose"][:, consts["idx"]] * consts["sign"]).pow(2)) * W["bending_prior_weight"]
    total = total + L["jaw_pose"].mul(consts["jaw"]).pow(2).sum() + L["expression"].pow(2).sum() * W["expr_prior_weight"] ** 2
    total = total + L["left_hand_pose"].pow(2).sum() * W["hand_prior_weight"] ** 2
    return total + L["right_hand_pose"].pow(2).sum() * W["hand_prior_weight"] ** 2


def gpu_times(fns):
    """{name: median microseconds} of each callable, REPS timed calls each, the callables alternating."""
    for fn in fns.values():
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(REPS):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b) * 1e3)
    return {k: float(np.median(v)) for k, v in ts.items()}


def bench(B, K, dev):
    I = make_inputs(B, K, dev)
    mk = lambda t: prior.create_prior(prior_type=t, dtype=torch.float32)
    loss = fitting.create_loss("smplify", rho=100.0, use_joints_conf=True, use_hands=True, use_face=True, body_pose_prior=mk("l2"),
                               shape_prior=mk("l2"), angle_prior=mk("angle"), expr_prior=mk("l2"), jaw_prior=mk("l2"),
                               left_hand_prior=mk("l2"), right_hand_prior=mk("l2"), interpenetration=False, differentiable=True).to(dev)
    loss.reset_loss_weights(dict(W, jaw_prior_weight=JAW_W))
    cam = create_camera(rotation=I["rotation"].clone(), translation=I["translation"].clone(), focal_length_x=I["focal_x"],
                        focal_length_y=I["focal_y"], center=I["center"], batch_size=B, dtype=torch.float32).to(dev)
    cam.rotation.requires_grad = False
    L = {b: I[b].clone().requires_grad_(True) for b in BLOCKS if b != "translation"}
    L["translation"] = cam.translation
    z = lambda n: torch.zeros(B, n, device=dev)
    consts = dict(idx=torch.tensor(O.ANGLE_IDX, device=dev), sign=torch.tensor(O.ANGLE_SIGN, device=dev), jaw=torch.tensor(JAW_W, device=dev))

    def clear():
        for v in L.values():
            v.grad = None

    def fused_module():
        clear()
        out = smplx.ModelOutput(joints=L["joints"], full_pose=torch.cat([z(3), L["body_pose"], z(99)], 1), betas=L["betas"],
                                body_pose=L["body_pose"], expression=L["expression"], jaw_pose=L["jaw_pose"],
                                left_hand_pose=L["left_hand_pose"], right_hand_pose=L["right_hand_pose"])
        loss(out, camera=cam, gt_joints=I["gt_joints"], joints_conf=I["joints_conf"], joint_weights=I["joint_weights"],
             use_vposer=True, pose_embedding=L["embedding"], stage=0).backward()

    def fused_engine():
        engine.objective_eval(I["joints"], I["rotation"], I["translation"], I["focal_x"], I["focal_y"], I["center"], I["gt_joints"],
                              I["joint_weights"], I["body_pose"], I["embedding"], I["betas"], joints_conf=I["joints_conf"],
                              expression=I["expression"], jaw_pose=I["jaw_pose"], left_hand_pose=I["left_hand_pose"],
                              right_hand_pose=I["right_hand_pose"], weights=W, jaw_prior_weight=JAW_W, prior_form="embedding")

    def torch_ops():
        clear()
        torch_objective(L, I, consts).backward()

    # the two compute the same thing (checked before anything is timed)
    fused_module()
    a = {k: v.grad.clone() for k, v in L.items()}
    torch_ops()
    for k, v in L.items():
        err = float((v.grad - a[k]).norm() / v.grad.norm())
        assert err < 1e-4, (k, err)
    rounds = [gpu_times(dict(fused_module=fused_module, fused_engine=fused_engine, torch_ops=torch_ops)) for _ in range(ROUNDS)]
    res = {k: float(np.median([r[k] for r in rounds])) for k in rounds[0]}
    res["spread"] = {k: [float(min(r[k] for r in rounds)), float(max(r[k] for r in rounds))] for k in rounds[0]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "objective_ext.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_objective needs a GPU: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    K = 136
    out = dict(what="microseconds per evaluation of SMPLifyLoss, forward + backward, halpe cfg (K = 136, hands + face, embedding prior); "
                    "median of %d timed calls after %d warm-up calls, median over %d rounds (spread: min / max of the rounds)" % (REPS, WARM, ROUNDS),
               device=torch.cuda.get_device_name(0), K=K, results={})
    for B in (1, 256):
        r = bench(B, K, dev)
        out["results"]["B=%d" % B] = r
        print("B = %3d: fused loss module %.1f us, engine.objective_eval %.1f us, torch ops %.1f us  (torch / fused module = %.1f x)" %
              (B, r["fused_module"], r["fused_engine"], r["torch_ops"], r["torch_ops"] / r["fused_module"]), flush=True)
    # Towards the kernel's own time: 65536 frames per call, ten engine.objective_eval calls enqueued back to back between the two
    # events, divided by ten.  Each call still holds the wrapper's checks and allocations on the host, so the figure is an UPPER
    # bound on the kernel's time (and the rate a lower bound); the bytes are counted by hand from the shapes: every input read
    # and every output written once.  Both the embedding prior and the mixture prior (8 components: 8 x 63 x 63 table reads per
    # frame, from cache) are timed, at this size and per call at B = 256.
    rng = np.random.RandomState(1)
    A = rng.normal(size=(8, 63, 63))
    gmm = prior.MaxMixturePrior(gmm=dict(means=0.2 * rng.normal(size=(8, 63)), covars=0.05 * (A @ A.transpose(0, 2, 1)) / 63 + 0.02 * np.eye(63),
                                         weights=np.full(8, 0.125)), num_gaussians=8, dtype=torch.float32)
    mixture = dict(means=gmm.means.to(dev).contiguous(), precisions=gmm.precisions.to(dev).contiguous(),
                   nll_weights=gmm.nll_weights.reshape(-1).to(dev).contiguous(), comp_const=None)

    def caller(I, form):
        kw = dict(prior_form="mixture", mixture=mixture) if form == "mixture" else dict(prior_form="embedding")
        operand = I["body_pose"] if form == "mixture" else I["embedding"]
        return lambda: engine.objective_eval(I["joints"], I["rotation"], I["translation"], I["focal_x"], I["focal_y"], I["center"],
                                             I["gt_joints"], I["joint_weights"], I["body_pose"], operand, I["betas"],
                                             joints_conf=I["joints_conf"], expression=I["expression"], jaw_pose=I["jaw_pose"],
                                             left_hand_pose=I["left_hand_pose"], right_hand_pose=I["right_hand_pose"], weights=W,
                                             jaw_prior_weight=JAW_W, **kw)
    I = make_inputs(256, K, dev)
    r = gpu_times({form: caller(I, form) for form in ("embedding", "mixture")})
    out["results"]["engine.objective_eval per call, B=256"] = r
    print("B = 256, engine.objective_eval per call: embedding prior %.1f us, mixture prior %.1f us" % (r["embedding"], r["mixture"]), flush=True)
    BK, NQ = 65536, 10
    I = make_inputs(BK, K, dev)
    for form, n in (("embedding", 32), ("mixture", 63)):
        call = caller(I, form)
        t = gpu_times(dict(k=lambda: [call() for _ in range(NQ)]))["k"] / NQ
        nbytes = BK * (K * (3 + 2 + 1 + 1 + 3) + 2 * (9 + 3 + 63 + n + 10 + 10 + 3 + 45 + 45) + 5) * 4
        out["results"]["B=%d %s, %d calls back to back" % (BK, form, NQ)] = dict(us_per_call_upper_bound_on_kernel=t, bytes_counted=nbytes,
                                                                               GBps_lower_bound=nbytes / t * 1e-3)
        print("B = %d, %s prior: %.1f us per call (upper bound on the kernel): %.1f MB counted, >= %.0f GB/s" %
              (BK, form, t, nbytes / 1e6, nbytes / t * 1e-3), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
