"""VPoser-v1 host side: checkpoint loading and the once-per-frame encoder.

The reference loads the external `human_body_prior` (cvpr19 branch) package:
`load_vposer(vposer_ckpt, vp_model='snapshot')` (smplifyx/fit_single_frame.py:241), decodes the
latent inside every closure evaluation (fitting.py:236-238 -- on the MI355X that is
csrc/vposer.h), and, with a regression prior, starts from
`vposer.encode(full_pose_prior).sample()` (fit_single_frame.py:245).  The encoder runs ONCE per
frame, outside the optimisation loop, so it lives here on the host (numpy); its architecture
follows the public VPoser-v1 definition:

    bn1 -> fc1 (in->512) -> leaky_relu(0.2) -> bn2 -> dropout (eval: off) -> fc2 (512->512)
        -> leaky_relu(0.2) -> Normal(mu = fc_mu, sigma = softplus(fc_logvar))

`.sample()` makes the reference non-deterministic; `encode` returns the mean by default and
draws the sample only when given a seeded generator.

`VPoser` / `load_vposer_model` are the OBJECT the reference holds (`vposer, _ = load_vposer(ckpt,
vp_model='snapshot'); vposer = vposer.to(device); vposer.eval()`): `decode(z, output_type='aa')`
runs the batched HIP decoder of csrc/vposer_batch.hip (engine.VPoserDecoder) and carries an
autograd graph whose backward is that kernel's; `encode(pose)` returns the Normal the reference
samples from, computed by the host encoder above -- or, for an object made with
`differentiable=True` and poses on the GPU, by the batched HIP encoder of csrc/vposer_encode.hip
(engine.VPoserEncoder) with a graph back to the poses.
"""
import glob
import os

import numpy as np
import torch
import torch.nn as nn

_DEC = (("fc1_w", "bodyprior_dec_fc1.weight"), ("fc1_b", "bodyprior_dec_fc1.bias"),
        ("fc2_w", "bodyprior_dec_fc2.weight"), ("fc2_b", "bodyprior_dec_fc2.bias"),
        ("out_w", "bodyprior_dec_out.weight"), ("out_b", "bodyprior_dec_out.bias"))
_ENC = (("enc_bn1_w", "bodyprior_enc_bn1.weight"), ("enc_bn1_b", "bodyprior_enc_bn1.bias"),
        ("enc_bn1_mean", "bodyprior_enc_bn1.running_mean"), ("enc_bn1_var", "bodyprior_enc_bn1.running_var"),
        ("enc_fc1_w", "bodyprior_enc_fc1.weight"), ("enc_fc1_b", "bodyprior_enc_fc1.bias"),
        ("enc_bn2_w", "bodyprior_enc_bn2.weight"), ("enc_bn2_b", "bodyprior_enc_bn2.bias"),
        ("enc_bn2_mean", "bodyprior_enc_bn2.running_mean"), ("enc_bn2_var", "bodyprior_enc_bn2.running_var"),
        ("enc_fc2_w", "bodyprior_enc_fc2.weight"), ("enc_fc2_b", "bodyprior_enc_fc2.bias"),
        ("enc_mu_w", "bodyprior_enc_mu.weight"), ("enc_mu_b", "bodyprior_enc_mu.bias"),
        ("enc_logvar_w", "bodyprior_enc_logvar.weight"), ("enc_logvar_b", "bodyprior_enc_logvar.bias"))
BN_EPS = 1e-5


def weights_from_state_dict(sd):
    """numpy weight dict (the keys engine.DeviceModel.set_vposer and encode() read) from a
    VPoser-v1 state dict (torch tensors or arrays, `bodyprior_*` names)."""
    def arr(v):
        return np.ascontiguousarray(v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v), np.float32)
    missing = [k for _, k in _DEC if k not in sd]
    if missing:
        raise KeyError("not a VPoser-v1 state dict, missing %s" % missing)
    w = {n: arr(sd[k]) for n, k in _DEC}
    if all(k in sd for _, k in _ENC):
        w.update({n: arr(sd[k]) for n, k in _ENC})
    return w


def load_vposer(vposer_ckpt):
    """Weights from `vposer_ckpt`: an .npz with the short names, a torch snapshot (.pt state
    dict), or a human_body_prior experiment directory (`snapshots/*.pt`, the newest is used, as
    `load_vposer(expr_dir, vp_model='snapshot')` does)."""
    path = os.path.expandvars(vposer_ckpt)
    if os.path.isdir(path):
        snaps = sorted(glob.glob(os.path.join(path, "snapshots", "*.pt")))
        if not snaps:
            raise ValueError("no snapshots/*.pt under %r" % path)
        path = snaps[-1]
    if path.endswith(".npz"):
        with np.load(path) as z:
            d = {k: z[k] for k in z.files}
        if "fc1_w" in d:
            return {k: np.ascontiguousarray(v, np.float32) for k, v in d.items()}
        return weights_from_state_dict(d)
    import torch
    sd = torch.load(path, map_location="cpu")
    if isinstance(sd, dict) and "state_dict" in sd:
        sd = sd["state_dict"]
    return weights_from_state_dict(sd)


def _leaky(x):
    return np.where(x > 0, x, 0.2 * x)


def _softplus(x):
    return np.log1p(np.exp(-np.abs(x))) + np.maximum(x, 0)


def _aa_to_matrot(pose):
    """[B, 21*3] axis-angle -> [B, 21*9] rotation matrices (plain Rodrigues, as the package's
    aa2matrot / torchgeometry angle_axis_to_rotation_matrix)."""
    aa = pose.reshape(-1, 3).astype(np.float64)
    ang = np.linalg.norm(aa, axis=1, keepdims=True)
    small = ang[:, 0] < 1e-6
    ax = aa / np.where(ang > 0, ang, 1.0)
    K = np.zeros((aa.shape[0], 3, 3))
    K[:, 0, 1], K[:, 0, 2] = -ax[:, 2], ax[:, 1]
    K[:, 1, 0], K[:, 1, 2] = ax[:, 2], -ax[:, 0]
    K[:, 2, 0], K[:, 2, 1] = -ax[:, 1], ax[:, 0]
    s, c = np.sin(ang)[:, :, None], np.cos(ang)[:, :, None]
    R = np.eye(3)[None] + s * K + (1 - c) * (K @ K)
    # first-order form near zero (torchgeometry's Taylor branch)
    Kt = np.zeros_like(K)
    Kt[:, 0, 1], Kt[:, 0, 2] = -aa[:, 2], aa[:, 1]
    Kt[:, 1, 0], Kt[:, 1, 2] = aa[:, 2], -aa[:, 0]
    Kt[:, 2, 0], Kt[:, 2, 1] = -aa[:, 1], aa[:, 0]
    R[small] = (np.eye(3)[None] + Kt)[small]
    return R.reshape(pose.shape[0], -1)


def _encoder_trunk(w, pose):
    """(x, f): the encoder's last hidden layer [B, 512] in float64 for [B, 63] poses, and the float64 weight accessor."""
    if "enc_fc1_w" not in w:
        raise ValueError("these VPoser weights carry no encoder (bodyprior_enc_*)")
    x = np.asarray(pose, np.float64).reshape(-1, 63)
    n_in = w["enc_fc1_w"].shape[1]
    if n_in == 189:
        x = _aa_to_matrot(x)
    elif n_in != 63:
        raise ValueError("unexpected VPoser encoder input width %d" % n_in)
    f = lambda k: w[k].astype(np.float64)
    x = (x - f("enc_bn1_mean")) / np.sqrt(f("enc_bn1_var") + BN_EPS) * f("enc_bn1_w") + f("enc_bn1_b")
    x = _leaky(x @ f("enc_fc1_w").T + f("enc_fc1_b"))
    x = (x - f("enc_bn2_mean")) / np.sqrt(f("enc_bn2_var") + BN_EPS) * f("enc_bn2_w") + f("enc_bn2_b")
    x = _leaky(x @ f("enc_fc2_w").T + f("enc_fc2_b"))
    return x, f


def encode(w, pose, generator=None):
    """VPoser-v1 encoder on [B, 63] body poses -> latent [B, latentD] (float32).

    Returns the mean of the posterior; with `generator` (numpy Generator) draws
    mean + sigma * N(0, 1), the reference's `.sample()` made reproducible.  An encoder whose
    first layer is 189 wide (rotation-matrix input, `data_shape [1, 21, 9]`) gets the poses as
    rotation matrices, a 63-wide one gets them as they are."""
    x, f = _encoder_trunk(w, pose)
    mu = x @ f("enc_mu_w").T + f("enc_mu_b")
    if generator is not None:
        sigma = _softplus(x @ f("enc_logvar_w").T + f("enc_logvar_b"))
        mu = mu + sigma * generator.standard_normal(mu.shape)
    return mu.astype(np.float32)


def encode_stats(w, pose):
    """(mean, sigma) of the encoder's posterior for [B, 63] body poses, both [B, latentD] float64: the two parameters of the
    Normal that `vposer.encode(pose)` returns in the reference (sigma = softplus(fc_logvar))."""
    x, f = _encoder_trunk(w, pose)
    return x @ f("enc_mu_w").T + f("enc_mu_b"), _softplus(x @ f("enc_logvar_w").T + f("enc_logvar_b"))


class _Decode(torch.autograd.Function):
    """body_pose [B, 63] = decode(z) with the engine on both sides: forward = sfx_vposer_decode, backward =
    sfx_vposer_decode_backward at the SAVED z (stateless).  First derivatives only."""

    @staticmethod
    def forward(ctx, dec, z):
        z = z.detach()
        ctx.dec = dec
        ctx.save_for_backward(z)
        return dec.decode(z)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dbody):
        z, = ctx.saved_tensors
        with torch.cuda.device(z.device):
            return None, ctx.dec.decode_backward(z, dbody)


class _Encode(torch.autograd.Function):
    """(mean, sigma) [B, latentD] = encode(pose [B, 63]) with the engine on both sides: forward = sfx_vposer_encode, backward =
    sfx_vposer_encode_backward at the SAVED pose (stateless).  First derivatives only."""

    @staticmethod
    def forward(ctx, enc, pose):
        pose = pose.detach()
        ctx.enc = enc
        ctx.save_for_backward(pose)
        return enc.encode(pose)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dmean, dsigma):
        pose, = ctx.saved_tensors
        with torch.cuda.device(pose.device):
            return None, ctx.enc.encode_backward(pose, dmean, dsigma)


class VPoser(nn.Module):
    """The object `load_vposer(...)` returns in the reference, over the HIP decoder: `.latentD`, `.to(device)`, `.eval()`,
    `.decode(z, output_type='aa')`, `.encode(pose)`.  `weights` is the numpy dict of load_vposer() above -- the same dict
    smplx.create(vposer=) / DeviceModel.set_vposer accept; it stays on the host (`.weights`), the device copy is an
    engine.VPoserDecoder per GPU, made at the first decode there.

    `differentiable=True` (the convention of smplx.create(differentiable=)): `encode` of poses on the GPU runs the HIP encoder
    (one engine.VPoserEncoder per GPU, made at the first encode there) and returns a Normal whose mean and scale carry a graph
    back to the poses, and `forward` (encode -> rsample -> decode) is provided.  The default object keeps the host encoder."""

    def __init__(self, weights, differentiable=False):
        super().__init__()
        missing = [k for k, _ in _DEC if k not in weights]
        if missing:
            raise KeyError("VPoser weights: missing %s" % missing)
        self.weights = {k: np.ascontiguousarray(v, np.float32) for k, v in weights.items()}
        self.latentD = int(self.weights["fc1_w"].shape[1])
        self.differentiable = bool(differentiable)
        self._decoders = {}
        self._encoders = {}

    def _encoder(self, device):
        from . import engine
        key = device.index if device.index is not None else torch.cuda.current_device()
        if key not in self._encoders:
            if "enc_fc1_w" not in self.weights:
                raise ValueError("these VPoser weights carry no encoder (bodyprior_enc_*)")
            with torch.cuda.device(key):
                self._encoders[key] = engine.VPoserEncoder(self.weights)
        return self._encoders[key]

    def _decoder(self, device):
        from . import engine
        key = device.index if device.index is not None else torch.cuda.current_device()
        if key not in self._decoders:
            with torch.cuda.device(key):
                self._decoders[key] = engine.VPoserDecoder(self.weights)
        return self._decoders[key]

    def decode(self, Zin, output_type="aa"):
        """[B, latentD] -> [B, 1, 21, 3] axis-angle (the reference then calls .view(1, -1)).  With a Zin that requires grad
        the result carries the graph back to it; float64 latents are cast in and out."""
        if output_type != "aa":
            raise ValueError("output_type=%r: only 'aa' (axis-angle) is provided" % (output_type,))
        if not torch.is_tensor(Zin) or Zin.device.type != "cuda":
            raise RuntimeError("VPoser.decode needs a latent on the GPU: the HIP decoder has no CPU fallback")
        if Zin.dim() != 2 or Zin.shape[1] != self.latentD:
            raise ValueError("Zin: shape %s, expected (B, %d)" % (tuple(Zin.shape), self.latentD))
        with torch.cuda.device(Zin.device):
            body = _Decode.apply(self._decoder(Zin.device), Zin.to(torch.float32))
        return body.to(Zin.dtype).view(Zin.shape[0], 1, 21, 3)

    def encode(self, Pin):
        """torch.distributions.Normal(mean, stddev) of the posterior for poses [B, 63] (any shape with 63 values per row), on
        Pin's device and dtype.  Default object, or a Pin on the CPU: without a graph, computed by the host encoder
        (encode_stats), once per frame in the reference.  `differentiable=True` and a Pin on the GPU: computed by the HIP
        encoder; mean and scale carry the graph back to Pin (first derivatives only), float64 poses are cast in and out."""
        if self.differentiable and torch.is_tensor(Pin) and Pin.device.type == "cuda":
            P = Pin.reshape(Pin.shape[0], -1)
            if P.shape[1] != 63:
                raise ValueError("Pin: shape %s, expected 63 values per row" % (tuple(Pin.shape),))
            with torch.cuda.device(Pin.device):
                mean, sigma = _Encode.apply(self._encoder(Pin.device), P.to(torch.float32))
            return torch.distributions.normal.Normal(mean.to(Pin.dtype), sigma.to(Pin.dtype))
        with torch.no_grad():
            return self._encode_host(Pin)

    def _encode_host(self, Pin):
        P = Pin.detach().to("cpu", torch.float64).reshape(Pin.shape[0], -1).numpy()
        mu, sigma = encode_stats(self.weights, P)
        t = lambda a: torch.as_tensor(a).to(device=Pin.device, dtype=Pin.dtype)
        return torch.distributions.normal.Normal(t(mu), t(sigma))

    def forward(self, Pin, output_type="aa"):
        """The VAE round trip of a `differentiable=True` object: q = encode(Pin), z = q.rsample() (torch's global generator),
        decode(z) -> {'mean': q.mean, 'std': q.scale, 'pose_aa': [B, 1, 21, 3]}.  This is the cvpr19 package's `forward` as
        recalled from its public source: human_body_prior is not available to compare against, so, like the rest of the VPoser
        surface, it is UNPINNED.  Any output_type but 'aa' raises, as in decode."""
        if not self.differentiable:
            raise NotImplementedError("VPoser.forward (encode -> sample -> decode) is not used by the reference's fitting path; "
                                      "it is provided by VPoser(weights, differentiable=True)")
        if output_type != "aa":
            raise ValueError("output_type=%r: only 'aa' (axis-angle) is provided" % (output_type,))
        q = self.encode(Pin)
        return {"mean": q.mean, "std": q.scale, "pose_aa": self.decode(q.rsample(), output_type="aa")}

    def close(self):
        for d in list(self._decoders.values()) + list(self._encoders.values()):
            d.close()
        self._decoders = {}
        self._encoders = {}


def load_vposer_model(vposer_ckpt, vp_model="snapshot", differentiable=False):
    """`load_vposer(expr_dir, vp_model='snapshot')` of human_body_prior as the reference unpacks it
    (fit_single_frame.py:241): (VPoser, None) -- the second element is the training configuration, which nothing reads.
    `differentiable`: see VPoser."""
    if vp_model != "snapshot":
        raise ValueError("vp_model=%r: only 'snapshot' is provided" % (vp_model,))
    return VPoser(load_vposer(vposer_ckpt), differentiable=differentiable), None
