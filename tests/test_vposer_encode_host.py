"""CPU tests of the stand-alone VPoser encoder's surface: the four sfx_vposer_encoder_* / sfx_vposer_encode* entry points in the
binding, every refusal of sfx_vposer_encoder_create (made before anything touches a device, so each names its own reason with
or without a GPU), the host side of smplifyx_amd.vposer.VPoser(differentiable=True), and the host packing of
csrc/vposer_pack.h -- batch norms folded into the linear layers in double, both orientations, zero pads -- through the
stand-alone program tests/vposer_pack_check.cpp (host AddressSanitizer + UBSan) against a float64 numpy folding.
The device side is tests/test_gpu_vposer_encode.py."""
import os
import subprocess

import numpy as np
import pytest
import torch

from smplifyx_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NAMES = ("sfx_vposer_encoder_create", "sfx_vposer_encoder_destroy", "sfx_vposer_encode", "sfx_vposer_encode_backward")
ENC = ("enc_bn1_w", "enc_bn1_b", "enc_bn1_mean", "enc_bn1_var", "enc_fc1_w", "enc_fc1_b",
       "enc_bn2_w", "enc_bn2_b", "enc_bn2_mean", "enc_bn2_var", "enc_fc2_w", "enc_fc2_b",
       "enc_mu_w", "enc_mu_b", "enc_logvar_w", "enc_logvar_b")


@pytest.fixture(scope="module")
def weights():
    return synthetic.make_synthetic_vposer(0, encoder_inputs=63)


def test_the_four_entry_points_are_declared_bound_and_exported():
    from smplifyx_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "sfx.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "smplify-x-partial_amd", "libsfx.so")],
                              capture_output=True, text=True, check=True).stdout.split()
    for name in NAMES:
        assert name + "(" in hdr, name
        assert name in _capi.SYMBOLS, name
        assert hasattr(_capi.load(), name), name
        assert name in exported, name


def _shaped(latent=32, hidden=512, n_in=63):
    """Consistent random encoder weights of any shape (the Python layer checks consistency, the library the shape rule)."""
    rng = np.random.RandomState(5)
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    w = {}
    for name, n in (("enc_bn1", n_in), ("enc_bn2", hidden)):
        w[name + "_w"], w[name + "_b"], w[name + "_mean"] = f(n), f(n), f(n)
        w[name + "_var"] = (0.5 + rng.uniform(size=n)).astype(np.float32)
    w["enc_fc1_w"], w["enc_fc1_b"] = f(hidden, n_in), f(hidden)
    w["enc_fc2_w"], w["enc_fc2_b"] = f(hidden, hidden), f(hidden)
    w["enc_mu_w"], w["enc_mu_b"] = f(latent, hidden), f(latent)
    w["enc_logvar_w"], w["enc_logvar_b"] = f(latent, hidden), f(latent)
    return w


def _set(w, key, index, value):
    w = dict(w)
    w[key] = w[key].copy()
    w[key][index] = value
    return w


def test_every_refusal_returns_minus_one_with_its_own_text(weights):
    from smplifyx_amd import _capi, engine
    cases = [
        (_shaped(hidden=256), r"error -1: .*hidden 512.*got 32/256"),
        (_shaped(latent=30), r"error -1: .*multiple of 4.*got 30/512"),
        (_shaped(latent=64), r"error -1: .*got 64/512"),
        (_shaped(latent=0), r"error -1: .*got 0/512"),
        (_shaped(n_in=64), r"error -1: .*63 \(axis-angle\) or 189 \(rotation matrix\) inputs, got 64"),
        (_shaped(n_in=126), r"error -1: .*got 126"),
        (_set(weights, "enc_bn1_var", 7, -2e-5), r"error -1: .*bn1 running_var \+ 1e-5 <= 0 at 7"),
        (_set(weights, "enc_bn2_var", 300, -2.0), r"error -1: .*bn2 running_var \+ 1e-5 <= 0 at 300"),
        (_set(weights, "enc_bn1_mean", 3, np.nan), r"error -1: .*bn1 has a non-finite value at 3"),
        (_set(weights, "enc_bn2_w", 11, np.inf), r"error -1: .*bn2 has a non-finite value at 11"),
        (_set(weights, "enc_bn2_var", 0, np.inf), r"error -1: .*bn2 has a non-finite value at 0"),
    ]
    for w, pattern in cases:
        with pytest.raises(_capi.SfxError, match=pattern):
            engine.VPoserEncoder(w)
    # inconsistent arrays never reach the library
    with pytest.raises(ValueError, match="enc_bn1_var"):
        engine.VPoserEncoder(dict(weights, enc_bn1_var=weights["enc_bn1_var"][:60]))
    with pytest.raises(ValueError, match="carry no encoder"):
        engine.VPoserEncoder(synthetic.make_synthetic_vposer(0))


@pytest.mark.parametrize("n_in", (63, 189))
def test_create_with_valid_weights_needs_a_gpu(n_in):
    """No GPU: -3, 'no HIP device' (no CPU fallback).  With one: a handle that closes."""
    from smplifyx_amd import _capi, engine
    w = synthetic.make_synthetic_vposer(0, latent=12, encoder_inputs=n_in)
    if torch.cuda.is_available():
        enc = engine.VPoserEncoder(w)
        assert enc.latent == 12 and enc.n_in == n_in
        enc.close()
        enc.close()
        return
    with pytest.raises(_capi.SfxError, match="error -3: no HIP device"):
        engine.VPoserEncoder(w)


def test_differentiable_object_on_the_cpu_is_the_default_object(weights):
    from smplifyx_amd import vposer
    pose = torch.tensor((0.3 * np.random.RandomState(2).normal(size=(3, 63))).astype(np.float32), requires_grad=True)
    q0 = vposer.VPoser(weights).encode(pose)
    vp = vposer.VPoser(weights, differentiable=True)
    assert vp.differentiable and not vposer.VPoser(weights).differentiable
    q1 = vp.encode(pose)
    assert isinstance(q1, torch.distributions.Normal)
    assert torch.equal(q0.mean, q1.mean) and torch.equal(q0.stddev, q1.stddev)
    assert not q1.mean.requires_grad and not q1.stddev.requires_grad
    assert np.array_equal(q1.mean.numpy(), vposer.encode(weights, pose.detach().numpy()))
    q64 = vp.encode(pose.detach().double().view(3, 1, 21, 3))
    assert q64.mean.dtype == torch.float64 and q64.mean.shape == (3, 32)


def test_forward_without_the_flag_still_raises(weights):
    from smplifyx_amd import vposer
    with pytest.raises(NotImplementedError):
        vposer.VPoser(weights)(torch.zeros(2, 63))
    vp = vposer.VPoser(weights, differentiable=True)
    with pytest.raises(ValueError, match="matrot"):
        vp(torch.zeros(2, 63), output_type="matrot")
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # the decoder half has no host form
        vp(torch.zeros(2, 63))


def test_load_vposer_model_passes_the_flag_on(tmp_path):
    from smplifyx_amd import vposer
    fn = str(tmp_path / "vposer.npz")
    np.savez(fn, **synthetic.make_synthetic_vposer(0, latent=12, encoder_inputs=189))
    vp, cfg = vposer.load_vposer_model(fn, vp_model="snapshot", differentiable=True)
    assert cfg is None and vp.differentiable and vp.latentD == 12 and vp.weights["enc_fc1_w"].shape == (512, 189)
    assert not vposer.load_vposer_model(fn)[0].differentiable


@pytest.fixture(scope="module")
def pack_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vposer_pack") / "vposer_pack_check")
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17",
                    "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "vposer_pack_check.cpp"), "-o", exe], check=True)
    return exe


def _run_pack(exe, w, tmp_path):
    hidden, n_in = w["enc_fc1_w"].shape
    latent = w["enc_mu_w"].shape[0]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([latent, hidden, n_in], np.int32).tobytes())
        for k in ENC:
            f.write(np.ascontiguousarray(w[k], np.float32).tobytes())
    r = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:]
    blob = open(fout, "rb").read()
    ok, kin = np.frombuffer(blob[:8], np.int32)
    return int(ok), int(kin), blob[8:]


def _ulp_distance(a, b):
    """Distance in float32 units in the last place (finite values of one sign pattern or across zero)."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


@pytest.mark.parametrize("L,n_in", ((32, 63), (32, 189), (12, 189)))
def test_packing_equals_the_float64_numpy_folding(pack_check, tmp_path, L, n_in):
    w = synthetic.make_synthetic_vposer(0, latent=L, encoder_inputs=n_in)
    ok, kin, blob = _run_pack(pack_check, w, tmp_path)
    assert ok == 1 and kin == (64 if n_in == 63 else 192)
    H = 512
    sizes = (("w1T", (kin, H)), ("w2T", (H, H)), ("whT", (H, 128)), ("w1p", (H, kin)), ("w2", (H, H)), ("wh", (128, H)),
             ("b1", (H,)), ("b2", (H,)), ("bh", (128,)))
    got, off = {}, 0
    for name, shape in sizes:
        n = int(np.prod(shape))
        got[name] = np.frombuffer(blob[off * 4:(off + n) * 4], np.float32).reshape(shape)
        off += n
    assert off * 4 == len(blob)
    f = lambda k: w[k].astype(np.float64)
    for bn, fc, wp, wT, bp, n in (("enc_bn1", "enc_fc1", "w1p", "w1T", "b1", n_in), ("enc_bn2", "enc_fc2", "w2", "w2T", "b2", H)):
        s = f(bn + "_w") / np.sqrt(f(bn + "_var") + 1e-5)
        t = f(bn + "_b") - f(bn + "_mean") * s
        W = (f(fc + "_w") * s[None, :]).astype(np.float32)
        b = (f(fc + "_b") + f(fc + "_w") @ t).astype(np.float32)
        assert np.array_equal(got[wp][:, :n], W), (wp, float(np.abs(got[wp][:, :n] - W).max()))      # bit for bit
        assert np.array_equal(got[wT][:n, :], W.T), wT
        assert not got[wp][:, n:].any() and not got[wT][n:, :].any(), (wp, "pad")
        d = _ulp_distance(got[bp], b)                                  # another summation order than numpy's
        print("%s: max ulp distance %d" % (bp, d.max()))
        assert d.max() <= 1, (bp, int(d.max()))
    head = np.zeros((128, H), np.float32)
    head[:L], head[64:64 + L] = w["enc_mu_w"], w["enc_logvar_w"]
    bh = np.zeros(128, np.float32)
    bh[:L], bh[64:64 + L] = w["enc_mu_b"], w["enc_logvar_b"]
    assert np.array_equal(got["wh"], head) and np.array_equal(got["whT"], head.T) and np.array_equal(got["bh"], bh)
    assert not got["wh"][L:64].any() and not got["wh"][64 + L:].any() and not got["bh"][L:64].any() and not got["bh"][64 + L:].any()


def test_packing_refuses_through_the_stand_alone_program_too(pack_check, tmp_path, weights):
    ok, kin, blob = _run_pack(pack_check, _set(weights, "enc_bn1_var", 62, -1.0), tmp_path)
    assert ok == 0 and b"bn1 running_var + 1e-5 <= 0 at 62" in blob
