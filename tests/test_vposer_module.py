"""CPU tests of the stand-alone VPoser surface: the four sfx_vposer_* entry points in the binding, their refusals on a box
without a GPU, and the host side of smplifyx_amd.vposer.VPoser (encode, load_vposer_model, the argument checks of decode).
The device side is tests/test_gpu_vposer_batch.py."""
import numpy as np
import pytest
import torch

from smplifyx_amd import synthetic


@pytest.fixture(scope="module")
def weights():
    return synthetic.make_synthetic_vposer(0, encoder_inputs=63)


def test_the_four_entry_points_are_bound():
    from smplifyx_amd import _capi
    for name in ("sfx_vposer_create", "sfx_vposer_destroy", "sfx_vposer_decode", "sfx_vposer_decode_backward"):
        assert name in _capi.SYMBOLS, name
        assert hasattr(_capi.load(), name), name


def test_create_refuses_a_bad_shape_with_its_own_message(weights):
    """hidden 256: refused before anything touches a device, so the message names the shape with or without a GPU."""
    from smplifyx_amd import _capi, engine
    w = dict(weights)
    w["fc1_w"], w["fc1_b"] = weights["fc1_w"][:256], weights["fc1_b"][:256]
    w["fc2_w"], w["fc2_b"] = weights["fc2_w"][:256, :256], weights["fc2_b"][:256]
    w["out_w"] = weights["out_w"][:, :256]
    with pytest.raises(_capi.SfxError, match=r"hidden 512.*got 32/256"):
        engine.VPoserDecoder(w)
    w = synthetic.make_synthetic_vposer(0, latent=32)
    w["fc1_w"] = np.ascontiguousarray(w["fc1_w"][:, :30])
    with pytest.raises(_capi.SfxError, match=r"got 30/512"):
        engine.VPoserDecoder(w)


def test_create_with_valid_weights_needs_a_gpu(weights):
    """No GPU: SfxError, as sfx_model_create (no CPU fallback).  With one: a handle that closes."""
    from smplifyx_amd import _capi, engine
    if torch.cuda.is_available():
        dec = engine.VPoserDecoder(weights)
        assert dec.latent == 32
        dec.close()
        dec.close()
        return
    with pytest.raises(_capi.SfxError, match="no HIP device"):
        engine.VPoserDecoder(weights)


def test_decode_argument_checks_need_no_device(weights):
    from smplifyx_amd.vposer import VPoser
    vp = VPoser(weights).to("cpu").eval()
    assert vp.latentD == 32 and vp.weights["fc1_w"].shape == (512, 32)
    z = torch.zeros(2, 32)
    with pytest.raises(ValueError, match="matrot"):
        vp.decode(z, output_type="matrot")          # before the device check
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vp.decode(z, output_type="aa")


def test_encode_returns_the_normal_the_reference_samples_from(weights):
    from oracle.vposer import VPoserEncoderRef
    from smplifyx_amd import vposer
    rng = np.random.RandomState(2)
    pose = (0.3 * rng.normal(size=(3, 63))).astype(np.float32)
    vp = vposer.VPoser(weights)
    q = vp.encode(torch.tensor(pose))
    assert isinstance(q, torch.distributions.Normal)
    assert q.mean.dtype == torch.float32 and q.mean.shape == (3, 32) and not q.mean.requires_grad
    assert np.array_equal(q.mean.numpy(), vposer.encode(weights, pose))
    ref = VPoserEncoderRef(weights).encode(torch.tensor(pose, dtype=torch.float64))
    np.testing.assert_allclose(q.stddev.numpy(), ref.stddev.detach().numpy(), rtol=1e-5, atol=1e-6)
    mu, sigma = vposer.encode_stats(weights, pose)
    assert mu.dtype == np.float64 and np.array_equal(mu.astype(np.float32), q.mean.numpy())
    np.testing.assert_allclose(sigma, ref.stddev.detach().numpy(), rtol=1e-5, atol=1e-6)
    torch.manual_seed(0)
    s = q.sample()
    assert s.shape == (3, 32) and torch.isfinite(s).all() and not torch.equal(s, q.mean)
    q64 = vp.encode(torch.tensor(pose, dtype=torch.float64).view(3, 21, 3))
    assert q64.mean.dtype == torch.float64 and q64.stddev.dtype == torch.float64


def test_load_vposer_model_returns_the_tuple_the_reference_unpacks(weights, tmp_path):
    from smplifyx_amd import vposer
    w12 = synthetic.make_synthetic_vposer(0, latent=12)
    fn = str(tmp_path / "vposer.npz")
    np.savez(fn, **w12)
    vp, cfg = vposer.load_vposer_model(fn, vp_model="snapshot")
    assert isinstance(vp, vposer.VPoser) and cfg is None
    assert vp.latentD == 12
    assert np.array_equal(vp.weights["out_w"], w12["out_w"])
    assert vp.to("cpu") is vp and vp.eval() is vp
