"""CPU tests of the differentiable SMPL-X forward's plumbing (no GPU, no compute): the C ABI binding of sfx_lbs_backward and the
`differentiable` flag of the smplx drop-in."""
import ctypes as C

import pytest
import torch


def test_lbs_backward_is_bound_with_the_documented_signature():
    """model, B, nine inputs, dvertices, djoints, nine gradients, stream: 21 pointer arguments plus B and the stream."""
    from smplifyx_amd import _capi
    assert "sfx_lbs_backward" in _capi.SYMBOLS
    res, args = _capi.SYMBOLS["sfx_lbs_backward"]
    assert res is C.c_int
    assert len(args) == 23
    assert args[1] is C.c_int32
    pointers = args[:1] + args[2:-1]
    assert len(pointers) == 21 and all(a is C.c_void_p for a in pointers)
    assert args[-1] is C.c_void_p
    lib = _capi.load()
    assert hasattr(lib, "sfx_lbs_backward")


def test_engine_names_the_nine_gradients_like_the_reference():
    from smplifyx_amd import engine
    assert engine.DeviceModel.LBS_INPUTS == ("global_orient", "body_pose", "betas", "expression", "jaw_pose", "leye_pose",
                                             "reye_pose", "left_hand_pose", "right_hand_pose")
    assert callable(engine.DeviceModel.lbs_backward)


def test_differentiable_model_constructs_without_a_gpu(synth_model):
    from smplifyx_amd import smplx
    plain = smplx.create(synth_model, batch_size=2)
    diff = smplx.create(synth_model, batch_size=2, differentiable=True)
    assert plain.differentiable is False and diff.differentiable is True
    assert [n for n, _ in diff.named_parameters()] == [n for n, _ in plain.named_parameters()]
    if torch.cuda.is_available():
        return              # (with a GPU the forward runs: tests/test_gpu_lbs_backward.py)
    errs = []
    for m in (plain, diff):
        with pytest.raises(RuntimeError, match="needs a GPU") as e:
            m()
        errs.append(str(e.value))
    assert errs[0] == errs[1]
