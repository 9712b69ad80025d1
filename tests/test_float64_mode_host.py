"""CPU tests of the float64 mode (sfx_batch_cfg.high_precision = 2): its C ABI bindings and the host-side validation of
FrameBatch(precision=...) (engine.check_precision).  No GPU needed."""
import ctypes as C

import pytest

import helpers as H

F64_ENTRIES = ("sfx_batch_set_stage_weights_f64", "sfx_batch_set_frames_f64", "sfx_batch_set_params_f64",
               "sfx_batch_get_params_f64", "sfx_batch_closure_f64", "sfx_batch_get_grad_f64")


def _body_cfg(**over):
    cfg = H.load_cfg("fit_smplx_combined_coco25.yaml", use_hands=False, use_face=False)
    cfg.update(float_dtype="float64")
    cfg.update(over)
    return cfg


def test_capi_binds_the_float64_entries_with_double_pointers():
    from smplifyx_amd import _capi
    f64p = C.POINTER(C.c_double)
    for name in F64_ENTRIES:
        assert name in _capi.SYMBOLS, name
        res, args = _capi.SYMBOLS[name]
        assert res is C.c_int
        if name == "sfx_batch_set_stage_weights_f64":
            assert args[1]._type_ is _capi.StageWeights64
            assert all(t is C.c_double or getattr(t, "_type_", None) is C.c_double for _, t in _capi.StageWeights64._fields_)
            continue
        reals = [a for a in args if a not in (C.c_void_p, C.c_int32)]
        assert reals and all(a is f64p for a in reals), (name, reals)
    assert C.sizeof(_capi.StageWeights64) == 11 * 8      # = sizeof(sfx_stage_weights_f64)


def test_float64_accepts_the_body_only_rows_configuration():
    from smplifyx_amd import engine
    cfg = _body_cfg()
    assert not cfg["use_vposer"] and not cfg["interpenetration"]
    assert engine.check_precision(cfg, "rows", precision="float64") == 2
    assert engine.check_precision(cfg, "rows", has_regression_pose=True, precision="float64") == 2


@pytest.mark.parametrize("setting,over,lbs_mode,has_reg", [
    ("use_vposer", dict(use_vposer=True), "rows", True),
    ("use_hands", dict(use_hands=True), "rows", True),
    ("use_face", dict(use_face=True), "rows", True),
    ("interpenetration", dict(interpenetration=True), "rows", True),
    ("lbs_mode", {}, "dense", True),
    ("float_dtype", dict(float_dtype="float32"), "rows", True),
    ("GMM", {}, "rows", False),
])
def test_float64_refuses_unsupported_settings(setting, over, lbs_mode, has_reg):
    from smplifyx_amd import engine
    with pytest.raises(ValueError, match=setting):
        engine.check_precision(_body_cfg(**over), lbs_mode, has_regression_pose=has_reg, precision="float64")


def test_unknown_precision_is_refused():
    from smplifyx_amd import engine
    with pytest.raises(ValueError, match="precision"):
        engine.check_precision(_body_cfg(), "rows", precision="float128")


@pytest.mark.parametrize("precision", [None, "mixed"])
@pytest.mark.parametrize("dtype,mode", [("float32", 0), ("float64", 1)])
def test_mixed_precision_maps_float_dtype_as_before(precision, dtype, mode):
    """precision missing or "mixed": cfg float_dtype picks high_precision 0 or 1, whatever else the cfg holds -- a cfg key
    `precision` included (the float64 mode is an engine-level FrameBatch option, never selected from a cfg)."""
    from smplifyx_amd import engine
    kw = {} if precision is None else {"precision": precision}
    for cfg in (H.load_cfg("fit_smplx_combined_coco25.yaml", float_dtype=dtype),
                H.load_cfg("fit_smplx_combined_coco25.yaml", float_dtype=dtype, use_hands=False, use_face=False),
                H.load_cfg("fit_smplx_combined_coco25.yaml", float_dtype=dtype, use_hands=False, use_face=False, precision="float64")):
        for lbs_mode in ("rows", "dense"):
            assert engine.check_precision(cfg, lbs_mode, **kw) == mode
            assert engine.check_precision(cfg, lbs_mode, has_regression_pose=False, **kw) == mode


def test_stage_weights_keep_the_cfg_floats_in_double():
    from smplifyx_amd import _capi, engine
    cfg = _body_cfg(body_pose_prior_weights=[404.0, 57.4, 4.78], shape_weights=[100.0, 50.0, 10.0])
    w32, n32 = engine.stage_weights_from_cfg(cfg)
    w64, n64 = engine.stage_weights_from_cfg(cfg, _capi.StageWeights64)
    assert n32 == n64 and len(w32) == len(w64)
    assert [w.body_pose_weight for w in w64] == [404.0, 57.4, 4.78]
    assert any(w.body_pose_weight != a.body_pose_weight for w, a in zip(w64, w32))      # 57.4 is not an fp32 number
    assert all(w.bending_prior_weight < 0 for w in w64)
    widened = engine.widen_stage_weights(w32)
    assert [w.body_pose_weight for w in widened] == [a.body_pose_weight for a in w32]
