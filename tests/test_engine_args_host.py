"""CPU tests of the Python bindings' shared pieces (no GPU, no compute): the tensor checker and the pair parser of _args, the
handle base of _capi, the packing of FrameBatch.set_frames / set_params in both modes, and what the stand-alone objective
refuses before it needs a device."""
import types

import numpy as np
import pytest
import torch


# ---------------------------------------------------------------- 1. the checker
def _cpu_only(**kw):
    """_args.tensor on a CPU tensor that passes every other test: the last refusal is the device's."""
    from smplifyx_amd import _args
    with pytest.raises(ValueError, match="no CPU fallback"):
        _args.tensor("x", torch.zeros(2, 3), **kw)


def test_checker_refuses_by_class_and_message():
    from smplifyx_amd import _args
    x = torch.zeros(2, 3)
    for cls in (TypeError, ValueError):
        with pytest.raises(cls, match="x: a torch tensor is needed, got list"):
            _args.tensor("x", [[0.0] * 3] * 2, (None, 3), non_tensor=cls)
    with pytest.raises(TypeError):                                  # the default class
        _args.tensor("x", np.zeros((2, 3), np.float32), (None, 3))
    _cpu_only(shape=(None, 3))
    _cpu_only(shape=(2, 3))
    for shape, want in (((None, 4), r"\('B', 4\)"), ((3, 3), r"\(3, 3\)"), ((None, 2, 3), r"\('B', 2, 3\)"), ((None,), r"\('B',\)")):
        with pytest.raises(ValueError, match=r"x: shape \(2, 3\), expected " + want):      # trailing, batch, rank (both ways)
            _args.tensor("x", x, shape)
    with pytest.raises(ValueError, match="x: float32 is needed, got torch.float64"):
        _args.tensor("x", x.double(), (None, 3))
    _cpu_only(shape=(None, 3), dtype=torch.float32, convert=False)
    with pytest.raises(ValueError, match="no CPU fallback"):        # "convert" lets the float64 tensor through to the device test
        _args.tensor("x", x.double(), (None, 3), convert=True)
    with pytest.raises(ValueError, match="x: int32 is needed, got torch.float32"):
        _args.tensor("x", x, (None, 3), dtype=torch.int32)
    xt = torch.zeros(3, 2).t()
    assert tuple(xt.shape) == (2, 3) and not xt.is_contiguous()
    with pytest.raises(ValueError, match=r"x: a contiguous tensor is needed \(strides \(1, 2\)\)"):
        _args.tensor("x", xt, (None, 3))
    with pytest.raises(ValueError, match="no CPU fallback"):
        _args.tensor("x", xt, (None, 3), make_contiguous=True)
    assert _args.tensor("x", None, (None, 3), optional=True) is None
    with pytest.raises(TypeError, match="got NoneType"):
        _args.tensor("x", None, (None, 3))
    with pytest.raises(ValueError, match="got NoneType"):
        _args.tensor("x", None, (None, 3), non_tensor=ValueError)


def test_output_tensor_and_pointer_helpers():
    from smplifyx_amd import _args
    cpu = torch.device("cpu")
    new = _args.out_tensor("out", None, (2, 3), cpu)
    assert tuple(new.shape) == (2, 3) and new.dtype == torch.float32 and new.is_contiguous()
    mine = torch.zeros(2, 3)
    assert _args.out_tensor("out", mine, (2, 3), cpu) is mine
    for bad in (torch.zeros(2, 4), torch.zeros(2, 3, dtype=torch.float64), torch.zeros(3, 2).t(), [0.0]):
        with pytest.raises(ValueError, match=r"out: a contiguous float32 \(2, 3\) tensor on cpu is needed"):
            _args.out_tensor("out", bad, (2, 3), cpu)
    assert _args.ptr(None) is None
    assert _args.ptr(mine).value == mine.data_ptr()
    assert _args.stream(1234).value == 1234                          # a given stream is passed through untouched


# ---------------------------------------------------------------- 2. the stand-alone objective, as far as a CPU reaches
def _objective_args(joints, **kw):
    B, K = 2, 3
    a = dict(joints=joints, rotation=torch.zeros(B, 3, 3), translation=torch.zeros(B, 3), focal_x=torch.ones(B),
             focal_y=torch.ones(B), center=torch.zeros(B, 2), gt_joints=torch.zeros(B, K, 2), joint_weights=torch.ones(B, K),
             body_pose=torch.zeros(B, 63), prior=torch.zeros(B, 32), betas=torch.zeros(B, 10), joints_conf=torch.ones(B, K),
             use_hands=False, use_face=False)
    a.update(kw)
    return a


def _camera_args(joints, **kw):
    B, K = 2, 3
    a = dict(joints=joints, rotation=torch.zeros(B, 3, 3), translation=torch.zeros(B, 3), focal_x=torch.ones(B),
             focal_y=torch.ones(B), center=torch.zeros(B, 2), gt_joints=torch.zeros(B, K, 2), init_count=torch.ones(K))
    a.update(kw)
    return a


@pytest.mark.parametrize("which", ("objective_eval", "camera_init_eval"))
def test_objective_refusals_reachable_without_a_device(which):
    """The joints are vetted first -- rank, K, device -- so without a GPU every call ends there.  The checks behind them
    (prior_form, weights, use_joints_conf: tests/test_gpu_objective.py) are not reached: a CPU `joints` is what the message
    names, whatever else is wrong with the call."""
    from smplifyx_amd import engine
    fn, args = getattr(engine, which), (_objective_args if which == "objective_eval" else _camera_args)
    big = engine.OBJECTIVE_MAX_K + 1
    assert engine.OBJECTIVE_MAX_K == 512
    for joints, msg in ((torch.zeros(2, 9), r"joints: shape \(2, 9\), expected \(B, K, 3\)"),
                        (torch.zeros(2, 3, 2), r"joints: shape \(2, 3, 2\), expected \(B, K, 3\)"),
                        ([[0.0] * 3] * 3, r"joints: shape \(\), expected \(B, K, 3\)"),
                        (torch.zeros(0, 3, 3), "joints: at least one frame is needed, got B = 0"),
                        (torch.zeros(2, 0, 3), r"joints: K = 0 keypoints, supported 1\.\.512"),
                        (torch.zeros(2, big, 3), r"joints: K = 513 keypoints, supported 1\.\.512"),
                        (torch.zeros(2, 3, 3), r"joints: a CUDA tensor is needed \(no CPU fallback\), got device cpu")):
        with pytest.raises(ValueError, match=msg):
            fn(**args(joints))
    cpu = torch.zeros(2, 3, 3)
    others = (dict(prior_form="spline"), dict(weights=dict(data_weight=1.0, momentum=0.9)), dict(joints_conf=None, use_joints_conf=True)) \
        if which == "objective_eval" else (dict(joints_conf=None, use_conf=True),)
    for kw in others:
        with pytest.raises(ValueError, match=r"joints: a CUDA tensor is needed \(no CPU fallback\)"):
            fn(**args(cpu, **kw))


# ---------------------------------------------------------------- 3. the handle base
def _stub_handle(destroy):
    from smplifyx_amd import _capi

    class Stub(_capi.Handle):
        _destroy = "stub_destroy"

        def __init__(self, h):
            self._lib = types.SimpleNamespace(stub_destroy=destroy)
            if h is not None:
                self._h = h
    return Stub


def test_handle_base_releases_once_and_never_raises_from_del():
    calls = []
    Stub = _stub_handle(calls.append)
    s = Stub(41)
    s.close()
    s.close()
    assert calls == [41] and s._h is None
    Stub(None).close()                                               # _h never set: nothing to release
    assert calls == [41]
    Stub(42).__del__()
    assert calls == [41, 42]
    bare = Stub.__new__(Stub)                                        # an __init__ that raised before anything was set
    bare.close()
    bare.__del__()
    assert calls == [41, 42]

    def boom(h):
        calls.append(h)
        raise RuntimeError("destroy failed")
    Boom = _stub_handle(boom)
    with pytest.raises(RuntimeError, match="destroy failed"):
        Boom(43).close()
    b = Boom(44)
    b.__del__()                                                      # swallowed
    b.__del__()
    assert calls == [41, 42, 43, 44]


def test_every_engine_handle_derives_from_the_base():
    from smplifyx_amd import _capi, engine
    want = dict(DeviceModel="sfx_model_destroy", VPoserDecoder="sfx_vposer_destroy", VPoserEncoder="sfx_vposer_encoder_destroy",
                FrameBatch="sfx_batch_destroy", BatchOptimizer="sfx_opt_destroy", Penetration="sfx_pen_destroy")
    for name, sym in want.items():
        cls = getattr(engine, name)
        assert issubclass(cls, _capi.Handle) and cls._destroy == sym and sym in _capi.SYMBOLS, name
        assert "close" not in vars(cls) and "__del__" not in vars(cls), name


# ---------------------------------------------------------------- 4. packing
B, K = 2, 3
KP, FOCAL, CENTER = 0.1, 1000.1, (320.25, 240.75)


def _frames(mode, **kw):
    from smplifyx_amd import engine
    a = dict(keypoints=np.full((B, K, 3), KP), joint_weights=np.array([1.0, 0.5, 0.25]), cam_init_mask=np.array([1.0, 0.0, 1.0]),
             focal=FOCAL, center=np.tile(CENTER, (B, 1)), data_weight=1.0)
    a.update(kw)
    return engine._pack_frames(mode, B, K, **a)


def test_pack_frames_float32_is_todays_arrays():
    from smplifyx_amd import engine
    rot = np.arange(18, dtype=np.float64).reshape(B, 3, 3) * 0.1
    kp, jw, cm, cam, R = _frames(engine._F32, est_tz=np.array([12.1, 24.3]), cam_rot=rot)
    want_cam = np.zeros((B, 6), np.float32)
    want_cam[:, 0] = want_cam[:, 1] = np.float32(FOCAL)
    want_cam[:, 2:4] = np.asarray(CENTER, np.float32)
    want_cam[:, 4] = np.float32(1.0)
    want_cam[:, 5] = np.asarray([12.1, 24.3], np.float32)
    for got, want in ((kp, np.full((B, K, 3), KP).astype(np.float32)), (jw, np.tile(np.float32([1.0, 0.5, 0.25]), (B, 1))),
                      (cm, np.tile(np.float32([1.0, 0.0, 1.0]), (B, 1))), (cam, want_cam), (R, rot.astype(np.float32).reshape(B, 9))):
        assert got.dtype == np.float32 and got.flags["C_CONTIGUOUS"] and got.shape == want.shape and np.array_equal(got, want)
    kp, jw, cm, cam, R = _frames(engine._F32)
    assert np.array_equal(cam[:, 5], np.zeros(B, np.float32))                                  # est_tz=None
    assert R.dtype == np.float32 and np.array_equal(R, np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (B, 1)))     # cam_rot=None


def test_pack_frames_float64_widens_the_data_and_keeps_the_camera():
    from smplifyx_amd import engine
    rot = np.arange(18, dtype=np.float64).reshape(B, 3, 3) * 0.1
    kp, jw, cm, cam, R = _frames(engine._F64, joint_weights=np.array([[0.1, 0.5, 0.25]]), est_tz=np.array([12.1, 24.3]), cam_rot=rot)
    for a in (kp, jw, cm, cam, R):
        assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    assert np.float64(np.float32(KP)) != KP
    assert kp.shape == (B, K, 3) and (kp == np.float64(np.float32(KP))).all()                  # through fp32, not 0.1
    assert jw.shape == (B, K) and np.array_equal(jw, np.tile(np.float64(np.float32([0.1, 0.5, 0.25])), (B, 1)))       # one frame's weights, both frames
    assert np.array_equal(cm, np.tile([1.0, 0.0, 1.0], (B, 1)))
    assert (cam[:, 0] == 1000.1).all() and (cam[:, 1] == 1000.1).all() and np.float64(np.float32(FOCAL)) != FOCAL      # the camera in double directly
    assert np.array_equal(cam[:, 2:4], np.tile(CENTER, (B, 1))) and (cam[:, 4] == 1.0).all()
    assert np.array_equal(cam[:, 5], [12.1, 24.3])
    assert np.array_equal(R, rot.astype(np.float32).astype(np.float64).reshape(B, 9)) and not np.array_equal(R, rot.reshape(B, 9))
    kp, jw, cm, cam, R = _frames(engine._F64)
    assert (cam[:, 5] == 0).all()
    assert R.dtype == np.float64 and np.array_equal(R, np.tile(np.eye(3).reshape(1, 9), (B, 1)))


@pytest.mark.parametrize("mode", ("_F32", "_F64"))
def test_pack_frames_focal_is_a_number_one_per_frame_or_a_pair_per_frame(mode):
    """focal: a number or [B] fills fx = fy; [B, 2] = (fx, fy) fills cam[:, 0] and cam[:, 1] separately; the mode's own dtype
    (float64 keeps a value that is no fp32 number); any other shape is refused by name, nothing is broadcast silently."""
    from smplifyx_amd import engine
    m = getattr(engine, mode)
    fx, fy = np.array([1000.1, 2400.3]), np.array([950.7, 2400.9])
    rnd = (lambda v: np.asarray(v, np.float64)) if mode == "_F64" else (lambda v: np.asarray(v, np.float32))
    assert mode == "_F32" or np.float64(np.float32(fx[0])) != fx[0]
    cam = _frames(m, focal=np.stack([fx, fy], 1))[3]
    assert cam.dtype == m.dtype and cam.shape == (B, 6)
    assert np.array_equal(cam[:, 0], rnd(fx)) and np.array_equal(cam[:, 1], rnd(fy)) and not np.array_equal(cam[:, 0], cam[:, 1])
    assert np.array_equal(cam[:, 2:4], np.tile(rnd(CENTER), (B, 1))) and (cam[:, 4] == 1.0).all() and (cam[:, 5] == 0).all()
    cam = _frames(m, focal=fx)[3]                                                                # [B]: one focal per frame
    assert np.array_equal(cam[:, 0], rnd(fx)) and np.array_equal(cam[:, 1], rnd(fx))
    for scalar in (FOCAL, np.float64(FOCAL), np.array(FOCAL)):
        cam = _frames(m, focal=scalar)[3]
        assert (cam[:, 0] == rnd(FOCAL)).all() and (cam[:, 1] == rnd(FOCAL)).all()
    cam = _frames(m, focal=[[5.0, 6.0], [7.0, 8.0]])[3]                                          # (a list of pairs is an array)
    assert cam[:, :2].tolist() == [[5.0, 6.0], [7.0, 8.0]]
    for bad in (np.ones(1), np.ones(B + 1), np.ones((1, 2)), np.ones((B, 1)), np.ones((B, 3)), np.ones((2, B, 2)), np.ones((B + 1, 2)),
                np.ones(0)):
        with pytest.raises(ValueError, match=r"focal must be a number, \[B\] or \[B, 2\] = \(fx, fy\) with B = 2, got shape "
                                             + str(tuple(bad.shape)).replace("(", r"\(").replace(")", r"\)")):
            _frames(m, focal=bad)


@pytest.mark.parametrize("mode", ("_F32", "_F64"))
def test_pack_params_broadcasts_and_rounds_only_what_it_did(mode):
    from smplifyx_amd import engine
    m = getattr(engine, mode)
    sizes = dict(cam_translation=3, global_orient=3, betas=10, left_hand_pose=12, right_hand_pose=12, expression=10, jaw_pose=3,
                 leye_pose=3, reye_pose=3, pose_embedding=32)
    betas = np.full((1, 10), 0.1)
    args, reg = engine._pack_params(m, B, sizes, 32, np.full(32, 0.1), dict(betas=betas, jaw_pose=None, global_orient=np.ones((B, 3))))
    assert len(args) == len(engine.PARAM_NAMES)
    by_name = dict(zip(engine.PARAM_NAMES, args))
    assert [n for n, a in by_name.items() if a is not None] == ["global_orient", "betas"]
    b = by_name["betas"]
    assert b.dtype == m.dtype and b.shape == (B, 10) and b.flags["C_CONTIGUOUS"]
    through_fp32 = np.float64(np.float32(0.1))
    assert through_fp32 != 0.1
    assert (b.astype(np.float64) == (0.1 if mode == "_F64" else through_fp32)).all()      # float64 keeps a value that is no fp32 number
    assert reg.dtype == m.dtype and reg.shape == (B, 32) and reg.flags["C_CONTIGUOUS"]
    assert (reg.astype(np.float64) == through_fp32).all()                   # the regression pose goes through fp32 in both
    args, reg = engine._pack_params(m, B, sizes, 32, None, {})
    assert args == [None] * 10 and reg is None


# ---------------------------------------------------------------- 5. the pair parser
def test_ign_part_pairs_parser():
    from smplifyx_amd import _args
    got = _args.ign_pairs(["9,16", (1, 2)])
    assert got.dtype == np.int32 and got.flags["C_CONTIGUOUS"] and got.tolist() == [[9, 16], [1, 2]]
    for nothing in ([], None, ()):
        e = _args.ign_pairs(nothing)
        assert e.dtype == np.int32 and e.shape == (0, 2)


# ---------------------------------------------------------------- 6. the bounded cache of the device calls' entries
def test_bounded_cache_evicts_the_oldest_and_a_hit_makes_an_entry_recent():
    import collections
    from smplifyx_amd import engine
    cache, made = collections.OrderedDict(), []

    def get(key):
        return engine._cached(cache, key, lambda: made.append(key) or [key], size=3)
    ents = {k: get(k) for k in "abcd"}
    assert list(cache) == ["b", "c", "d"] and "a" not in cache               # four keys, size 3: the first is gone
    assert get("b") is ents["b"] and list(cache) == ["c", "d", "b"]          # a hit marks the entry recent ...
    get("e")
    assert list(cache) == ["d", "b", "e"]                                    # ... so the next insert evicts another
    assert get("d") is ents["d"] and get("b") is ents["b"]
    assert made == ["a", "b", "c", "d", "e"]                                 # made once per resident key
    assert get("a") is not ents["a"] and made[-1] == "a"                     # an evicted key is made again
    with pytest.raises(KeyError):                                            # a make() that raises leaves no entry
        engine._cached(cache, "z", lambda: {}["z"], size=3)
    assert "z" not in cache and len(cache) == 3
    assert engine._cached.__defaults__ == (8,)                               # the size the device calls run with
