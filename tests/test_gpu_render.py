"""GPU tests of the mesh rasteriser (sfx_render_meshes, csrc/raster.hip; engine.render_meshes; utils.render_mesh /
optimization_visualization; driver.render_overlays; the render_overlays key of main and fit_single_frame) against the numpy oracle
of tests/raster_common.py.

Images are 75 x 53 (W no multiple of 64, H odd: several workgroups per image, a ragged last one) and 160 x 120 for the body.
Tolerances come from the number formats, not from what the kernels give:
  projection   10 x the error of the same formula evaluated in float32 numpy against float64
  coverage     exact.  The oracle is fed the device's OWN float32 screen positions (checked in the projection test), so both
               sides snap the same numbers and the integer coverage must agree at every pixel
  visibility   the winning triangle agrees wherever the oracle's nearest and second-nearest depths differ by more than 1e-4
               relative (float32 depth error is of order 1e-6); such near ties may be at most 0.5 % of the covered pixels
  depth        10 x the error of the float32-numpy depth against float64
  colour       +-1 level per channel where the triangle agrees (the shading is float32 on the device, float64 in the oracle);
               alpha exactly 0 or 255; background bytes copied exactly
Every test here fails on a library without the sfx_render_meshes symbol."""
import os
import pickle

import numpy as np
import pytest
import torch

import helpers as H
import raster_common as RC

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HS, WS = 53, 75
NEAR_TIE = 1e-4
ALL = ("rgba", "depth", "tri", "screen", "dropped")


def _rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _gpu(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device="cuda").to(dtype).contiguous()


def render(verts, faces, t, focal, center, Hh, Ww, R=None, bg=None, want=ALL, **kw):
    """engine.render_meshes on host arrays ([B, ...]); numpy results."""
    from smplifyx_amd import engine
    out = engine.render_meshes(_gpu(verts), faces, _gpu(t), _gpu(focal), _gpu(center), Hh, Ww, rotation=_gpu(R),
                               background=_gpu(bg, torch.uint8), want=want, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _scene(name):
    """(verts float32 [V, 3], faces, t [3], focal [2], center [2], R [3, 3], H, W)"""
    from smplifyx_amd import synthetic
    ico_v, ico_f = RC.icosphere(2)
    if name == "icosphere":
        assert ico_v.shape == (162, 3) and ico_f.shape == (320, 3)
        return (ico_v.astype(np.float32), ico_f, np.array([0.12, -0.07, 3.0], np.float32), np.array([61.0, 58.0], np.float32),
                np.array([WS / 2 + 0.3, HS / 2 - 0.2], np.float32), _rot([1, 2, 3], 0.4).astype(np.float32), HS, WS)
    if name == "two spheres":
        v = np.concatenate([ico_v, 0.8 * ico_v @ _rot([0, 1, 1], 0.3).T + np.array([0.7, 0.2, -0.3])])
        return (v.astype(np.float32), np.concatenate([ico_f, ico_f + 162]), np.array([-0.3, 0.05, 3.2], np.float32),
                np.array([55.0, 55.0], np.float32), np.array([WS / 2, HS / 2], np.float32), None, HS, WS)
    if name == "body":
        if not synthetic.topology_available():
            pytest.skip("tests/golden/smplx_topology.npz is a local build product (tools/make_topology.py)")
        tp = synthetic.load_topology()
        v = np.asarray(tp["vertices"], np.float64)
        v = (v - (v.max(0) + v.min(0)) / 2.0).astype(np.float32)
        extent = float(np.ptp(v, axis=0)[:2].max())
        return (v, np.asarray(tp["faces"], np.int64), np.array([0.02, 0.01, 3.0], np.float32),
                np.full(2, 0.85 * 120 * 3.0 / extent, np.float32), np.array([80.0, 60.0], np.float32),
                _rot([0, 1, 0], 0.5).astype(np.float32), 120, 160)
    raise KeyError(name)


_memo = {}


def scene(name):
    """The scene, the device's render of it and the oracle's rasterisation of the device's screen positions: made once."""
    if name not in _memo:
        v, f, t, focal, c, R, Hh, Ww = _scene(name)
        dev = render(v[None], f, t[None], focal[None], c[None], Hh, Ww, R=None if R is None else R[None])
        ras = RC.rasterize(dev["screen"][0], f, Hh, Ww)
        _memo[name] = dict(v=v, f=f, t=t, focal=focal, c=c, R=R, H=Hh, W=Ww, dev=dev, ras=ras)
    return _memo[name]


def near_ties(ras):
    with np.errstate(invalid="ignore"):
        return (ras["tri"] >= 0) & np.isfinite(ras["second"]) & (ras["second"] - ras["depth"] <= NEAR_TIE * ras["depth"])


def check_against_oracle(name, dev, ras, b=0):
    """Coverage exact, visibility up to near ties, depth at 10 x the float32 formula's error.  Returns the agreeing pixels."""
    tri, depth = dev["tri"][b], dev["depth"][b]
    covered = ras["tri"] >= 0
    n_cov = int(covered.sum())
    assert n_cov > 300, (name, n_cov)
    assert np.array_equal(tri >= 0, covered), (name, np.argwhere((tri >= 0) != covered)[:8].tolist())
    ties = near_ties(ras)
    share = ties.sum() / float(n_cov)
    print("%s: %d covered pixels, %d near ties (%.3f %%)" % (name, n_cov, ties.sum(), 100 * share))
    assert share <= 0.005, (name, share)
    wrong = covered & ~ties & (tri != ras["tri"])
    assert not wrong.any(), (name, int(wrong.sum()), np.argwhere(wrong)[:8].tolist())
    agree = covered & (tri == ras["tri"])
    err32 = np.abs(ras["depth32"][agree].astype(np.float64) - ras["depth"][agree]).max()
    err = np.abs(depth[agree].astype(np.float64) - ras["depth"][agree]).max()
    print("%s: depth error %.3e, float32 numpy %.3e" % (name, err, err32))
    assert err32 > 0 and err <= 10 * err32, (name, err, err32)
    assert np.isposinf(depth[~covered]).all() and (tri[~covered] == -1).all()
    return agree


@pytest.mark.parametrize("name", ["icosphere", "two spheres", "body"])
def test_projection(name):
    from smplifyx_amd.camera import PerspectiveCamera
    s = scene(name)
    p64 = RC.project(s["v"], s["t"], s["focal"], s["c"], s["R"], np.float64)
    p32 = RC.project(s["v"], s["t"], s["focal"], s["c"], s["R"], np.float32)
    bound = 10 * np.abs(p32.astype(np.float64) - p64).max()
    err = np.abs(s["dev"]["screen"][0].astype(np.float64) - p64).max()
    print("%s: projection error %.3e, 10 x float32 numpy %.3e" % (name, err, bound))
    assert bound > 0 and err <= bound
    cam = PerspectiveCamera(rotation=None if s["R"] is None else torch.as_tensor(s["R"])[None], translation=torch.as_tensor(s["t"])[None],
                            focal_length_x=torch.as_tensor(s["focal"][:1]), focal_length_y=torch.as_tensor(s["focal"][1:]),
                            center=torch.as_tensor(s["c"])[None])
    with torch.no_grad():
        uv = cam(torch.as_tensor(s["v"])[None])[0].numpy()
    # the module's float32 einsum and the kernel are both within `bound` of the float64 pixels
    assert np.abs(uv.astype(np.float64) - p64[:, :2]).max() <= bound
    assert np.abs(uv.astype(np.float64) - s["dev"]["screen"][0, :, :2]).max() <= 2 * bound


@pytest.mark.parametrize("name", ["icosphere", "two spheres", "body"])
def test_coverage_visibility_depth(name):
    s = scene(name)
    assert s["dev"]["dropped"].tolist() == [0] and s["ras"]["dropped"] == 0
    check_against_oracle(name, s["dev"], s["ras"])
    if name == "icosphere":                                             # closed manifold: every silhouette pixel hit exactly twice
        assert set(np.unique(s["ras"]["hits"]).tolist()) == {0, 2}
    if name == "two spheres":                                           # both spheres are seen
        seen = np.unique(s["dev"]["tri"][0])
        assert (seen[seen >= 0] < 320).any() and (seen >= 320).any()


def _back_project(xy, z, focal, c, t):
    """The world point (R = I) that lands on pixel position xy at camera depth z."""
    return np.array([(xy[0] - c[0]) / focal[0] * z, (xy[1] - c[1]) / focal[1] * z, z], np.float64) - t


def test_edge_cases_in_one_mesh():
    ico_v, ico_f = RC.icosphere(2)
    t, focal, c = np.array([0.0, 0.0, 3.0]), np.array([40.0, 40.0]), np.array([WS / 2.0, HS / 2.0])
    bp = lambda xy, z: _back_project(xy, z, focal, c, t)
    extra = [
        [bp((-4000.0, -3000.0), 6.0), bp((5000.0, -2500.0), 6.0), bp((100.0, 6000.0), 6.0)],      # 0 far larger than the image
        [bp((300.0, 10.0), 2.0), bp((340.0, 12.0), 2.0), bp((310.0, 50.0), 2.0)],                  # 1 wholly off-screen
        [bp((5.0, 5.0), 2.0), bp((9.0, 9.0), 2.0), bp((9.0, 9.0), 2.0)],                            # 2 zero area (two corners coincide)
        [bp((3.6, 3.55), 2.0), bp((4.4, 3.6), 2.0), bp((4.0, 4.45), 2.0)],                          # 3 between pixel centres
        [bp((10.0, 10.0), 2.0), bp((30.0, 10.0), 2.0), bp((20.0, 30.0), 0.01)],                     # 4 a corner behind znear
        [bp((40.0, 10.0), 2.0), bp((60.0, 10.0), 2.0), np.array([np.nan, 0.0, 0.0])],               # 5 a NaN corner
    ]
    v = np.concatenate([ico_v * 0.9] + [np.stack(e) for e in extra]).astype(np.float32)
    f = np.concatenate([ico_f, 162 + np.arange(18).reshape(6, 3)])
    big, off, flat, between = 320, 321, 322, 323
    args = (t[None].astype(np.float32), focal[None].astype(np.float32), c[None].astype(np.float32), HS, WS)
    full = render(v[None], f, *args)
    part = render(v[None], f[:-2], *args)
    assert full["dropped"].tolist() == [2] and part["dropped"].tolist() == [0]
    for k in ("rgba", "depth", "tri"):
        assert np.array_equal(full[k], part[k]), k
    ras = RC.rasterize(full["screen"][0], f, HS, WS)
    assert ras["dropped"] == 2
    # the oracle sees the cases as they are named
    sx, sy, ok = RC.snap(full["screen"][0])
    box = RC.pixel_box([int(a) for a in sx[f[big]]], [int(a) for a in sy[f[big]]], HS, WS)
    assert box == (0, 0, WS - 1, HS - 1)                               # 3 975 pixels: beyond one lane's 256, the wavefront's path
    assert ok[f[:-2]].all() and not ok[f[-2]].all() and not ok[f[-1]].all()
    for idx in (off, flat, between):
        assert not RC.coverage_mask([int(a) for a in sx[f[idx]]], [int(a) for a in sy[f[idx]]], HS, WS).any(), idx
    check_against_oracle("edge cases", full, ras)
    tri = full["tri"][0]
    assert (tri >= 0).all()                                             # the large triangle lies behind the whole image
    assert (tri == big).sum() > 2000 and (tri < 320).sum() > 300
    assert not np.isin(tri, [off, flat, between, 324, 325]).any()
    assert np.array_equal(full["rgba"][0][..., 3], np.full((HS, WS), 255, np.uint8))


@pytest.mark.parametrize("name", ["icosphere", "two spheres"])
def test_colour_and_compositing(name):
    s = scene(name)
    v, f, t, focal, c, R = (s[k] for k in ("v", "f", "t", "focal", "c", "R"))
    ras, dev = s["ras"], s["dev"]
    _, _, ok = RC.snap(dev["screen"][0])
    want = RC.shade(ras, RC.camera_points(v.astype(np.float64), t, R), f, ok)
    agree = (ras["tri"] >= 0) & (dev["tri"][0] == ras["tri"])
    rgba = dev["rgba"][0]
    diff = np.abs(rgba[..., :3].astype(np.int32) - want.astype(np.int32))[agree]
    print("%s: %d shaded pixels, %d a level off, levels %d..%d" % (name, agree.sum(), (diff.max(1) == 1).sum(), want[agree].min(), want[agree].max()))
    assert diff.max() <= 1
    assert want[agree].max() - want[agree].min() > 40                   # the shading is not flat
    covered = dev["tri"][0] >= 0
    assert set(np.unique(rgba[..., 3]).tolist()) == {0, 255} and np.array_equal(rgba[..., 3] == 255, covered)
    assert not rgba[~covered].any()                                     # background=None: black, alpha 0
    bg = np.random.RandomState(4).randint(0, 256, size=(1, s["H"], s["W"], 3)).astype(np.uint8)
    over = render(v[None], f, t[None], focal[None], c[None], s["H"], s["W"], R=None if R is None else R[None], bg=bg, want=("rgba",))["rgba"][0]
    assert np.array_equal(over[~covered][:, :3], bg[0][~covered]) and not over[~covered][:, 3].any()
    assert np.array_equal(over[covered], rgba[covered])
    # another base colour and one light: the colour follows
    red = render(v[None], f, t[None], focal[None], c[None], s["H"], s["W"], R=None if R is None else R[None], want=("rgba",),
                 base_rgb=(1.0, 0.0, 0.5), lights=(((0.0, 0.0, -1.0), 2.0),))["rgba"][0]
    want_red = RC.shade(ras, RC.camera_points(v.astype(np.float64), t, R), f, ok, base_rgb=(1.0, 0.0, 0.5), lights=(((0.0, 0.0, -1.0), 2.0),))
    assert np.abs(red[..., :3].astype(np.int32) - want_red.astype(np.int32))[agree].max() <= 1 and not red[..., 1].any()
    # no light at all: the mesh is black but still there
    dark = render(v[None], f, t[None], focal[None], c[None], s["H"], s["W"], R=None if R is None else R[None], want=("rgba",), lights=())["rgba"][0]
    assert not dark[..., :3].any() and np.array_equal(dark[..., 3] == 255, covered)


def test_batch_independence():
    a, b = scene("icosphere"), scene("two spheres")
    Hh, Ww = a["H"], a["W"]
    V = 162
    others = [b["v"][:V] * 1.3, b["v"][V:] + np.float32(0.2)]
    verts = np.stack([others[0], a["v"], others[1]])
    t = np.stack([b["t"], a["t"], np.array([0.5, 0.4, 2.5], np.float32)])
    focal = np.stack([b["focal"], a["focal"], np.array([80.0, 75.0], np.float32)])
    c = np.stack([b["c"], a["c"], np.array([30.0, 20.0], np.float32)])
    R = np.stack([np.eye(3, dtype=np.float32), a["R"], _rot([1, 0, 0], 1.0).astype(np.float32)])
    bg = np.random.RandomState(8).randint(0, 256, size=(3, Hh, Ww, 3)).astype(np.uint8)
    alone = render(a["v"][None], a["f"], a["t"][None], a["focal"][None], a["c"][None], Hh, Ww, R=a["R"][None], bg=bg[1:2])
    assert np.array_equal(alone["tri"], a["dev"]["tri"]) and np.array_equal(alone["depth"], a["dev"]["depth"])
    for max_pixels in (1 << 26, 2 * Hh * Ww, Hh * Ww, 1):              # one launch; chunks of 2 + 1; of 1; of 1 (never fewer)
        batch = render(verts, a["f"], t, focal, c, Hh, Ww, R=R, bg=bg, max_pixels=max_pixels)
        for k in ALL:
            assert np.array_equal(batch[k][1], alone[k][0]), (max_pixels, k)
        if max_pixels == 1 << 26:
            whole = batch
        else:
            for k in ALL:
                assert np.array_equal(batch[k], whole[k]), (max_pixels, k)
    assert (whole["tri"][0] >= 0).sum() > 300 and (whole["tri"][2] >= 0).sum() > 300


def test_refusals_and_empty_batch():
    import ctypes as C
    from smplifyx_amd import _capi, engine
    s = scene("icosphere")
    Hh, Ww = s["H"], s["W"]
    g = dict(vertices=_gpu(s["v"][None]), translation=_gpu(s["t"][None]), focal=_gpu(s["focal"][None]), center=_gpu(s["c"][None]))
    call = lambda **kw: engine.render_meshes(**dict(dict(g, faces=s["f"], H=Hh, W=Ww), **kw))
    assert call()["rgba"].shape == (1, Hh, Ww, 4)
    for key in ("vertices", "translation", "focal", "center"):
        with pytest.raises(ValueError, match="CUDA"):
            call(**{key: g[key].cpu()})
    with pytest.raises(TypeError):
        call(vertices=s["v"][None])
    bad = [dict(vertices=g["vertices"][0]), dict(vertices=g["vertices"].double()), dict(translation=g["translation"][:, :2]),
           dict(center=g["center"].double()), dict(focal=_gpu(np.ones((1, 3)))), dict(rotation=_gpu(np.eye(3))),
           dict(rotation=torch.eye(3)[None]), dict(background=_gpu(np.zeros((1, Hh, Ww, 3)))),
           dict(background=_gpu(np.zeros((1, Hh, Ww + 1, 3)), torch.uint8)), dict(faces=s["f"][:, :2]), dict(faces=s["f"] + 1),
           dict(faces=torch.as_tensor(s["f"]).float()), dict(want=("rgba", "normals")), dict(want=()), dict(H=0), dict(znear=0.0),
           dict(lights=RC.LIGHTS * 2 + RC.LIGHTS[:1]), dict(base_rgb=(1.0, 1.0))]
    for kw in bad:
        with pytest.raises(ValueError):
            call(**kw)
    assert len(RC.LIGHTS * 2) == engine.RENDER_MAX_LIGHTS
    assert call(lights=RC.LIGHTS * 2)["rgba"].shape == (1, Hh, Ww, 4)
    # the library itself: nine lights are refused before anything is launched or read, B = 0 returns before any pointer is read
    lib = _capi.load()
    cfg = engine.render_cfg()
    null = [None] * 17
    assert lib.sfx_render_meshes(C.byref(cfg), 0, 162, 320, Hh, Ww, *null, None) == 0
    assert lib.sfx_render_meshes(C.byref(cfg), 1, 162, 320, Hh, Ww, *null, None) == -1
    assert "NULL" in lib.sfx_last_error().decode()
    cfg.n_lights = 9
    assert lib.sfx_render_meshes(C.byref(cfg), 1, 162, 320, Hh, Ww, *null, None) == -1
    assert "9 lights" in lib.sfx_last_error().decode()
    cfg = engine.render_cfg()
    for dims in ((1, 0, 320, Hh, Ww), (1, 162, 0, Hh, Ww), (1, 162, 320, 65536, 32768), (3, 162, 320, 32768, 32768)):
        assert lib.sfx_render_meshes(C.byref(cfg), *dims, *null, None) == -1, dims
    empty = call(vertices=g["vertices"][:0], translation=g["translation"][:0], focal=g["focal"][:0], center=g["center"][:0], want=ALL)
    assert empty["rgba"].shape == (0, Hh, Ww, 4) and empty["depth"].shape == (0, Hh, Ww) and empty["tri"].shape == (0, Hh, Ww)
    assert empty["screen"].shape == (0, 162, 3) and empty["dropped"].shape == (0,)
    assert all(v.is_cuda for v in empty.values())


class _Mesh(object):
    def __init__(self, vertices, faces):
        self.vertices, self.faces = vertices, faces


def test_render_mesh_keeps_the_reference_conventions():
    from smplifyx_amd import utils
    s = scene("two spheres")                                            # (R = I, as the reference's camera)
    bg = np.random.RandomState(2).randint(0, 256, size=(s["H"], s["W"], 3)).astype(np.uint8)
    rotated = s["v"].astype(np.float64) * np.array([1.0, -1.0, -1.0])   # by pi about x (utils.py:454-456)
    transl = s["t"].astype(np.float64).copy()
    transl[0] *= -1.0                                                   # utils.py:460
    assert s["focal"][0] == s["focal"][1]
    got = utils.render_mesh(bg.astype(np.float32) / 255.0, _Mesh(rotated, s["f"]), s["c"], transl, float(s["focal"][0]), s["W"], s["H"])
    want = render(s["v"][None], s["f"], s["t"][None], s["focal"][None], s["c"][None], s["H"], s["W"], bg=bg[None], want=("rgba",))["rgba"][0]
    assert got.dtype == np.uint8 and got.shape == (s["H"], s["W"], 3)
    assert np.array_equal(got, want[..., :3])
    assert (want[..., 3] == 255).sum() > 300 and np.array_equal(got[want[..., 3] == 0], bg[want[..., 3] == 0])


def _setup(synth_model, cfg):
    from smplifyx_amd import smplx, utils
    from smplifyx_amd.camera import create_camera
    jm = utils.JointMapper(H.joint_map_for(cfg))
    model_params = dict(model_path=synth_model, joint_mapper=jm, create_global_orient=True, create_body_pose=True,
                        create_betas=True, create_left_hand_pose=True, create_right_hand_pose=True, create_expression=True,
                        create_jaw_pose=True, create_leye_pose=True, create_reye_pose=True, create_transl=False, dtype=torch.float32)
    args = {k: v for k, v in cfg.items() if k not in model_params and k != "gender"}
    bm = smplx.create(gender="neutral", **model_params, **args).to("cuda")
    cam = create_camera(focal_length_x=500.0, focal_length_y=500.0, dtype=torch.float32, **cfg).to("cuda")
    return bm, cam


def test_optimization_visualization_writes_the_overlay(synth_model, tmp_path):
    from PIL import Image
    from smplifyx_amd import engine, utils
    cfg = H.load_cfg("fit_smplx_combined_coco25.yaml", use_hands=False, use_face=False)
    cfg["use_vposer"] = False
    bm, cam = _setup(synth_model, cfg)
    Hh, Ww = 120, 160
    with torch.no_grad():
        cam.translation[:] = torch.tensor([[0.05, 0.3, 9.0]])
        cam.center[:] = torch.tensor([[Ww / 2.0, Hh / 2.0]])
    pose = torch.zeros([1, 63], device="cuda")
    pose[0, 47] = -0.8
    img = np.random.RandomState(6).randint(0, 256, size=(Hh, Ww, 3)).astype(np.uint8)
    out = str(tmp_path / "overlay.png")
    utils.optimization_visualization(img.astype(np.float32) / 255.0, "", pose, bm, cam, 500.0, Ww, Hh, out, None, True, str(tmp_path / "mesh.obj"))
    png = np.asarray(Image.open(out))
    assert png.shape == (Hh, Ww, 3) and png.dtype == np.uint8
    verts = bm(return_verts=True, body_pose=pose).vertices.detach()
    ref = engine.render_meshes(verts.contiguous(), bm.faces, cam.translation.detach(), 500.0, cam.center, Hh, Ww,
                               background=_gpu(img[None], torch.uint8), want=("rgba", "tri"))
    rgba, tri = ref["rgba"][0].cpu().numpy(), ref["tri"][0].cpu().numpy()
    n_cov = int((tri >= 0).sum())
    assert n_cov > 300
    assert np.array_equal(png, rgba[..., :3])
    # the mesh colour is a shade of (0.4, 0.4, 0.7): never a pixel of the random image
    assert int((png != img).any(2).sum()) >= n_cov - 3 and np.array_equal(png[tri < 0], img[tri < 0])
    utils.optimization_visualization(img, "", pose, bm, cam, 500.0, Ww, Hh, None, None, True, "")       # no path: nothing to do


def test_fit_single_frame_writes_out_img_fn(synth_model, tmp_path):
    from PIL import Image
    from scipy.spatial.transform import Rotation as Rot
    from smplifyx_amd import prior
    from smplifyx_amd.fit_single_frame import fit_single_frame
    g = np.load(os.path.join(GOLD, "e2e_synth.npz"))
    cfg = H.load_cfg("fit_smplx_combined_coco25.yaml", use_hands=False, use_face=False)
    cfg.update(use_camera_prior=False, regression_prior="ExPose", use_vposer=False)
    bm, camera = _setup(synth_model, cfg)
    Hh, Ww, scale = 150, 200, 0.25                                      # the golden keypoints are for 800 x 600 at focal 5000
    kp = g["keypoints"][1:2].copy()
    kp[:, :, :2] *= scale
    expose = {"body_pose": Rot.from_euler("XYZ", g["reg_pose"][1].reshape(21, 3).astype(np.float64)).as_matrix().astype(np.float32),
              "global_orient": Rot.from_euler("XYZ", g["reg_global"][1].astype(np.float64)[None]).as_matrix().astype(np.float32)}
    a = dict(cfg, focal_length=5000.0 * scale)
    for k in ("result_folder", "output_folder", "mesh_folder", "render_overlays"):
        a.pop(k, None)
    mk = lambda t: prior.create_prior(prior_type=t, dtype=torch.float32)
    img = np.random.RandomState(12).randint(0, 256, size=(Hh, Ww, 3)).astype(np.uint8)
    jw = torch.tensor(H.base_joint_weights(cfg, 25)).unsqueeze(0)
    common = dict(body_model=bm, camera=camera, joint_weights=jw, dtype=torch.float32, shape_prior=mk("l2"), expr_prior=None,
                  body_pose_prior=mk("l2"), left_hand_prior=None, right_hand_prior=None, jaw_prior=None, angle_prior=mk("angle"),
                  expose_results=expose, result_folder=str(tmp_path))
    png = str(tmp_path / "output.png")
    fit_single_frame(img.astype(np.float32) / 255.0, kp, result_fn=str(tmp_path / "a.pkl"), out_img_fn=png, **common, **a)
    assert not os.path.exists(png)                                      # not asked for: nothing is drawn
    fit_single_frame(img.astype(np.float32) / 255.0, kp, result_fn=str(tmp_path / "b.pkl"), out_img_fn=png, render_overlays=True,
                     **common, **a)
    im = np.asarray(Image.open(png))
    assert im.shape == (Hh, Ww, 3)
    changed = (im != img).any(2)
    assert 300 < changed.sum() < Hh * Ww // 2, changed.sum()
    assert not os.path.exists(str(tmp_path / "vertices.ply"))


def test_main_writes_overlays_only_when_asked(synth_model, tmp_path):
    import json
    import warnings
    from PIL import Image
    from scipy.spatial.transform import Rotation as Rot
    from smplifyx_amd import main as amd_main
    g = np.load(os.path.join(GOLD, "e2e_synth.npz"))
    data, models, expose_dir = tmp_path / "data", tmp_path / "models" / "smplx", tmp_path / "expose"
    for d in (data / "images", data / "keypoints", models, expose_dir):
        os.makedirs(d)
    np.savez(models / "SMPLX_NEUTRAL.npz", **synth_model)
    names = ["frame_a", "frame_b"]
    Hh, Ww = 150, 200
    scale = Ww / 800.0                                                  # the golden keypoints are for 800 x 600 at focal 5000
    imgs = np.random.RandomState(9).randint(0, 256, size=(2, Hh, Ww, 3)).astype(np.uint8)
    for i, n in enumerate(names):
        Image.fromarray(imgs[i]).save(data / "images" / (n + ".png"))
        kp = g["keypoints"][i].copy()
        kp[:, :2] *= scale
        json.dump({"people": [{"pose_keypoints_2d": [float(v) for v in kp.reshape(-1)],
                               "hand_left_keypoints_2d": [], "hand_right_keypoints_2d": [], "face_keypoints_2d": []}]},
                  open(data / "keypoints" / (n + "_keypoints.json"), "w"))
        os.makedirs(expose_dir / (n + ".jpg"))
        np.savez(expose_dir / (n + ".jpg") / (n + ".jpg_params.npz"),
                 body_pose=Rot.from_euler("XYZ", g["reg_pose"][i].reshape(21, 3).astype(np.float64)).as_matrix().astype(np.float32),
                 global_orient=Rot.from_euler("XYZ", g["reg_global"][i].astype(np.float64)[None]).as_matrix().astype(np.float32))
    cfg = H.load_cfg("fit_smplx_combined_coco25.yaml", use_hands=False, use_face=False)
    cfg.update(use_camera_prior=False, use_face_contour=False, regression_prior="ExPose", data_folder=str(data),
               model_folder=str(tmp_path / "models"), expose_results_directory=str(expose_dir), pixie_results_directory=None,
               focal_length=5000.0 * scale, visualize=True)
    assert cfg["render_overlays"] is False
    for asked in (True, False):
        out = tmp_path / ("out_%d" % asked)
        with warnings.catch_warnings(record=True) as wlist:
            warnings.simplefilter("always")
            n = amd_main.main(**dict(cfg, output_folder=str(out), render_overlays=asked))
        assert n == 2
        assert "visualize / interactive: rendering and progress output are outside the fitting path" in " ".join(str(w.message) for w in wlist)
        for i, nme in enumerate(names):
            assert os.path.isfile(out / "results" / nme / "000.pkl") and os.path.isdir(out / "images" / nme / "000")
            png = out / "images" / nme / "000" / "output.png"
            assert not os.path.exists(out / "results" / nme / "vertices.ply")        # (save_vertices is off)
            if not asked:
                assert not os.path.exists(png)
                continue
            im = np.asarray(Image.open(png))
            assert im.shape == (Hh, Ww, 3)
            changed = (im != imgs[i]).any(2)
            assert 300 < changed.sum() < Hh * Ww // 2, changed.sum()    # a body over the image, the rest untouched
            res = pickle.load(open(out / "results" / nme / "000.pkl", "rb"))
            assert res["H"] == Hh and res["W"] == Ww
