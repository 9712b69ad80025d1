"""CPU tests of the device evaluation's surface (sfx_eval_align / sfx_eval_nearest, engine.align_errors, engine.nearest_distances,
evaluation.compute_v2v(device=True)): the declarations and their bindings, what is refused before any launch, and that the
default host path of compute_v2v returns what it returned before the keywords existed.  No GPU needed."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from smplifyx_amd import _capi, engine, evaluation as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "evaluation.npz"))
ENTRY_POINTS = ("sfx_eval_align", "sfx_eval_nearest")


def _t(*shape):
    return torch.zeros(*shape, dtype=torch.float32)


def test_header_declares_both_entries_with_the_reference_lines_they_replace():
    hdr = open(os.path.join(ROOT, "include", "sfx.h")).read()
    for name in ENTRY_POINTS:
        assert len(re.findall(r"\bint\s+%s\s*\(" % name, hdr)) == 1, name
        assert name in _capi.SYMBOLS, name
    align_doc = hdr[:hdr.index("int  sfx_eval_align")].rsplit("/*", 1)[-1]
    for lines in ("utils.py:540-595", ":597-614", ":650-668", ":729-772"):
        assert lines in align_doc, lines
    nearest_doc = hdr[hdr.index("int  sfx_eval_align"):hdr.index("int  sfx_eval_nearest")]
    assert "utils.py:622-648" in nearest_doc
    for mode, value in engine.ALIGN_MODES.items():
        assert re.search(r"SFX_ALIGN_%s = %d\b" % (mode.upper(), value), hdr), mode
    assert re.search(r"#define SFX_ALIGN_MAX_ANCHORS %d\b" % engine.ALIGN_MAX_ANCHORS, hdr)
    assert re.search(r"#define SFX_NEAREST_MAX_THRESH %d\b" % engine.NEAREST_MAX_THRESH, hdr)


def test_units_list_names_evaluate_once_and_the_solve_has_a_header_of_its_own():
    csrc = os.path.join(ROOT, "smplify-x-partial_amd", "csrc")
    units = [l.split()[0] for l in open(os.path.join(csrc, "units.txt")) if l.strip() and not l.startswith("#")]
    assert units.count("evaluate") == 1
    assert os.path.exists(os.path.join(csrc, "evaluate.hip"))
    solve = open(os.path.join(csrc, "procrustes3.h")).read()
    assert "hip_runtime" not in solve and not re.search(r"\bhip[A-Z]\w+\(", solve)      # no HIP runtime call in it


def test_bindings_take_the_arguments_the_header_declares():
    assert len(_capi.SYMBOLS["sfx_eval_align"][1]) == 12
    assert len(_capi.SYMBOLS["sfx_eval_nearest"][1]) == 15
    lib = _capi.load()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name)


def test_align_errors_refuses_before_any_launch():
    est, gt = _t(2, 14, 3), _t(2, 14, 3)
    with pytest.raises(ValueError, match="no CPU fallback"):
        engine.align_errors(est, gt)
    with pytest.raises(TypeError, match="torch tensor"):
        engine.align_errors(np.zeros((2, 14, 3), np.float32), gt)
    with pytest.raises(TypeError, match="torch tensor"):
        engine.align_errors(est, np.zeros((2, 14, 3), np.float32))
    with pytest.raises(ValueError, match=r"gt: shape \(2, 15, 3\)"):
        engine.align_errors(est, _t(2, 15, 3))
    with pytest.raises(ValueError, match=r"est: shape \(2, 14\)"):
        engine.align_errors(_t(2, 14), gt)
    with pytest.raises(ValueError, match=r"mask: shape \(2, 13\)"):
        engine.align_errors(est, gt, mask=torch.ones(2, 13, dtype=torch.bool))
    with pytest.raises(ValueError, match="torch.bool or torch.uint8"):
        engine.align_errors(est, gt, mask=torch.ones(2, 14))
    with pytest.raises(ValueError, match="mode"):
        engine.align_errors(est, gt, mode="rigid")
    with pytest.raises(ValueError, match=r"anchors: \[2, 14\] outside the 14 points"):
        engine.align_errors(est, gt, mode="pelvis", anchors=(2, 14))
    with pytest.raises(ValueError, match="anchors"):
        engine.align_errors(est, gt, mode="pelvis", anchors=(-1,))
    with pytest.raises(ValueError, match="anchors: 9 given"):
        engine.align_errors(est, gt, mode="pelvis", anchors=range(9))
    with pytest.raises(ValueError, match="anchors: 0 given"):
        engine.align_errors(est, gt, mode="pelvis", anchors=())


def test_nearest_distances_refuses_before_any_launch():
    a, b = _t(2, 5, 3), _t(2, 7, 3)
    with pytest.raises(ValueError, match="no CPU fallback"):
        engine.nearest_distances(a, b, [0.1])
    with pytest.raises(TypeError, match="torch tensor"):
        engine.nearest_distances(a.numpy(), b)
    with pytest.raises(ValueError, match=r"b: shape \(3, 7, 3\)"):
        engine.nearest_distances(a, _t(3, 7, 3))
    with pytest.raises(ValueError, match=r"a: shape \(2, 5, 2\)"):
        engine.nearest_distances(_t(2, 5, 2), b)
    with pytest.raises(ValueError, match="thresholds: 9 given"):
        engine.nearest_distances(a, b, np.linspace(0.1, 0.9, 9))
    with pytest.raises(ValueError, match=r"mask_b: shape \(2, 5\)"):
        engine.nearest_distances(a, b, mask_a=torch.ones(2, 5, dtype=torch.bool), mask_b=torch.ones(2, 5, dtype=torch.bool))


def test_compute_v2v_device_refuses_before_any_launch():
    al = {"procrustes": E.ProcrustesAlignmentMPJPE(), "pelvis": E.PelvisAlignmentMPJPE()}
    with pytest.raises(ValueError, match="no CPU fallback"):
        E.compute_v2v(_t(2, 14, 3), _t(2, 14, 3), al, device=True)
    with pytest.raises(TypeError, match="vertices_fitted: a torch tensor"):
        E.compute_v2v(np.zeros((2, 14, 3)), _t(2, 14, 3), al, device=True)
    with pytest.raises(TypeError, match="vertices_target: a torch tensor"):
        E.compute_v2v(_t(2, 14, 3), np.zeros((2, 14, 3)), al, device=True)
    with pytest.raises(ValueError, match=r"shape \(2, 14\)"):
        E.compute_v2v(_t(2, 14), _t(2, 14, 3), al, device=True)
    with pytest.raises(ValueError, match="masks"):
        E.compute_v2v(np.zeros((2, 14, 3)), np.zeros((2, 14, 3)), al, masks=np.ones((2, 14), bool))


def test_compute_v2v_device_refuses_other_alignments_by_exact_type():
    class Mine(E.ProcrustesAlignmentMPJPE):
        def __call__(self, est, gt):
            return {"point": np.zeros(len(est)), "fscore": {}}

    x = _t(2, 14, 3)
    with pytest.raises(TypeError, match=r"alignments\['mine'\].*Mine"):
        E.compute_v2v(x, x, {"ok": E.PelvisAlignmentMPJPE(), "mine": Mine()}, device=True)
    with pytest.raises(TypeError, match=r"alignments\['scale'\].*ScaleAlignment"):
        E.compute_v2v(x, x, {"scale": E.ScaleAlignment()}, device=True)
    with pytest.raises(TypeError, match="PelvisAlignment"):
        E.compute_v2v(x, x, {"p": E.PelvisAlignment()}, device=True)
    # the host path goes on taking any callable
    out = E.compute_v2v(G["j_est"][None], G["j_gt"][None], {"mine": Mine()})
    assert out["point"]["mine"].shape == (1, 14)


def test_compute_v2v_defaults_are_the_host_path_bit_for_bit():
    sig = inspect.signature(E.compute_v2v)
    assert list(sig.parameters) == ["vertices_fitted", "vertices_target", "alignments", "vids", "masks", "device"]
    assert sig.parameters["masks"].default is None and sig.parameters["device"].default is False
    est, gt = np.stack([G["v_est"], G["v_est"][::-1]]), np.stack([G["v_gt"], G["v_gt"][::-1]])
    vids = np.arange(0, 400, 2)
    al = {"procrustes": E.ProcrustesAlignmentMPJPE(fscore_thresholds=[0.05, 0.2]), "pelvis": E.PelvisAlignmentMPJPE([0.3])}
    for kw in ({}, dict(masks=None, device=False)):
        out = E.compute_v2v(est, gt, al, vids=vids, **kw)
        assert set(out) == {"point", "fscore"} and set(out["point"]) == set(al) == set(out["fscore"])
        for name, align in al.items():
            direct = [align(est[b][vids], gt[b][vids]) for b in range(2)]
            assert out["point"][name].dtype == np.float64
            assert np.array_equal(out["point"][name], np.stack([d["point"] for d in direct]))
            assert set(out["fscore"][name]) == set(align.fscore_thresholds)
            for t in align.fscore_thresholds:
                assert np.array_equal(out["fscore"][name][t], np.stack([np.asarray(d["fscore"][t]["fscore"]) for d in direct]))
    # and the reference's own numbers for the whole set
    whole = E.compute_v2v(G["v_est"][None], G["v_gt"][None], {"p": E.ProcrustesAlignmentMPJPE()})
    assert np.allclose(whole["point"]["p"][0], G["v_procrustes_mpjpe"], rtol=1e-9, atol=1e-12)


def test_module_docstring_names_the_device_path():
    assert "nothing here runs on the device" not in E.__doc__.lower()
    assert "device=True" in E.__doc__ and "evaluate.hip" in E.__doc__
