"""helpers.dense_weights_model on the CPU: the model the GPU tests of tests/test_gpu_dense_weights.py stand on is what its
docstring says, and the oracle is as good a reference on it as on the base model."""
import numpy as np
import torch

import helpers as H


def test_dense_weights_model_is_what_the_gpu_tests_assume(synth_model):
    d = H.dense_weights_model(synth_model)              # (asserts its own preconditions)
    assert H.dense_weights_model(synth_model) is d and set(d) == set(synth_model)
    for k in synth_model:
        if k != "weights":
            assert d[k] is synth_model[k], k
    W0, W = np.asarray(synth_model["weights"]), np.asarray(d["weights"])
    assert W.dtype == W0.dtype and W.shape == W0.shape == (10475, 55)
    V = W.shape[0]
    nz = (W != 0).sum(1)
    cls = np.repeat(H.dense_tile_classes(V), H.DENSE_TILE)[:V]
    kv = np.isin(np.arange(V), H.keypoint_vertices(synth_model))
    assert len(H.dense_tile_classes(V)) == 655 and kv.sum() >= 300
    for c, n in H.DENSE_CLASS_COUNT.items():
        m = (cls == c) & ~kv
        assert m.sum() > 1000 and np.all(nz[m] == n), (c, n)
    own = np.isin(cls, (0, 5)) & ~kv
    assert np.array_equal(W[own], W0[own]) and nz[own].max() <= 3
    assert np.all(nz[kv] == H.DENSE_KEYPOINT_COUNT) and np.all(cls[V - 11:] == 4)
    # the weights the model had keep their joints and 90 % of their value
    assert np.all(W[W0 != 0] > 0) and np.abs(W[~own][W0[~own] != 0] / W0[~own][W0[~own] != 0] - 0.9).max() < 1e-6


def test_the_oracle_is_as_exact_on_dense_weights(synth_model):
    """The float32 oracle against the independent float64 numpy forward at one far pose: 5e-7 m on the base model and on the
    dense-weights model alike -- a tenth of the 5e-6 m the device is held to."""
    from oracle import lbs_numpy
    cfg = H.load_cfg("fit_smplx_combined_halpe.yaml")
    P = H.random_params(np.random.RandomState(8), 1)
    q = {("body_pose" if k == "pose_embedding" else k): v[0] for k, v in P.items()}
    for model in (synth_model, H.dense_weights_model(synth_model)):
        bm = H.oracle_model(model, cfg, torch.float32)
        bm.reset_params(**{k: v for k, v in P.items() if k != "pose_embedding"})
        with torch.no_grad():
            o = bm(return_verts=True, body_pose=torch.tensor(P["pose_embedding"]))
        ref = lbs_numpy.forward(model, q, joint_map=H.joint_map_for(cfg))
        assert np.abs(o.vertices[0].numpy() - ref["vertices"]).max() < 5e-7
        assert np.abs(o.joints[0].numpy() - ref["joints"]).max() < 5e-7
