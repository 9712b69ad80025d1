"""Shared by tests/test_gpu_objective.py and tests/test_objective_host.py: the per-component form of the mixture prior as an
oracle (oracle/prior_gmm.py restates the merged form only) and the mixture of tests/golden/gmm.npz."""
import os

import numpy as np
import torch

from oracle.prior_gmm import MaxMixtureRef

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class _PerComponentRef(MaxMixtureRef):
    """MaxMixturePrior(use_merged=False) (prior.py:203-225) on the tables of oracle.prior_gmm.MaxMixtureRef, one value per row:
    m* = argmin_m [d^T P_m d + 0.5 (log(det cov_m + eps) + D log 2 pi)], value(m*) - log nll_weights_m*."""

    def __init__(self, means, covars, weights, dtype=torch.float32, epsilon=1e-16):
        super().__init__(means, covars, weights, dtype)
        np_dtype = np.float32 if dtype == torch.float32 else np.float64
        covs = np.asarray(covars).astype(np_dtype)
        D = covs.shape[-1]
        self.const = torch.tensor(0.5 * (np.log(np.linalg.det(covs) + epsilon) + D * np.log(np.asarray(2 * np.pi, np_dtype))), dtype=dtype)

    def __call__(self, pose, betas=None):
        diff = pose.unsqueeze(1) - self.means
        ll = (torch.einsum("mij,bmj->bmi", self.precisions, diff) * diff).sum(-1) + self.const
        best = torch.argmin(ll, dim=1)
        return ll.gather(1, best[:, None])[:, 0] - torch.log(self.nll_weights[0, best])


def _gmm():
    g = np.load(os.path.join(GOLD, "gmm.npz"))
    return dict(means=g["means"], covars=g["covars"], weights=g["weights"]), g["poses"]
