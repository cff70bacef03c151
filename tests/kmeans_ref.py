"""A numpy restatement of R's kmeans(x, centers=<matrix>, algorithm="Lloyd"), the definition batchelor_amd.kmeans is held to.

Labels start as "none".  Every iteration assigns each observation to its nearest centre by the direct distance
sum((x - c)^2), ties to argmin's first index (R's strict `<` scan); if no label changed the run has converged; otherwise
every centre becomes the mean of its members and `iter` counts the assignments; after iter_max of them the loop ends
behind the update with converged = False.  Either way the centres are the means of the returned labels.
"""
from dataclasses import dataclass

import numpy as np


@dataclass
class RefResult:
    cluster: np.ndarray      # 1-based int32
    centers: np.ndarray      # K x d
    withinss: np.ndarray
    tot_withinss: float
    size: np.ndarray
    iter: int
    converged: bool
    margin: float            # smallest tie margin met: min over iterations and observations of (second - best) / (second + |x|^2)


def direct_distances(x, centers, block=512):
    """D[i, j] = sum_k (x[i, k] - centers[j, k])^2, taken directly in FP64."""
    out = np.empty((x.shape[0], centers.shape[0]))
    for a in range(0, x.shape[0], block):
        diff = x[a:a + block, None, :] - centers[None, :, :]
        out[a:a + block] = np.einsum("ijk,ijk->ij", diff, diff)
    return out


def kmeans_ref(x, centers, iter_max=10):
    x = np.ascontiguousarray(x, dtype=np.float64)
    centers = np.array(centers, dtype=np.float64)
    n, K = x.shape[0], centers.shape[0]
    if centers.ndim != 2 or centers.shape[1] != x.shape[1]:
        raise ValueError("must have same number of columns in 'x' and 'centers'")
    if K < 1 or K > n:
        raise ValueError("more cluster centers than observations")
    if np.unique(centers, axis=0).shape[0] != K:
        raise ValueError("initial centers are not distinct")
    x2 = np.einsum("ik,ik->i", x, x)
    labels = np.full(n, -1, dtype=np.int64)
    margin = np.inf
    it, converged = 0, False
    while it < iter_max:
        it += 1
        D = direct_distances(x, centers)
        new = np.argmin(D, axis=1)
        if K > 1:
            two = np.partition(D, 1, axis=1)[:, :2]
            denom = two[:, 1] + x2
            ok = denom > 0
            if ok.any():
                margin = min(margin, float(((two[:, 1] - two[:, 0])[ok] / denom[ok]).min()))
            if (~ok).any():
                margin = 0.0
        if np.array_equal(new, labels):
            converged = True
            break
        labels = new
        size = np.bincount(labels, minlength=K)
        if (size == 0).any():
            raise ValueError("empty cluster: try a better set of initial centers")
        for j in range(K):
            centers[j] = x[labels == j].mean(axis=0)
    size = np.bincount(labels, minlength=K)
    diff = x - centers[labels]
    per = np.einsum("ik,ik->i", diff, diff)
    withinss = np.bincount(labels, weights=per, minlength=K)
    return RefResult(cluster=(labels + 1).astype(np.int32), centers=centers, withinss=withinss,
                     tot_withinss=float(withinss.sum()), size=size.astype(np.int32), iter=it, converged=converged,
                     margin=margin)
