"""CPU restatement of clusterMNN() (R/clusterMNN.R:101-312) in numpy, built on oracle.fastmnn_oracle.reduced_mnn.
A helper module of the clusterMNN tests (not a conftest); it imports nothing from the package under test.
Batches are genes x cells, indices 1-based, None = NULL.  Cluster levels: the sorted unique labels of a batch (the order of
sumCountsAcrossCells).  Squared distances are added over the columns in ascending order, one double at a time, as
queryKNN's and colSums' loops do: that fixes every bit of the distances the bandwidth is the median of."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any

import numpy as np

from oracle import fastmnn_oracle as orc


def cosine_l2(x, subset_row=None):
    """cosineNorm(x, mode="l2norm", subset.row=) (R/cosineNorm.R:63-82)."""
    y = x if subset_row is None else x[np.asarray(subset_row, dtype=np.int64) - 1]
    return np.sqrt((y * y).sum(axis=0))


def compute_centroids(x, clusters, restrict=None):
    """.compute_centroids for one batch (R/clusterMNN.R:231-244): genes x levels, and the levels."""
    clusters = np.asarray(clusters)
    levels = np.unique(clusters)
    if restrict is not None:
        r = np.asarray(restrict, dtype=np.int64) - 1
        x, clusters = x[:, r], clusters[r]
    return np.stack([x[:, clusters == lv].mean(axis=1) for lv in levels], axis=1), levels


def full_rank_pca(centroids, subset_row=None, correct_all=False):
    """.full_rank_pca (R/clusterMNN.R:171-181) = multiBatchPCA(ExactParam(), d = sum(ncol) - 1, get.all.genes=correct.all)
    (R/multiBatchPCA.R:211-322, .make_pca_metadata :401-414).  Returns (rotation, centers, pcs, rotation_used,
    centers_used)."""
    G = centroids[0].shape[0]
    sub = None if subset_row is None else np.asarray(subset_row, dtype=np.int64) - 1
    cs = centroids if sub is None else [c[sub] for c in centroids]
    grand = sum(c.mean(axis=1) for c in cs) / len(cs)
    scaled = np.concatenate([(c - grand[:, None]) / np.sqrt(c.shape[1]) for c in cs], axis=1)
    d = min(sum(c.shape[1] for c in cs) - 1, scaled.shape[0])
    u, s, vt = np.linalg.svd(scaled, full_matrices=False)
    u = u[:, :d]
    pcs = [(c - grand[:, None]).T @ u for c in cs]
    rotation, centers = u, grand
    if correct_all and sub is not None:
        left = np.setdiff1d(np.arange(G), sub)
        ls = [c[left] for c in centroids]
        lgrand = sum(c.mean(axis=1) for c in ls) / len(ls)
        lscaled = np.concatenate([(c - lgrand[:, None]) / np.sqrt(c.shape[1]) for c in ls], axis=1)
        rotation = np.zeros((G, d))
        rotation[sub] = u
        rotation[left] = (lscaled @ vt[:d].T) / s[:d]
        centers = np.zeros(G)
        centers[sub] = grand
        centers[left] = lgrand
    return rotation, centers, pcs, u, grand


def squared_distances(x, centers):
    """[cells x centroids]: sum over the columns, ascending, of (x[i, t] - centers[j, t])^2."""
    d2 = np.zeros((x.shape[0], centers.shape[0]))
    for t in range(x.shape[1]):
        df = x[:, t, None] - centers[None, :, t]
        d2 += df * df
    return d2


def nearest_distance(x, centers):
    """queryKNN(query=x, X=centers, k=1, get.index=FALSE)$distance[,1]."""
    return np.sqrt(squared_distances(x, centers).min(axis=1))


def smooth_gaussian_from_centroids(x, centers, sigma, delta):
    """.smooth_gaussian_from_centroids (R/clusterMNN.R:286-312)."""
    weights = -squared_distances(x, centers) / sigma ** 2
    norm = np.exp(weights - weights.max(axis=1, keepdims=True))
    norm = norm / norm.sum(axis=1, keepdims=True)
    out = x.copy()
    for j in range(centers.shape[0]):
        out += np.outer(norm[:, j], delta[j])
    return out


def propagate_to_cells(x, rotation_used, centers_used, centroids_pc, corrected_pc, restrict=None, subset_row=None,
                       l2=None):
    """One batch of .propagate_to_cells (R/clusterMNN.R:262-282): (smoothed cells x d, sigma, cur)."""
    y = x if subset_row is None else x[np.asarray(subset_row, dtype=np.int64) - 1]
    if l2 is not None:
        y = y / np.maximum(l2, 1e-8)
    cur = y.T @ rotation_used - centers_used @ rotation_used
    dist = nearest_distance(cur, centroids_pc)
    if restrict is not None:
        dist = dist[np.asarray(restrict, dtype=np.int64) - 1]
    sigma = float(np.median(dist))
    return smooth_gaussian_from_centroids(cur, centroids_pc, sigma, corrected_pc - centroids_pc), sigma, cur


def meta_clusters(pairs, nrows):
    """components(make_graph(rbind(left, right), n=nrows, directed=FALSE))$membership: numbered from 1 in order of each
    component's lowest row."""
    label = np.arange(nrows)
    changed = True
    edges = [(int(a) - 1, int(b) - 1) for left, right in pairs for a, b in zip(left, right)]
    while changed:  # label propagation to the component's lowest row
        changed = False
        for a, b in edges:
            m = min(label[a], label[b])
            if label[a] != m or label[b] != m:
                label[a] = label[b] = m
                changed = True
    out = np.zeros(nrows, dtype=np.int64)
    seen = {}
    for i in range(nrows):
        out[i] = seen.setdefault(int(label[i]), len(seen) + 1)
    return out


@dataclass
class ClusterMnnRef:
    corrected: np.ndarray
    batch: np.ndarray
    cluster: np.ndarray
    rotation: np.ndarray
    centers: np.ndarray
    merge_info: Any
    sigma: np.ndarray
    cluster_info: dict
    merged: Any  # the centroid-level reduced_mnn result


def _cluster_mnn_list(batches, restrict, clusters, cos_norm, merge_order, auto_merge, min_batch_skip, subset_row,
                      correct_all, names):
    if not isinstance(clusters, (list, tuple)):
        raise ValueError("'clusters' must be either a list or a BlusterParam object")
    if len(clusters) != len(batches):
        raise ValueError("'...' and 'clusters' should be of the same length")
    for b, c in zip(batches, clusters):
        if b.shape[1] != len(c):
            raise ValueError("corresponding entries of '...' and 'clusters' should have the same number of cells")
    restrict = [None] * len(batches) if restrict is None else list(restrict)
    l2 = [cosine_l2(b, subset_row) if cos_norm else None for b in batches]                      # :139-142
    normed = [b if s is None else b / np.maximum(s, 1e-8) for b, s in zip(batches, l2)]
    cents, levels = zip(*[compute_centroids(b, c, r) for b, c, r in zip(normed, clusters, restrict)])  # :143
    rotation, centers, pcs, u, grand = full_rank_pca(list(cents), subset_row, correct_all)      # :145
    merged = orc.reduced_mnn(*pcs, k=1, merge_order=merge_order, auto_merge=auto_merge,
                             min_batch_skip=min_batch_skip, names=names)                       # :147
    if names is not None:  # R/fastMNN.R:419-427: batch ids become the batches' names
        merged.batch = np.asarray(list(names), dtype=object)[np.asarray(merged.batch) - 1]
        merged.merge_info.left = [[names[i - 1] for i in s] for s in merged.merge_info.left]
        merged.merge_info.right = [[names[i - 1] for i in s] for s in merged.merge_info.right]
    parts, sigma, batch, last = [], [], [], 0
    for b, (x, p) in enumerate(zip(batches, pcs)):                                              # :149-152
        after = merged.corrected[last:last + p.shape[0]]
        out, s, _ = propagate_to_cells(x, u, grand, p, after, restrict[b], subset_row, l2[b])
        parts.append(out)
        sigma.append(s)
        batch.append(np.repeat(merged.batch[last:last + 1], x.shape[1]))
        last += p.shape[0]
    info = {"cluster": np.concatenate(levels), "batch": merged.batch, "meta": meta_clusters(merged.merge_info.pairs, last)}
    return ClusterMnnRef(corrected=np.concatenate(parts), batch=np.concatenate(batch),
                         cluster=np.concatenate([np.asarray(c) for c in clusters]), rotation=rotation, centers=centers,
                         merge_info=merged.merge_info, sigma=np.asarray(sigma), cluster_info=info, merged=merged)


def cluster_mnn(*batches, batch=None, restrict=None, clusters, cos_norm=True, merge_order=None, auto_merge=False,
                min_batch_skip=0.0, subset_row=None, correct_all=False):
    """clusterMNN() (R/clusterMNN.R:101-169) for a list of clusters."""
    batches = [np.asarray(b, dtype=np.float64) for b in batches]
    if len(batches) > 1:
        return _cluster_mnn_list(batches, restrict, clusters, cos_norm, merge_order, auto_merge, min_batch_skip,
                                 subset_row, correct_all, None)
    x = batches[0]
    batch = np.asarray(batch)
    if isinstance(clusters, (list, tuple)):
        if len(clusters) != 1:
            raise ValueError("'clusters' must be a list of length 1 when '...' contains one element")
    else:
        raise ValueError("'clusters' must be either a list or a BlusterParam object")
    call = np.asarray(clusters[0])
    levels = sorted(set(batch.tolist()))
    mask = None
    if restrict is not None and restrict[0] is not None:
        mask = np.zeros(x.shape[1], dtype=bool)
        mask[np.asarray(restrict[0], dtype=np.int64) - 1] = True
    parts, cparts, rparts = [], [], (None if mask is None else [])
    reorder = np.zeros(x.shape[1], dtype=np.int64)
    last = 0
    for lv in levels:  # divideIntoBatches(byrow=FALSE) and split(clusters[[1]], batch) (:121-132)
        keep = batch == lv
        parts.append(x[:, keep])
        cparts.append(call[keep])
        if mask is not None:
            rparts.append(np.flatnonzero(mask[keep]) + 1)
        reorder[keep] = last + np.arange(1, int(keep.sum()) + 1)
        last += int(keep.sum())
    out = _cluster_mnn_list(parts, rparts, cparts, cos_norm, merge_order, auto_merge, min_batch_skip, subset_row,
                            correct_all, [str(lv) for lv in levels])
    out.corrected = out.corrected[reorder - 1]
    out.batch = out.batch[reorder - 1]
    out.cluster = out.cluster[reorder - 1]
    return out
