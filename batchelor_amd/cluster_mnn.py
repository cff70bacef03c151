"""clusterMNN() (R/clusterMNN.R:101-169): MNN correction of cluster centroids, propagated to every cell.

The MNN search runs on a few hundred centroids (`reducedMNN(k=1)` on their full-rank PCs); the per-cell work is two
streaming passes over each genes x cells matrix -- the centroid means and the projection -- plus a Gaussian smoothing of
the centroids' correction vectors, all on the device behind the bmx_cluster_* entry points (csrc/cluster_mnn.hip).  The
batches are uploaded once and stay in HBM between the two passes.  The full-rank PCA of the centroids (`.full_rank_pca`,
:171-181) runs on the host: its input is genes x (number of clusters).

With `clusters=KmeansParam(...)` every batch is clustered here first (.format_clusters, :199-221): the `subset_row` rows
of the raw batch, its own PCA to `cluster_d` components (the single-batch DevicePCA, or a host SVD where the blocked
iteration cannot take the shape), then kmeans() on the device (csrc/kmeans.hip).  The labels then go the way labels
given by the caller go.  A batch is uploaded once for that PCA and once more for bmx_cluster_*.

The batches are all dense or all scipy.sparse (any format, matrix or array: what multiBatchNorm returns for sparse counts
goes straight in).  Sparse ones are made canonical CSC on the host and stay CSC in HBM (bmx_cluster_sparse_*): both
streaming passes walk the stored entries only, and everything after them -- the centroids' PCA, the merge, the nearest
centroid, the median, the smoothing -- is the dense call's, so the result is the dense call's: dense cells x d.  Under
`clusters=KmeansParam(...)` a sparse batch's PCs come from a one-batch DeviceSparsePCA over its `subset_row` rows; where
that handle cannot take the shape, and with cluster_d=None (kmeans takes dense observations), those rows are made dense
on the host, which is refused above multi_batch_pca.DENSIFY_CAP_BYTES.

Out of scope (a clear error): bluster methods other than k-means (NNGraphParam and the rest), more than 257 clusters in
total (the merge engine takes at most 256 columns), SingleCellExperiment inputs, a mixture of sparse and dense batches.
"""
from __future__ import annotations

import ctypes
import warnings
from dataclasses import dataclass
from typing import Any, List, Optional

import numpy as np
import scipy.sparse as sp

from . import _lib
from ._handle import ResidentHandle
from .inputs import (all_sparse, canonical_csc, check_restrict_length, check_same_dim, check_same_rows, csc_block_width,
                     divide_into_batches, restrict_list, subset_index, unpack_batches)
from .kmeans import MAX_CENTERS, KmeansParam, kmeans
from .multi_batch_pca import DevicePCA, DeviceSparsePCA, _csc_rows, densify, device_pca_takes
from .reduced_mnn import reducedMNN

MAX_DIMS = 256          # columns the merge engine takes (csrc/engine.hip)
BLOCK_BYTES = 1 << 28   # a batch above this size goes to the device in column blocks of about this many bytes
SPARSE_BLOCK_CELLS = None  # cells per uploaded block of a CSC batch; None: about BLOCK_BYTES of stored entries


@dataclass
class ClusterMnnResult:
    """What clusterMNN() returns: the corrected low-rank coordinates of every cell and the metadata of R/clusterMNN.R:153-164."""
    corrected: np.ndarray      # cells x d, cells in the caller's order
    batch: np.ndarray          # batch id (1-based) or name per cell
    cluster: np.ndarray        # each cell's cluster label
    rotation: np.ndarray       # genes x d (all genes with correct_all, else the subset's)
    centers: np.ndarray        # genes
    merge_info: Any            # of the centroid-level reducedMNN; pairs index the rows of cluster_info
    sigma: np.ndarray          # per batch: the bandwidth of the smoothing
    cluster_info: dict         # columns "cluster", "batch", "meta", one row per centroid
    # "stage_ms": upload, centroids, projection, nearest_median, smoothing; "merge": per merge sizes; "clustering": None for
    # labels given by the caller, else per batch what clustered it (path of the PCA, d, K, iter, converged, stage_ms);
    # "pca" of a sparse batch: "device-sparse-pca", or "densified: " + the dense path its subset rows then took
    stats: Optional[dict] = None


def _format_clusters(ncells, clusters):
    """.format_clusters (R/clusterMNN.R:185-227), the list branch."""
    if not isinstance(clusters, (list, tuple)):
        raise ValueError("'clusters' must be either a list or a BlusterParam object")
    if len(clusters) != len(ncells):
        raise ValueError("'...' and 'clusters' should be of the same length")
    out = []
    for n, c in zip(ncells, clusters):
        c = np.asarray(c)
        if c.ndim != 1 or c.shape[0] != n:
            raise ValueError("corresponding entries of '...' and 'clusters' should have the same number of cells")
        out.append(c)
    return out


def _check_clustering(param, ncells, cluster_d):
    """The argument errors of clusters=KmeansParam that need no device; returns every batch's number of centres."""
    if cluster_d is not None and (isinstance(cluster_d, (bool, np.bool_)) or not isinstance(cluster_d, (int, np.integer))
                                  or cluster_d < 1):
        raise ValueError("'cluster_d' must be a positive integer or None")
    for name in ("iter_max", "nstart"):
        v = getattr(param, name)
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"'{name}' of a KmeansParam must be a positive integer")
    ks = []
    for b, n in enumerate(ncells):
        k = param.n_centers(n)
        if k < 1 or k > min(n, MAX_CENTERS):
            raise ValueError(f"batch {b + 1} of {n} cells cannot be split into {k} clusters: kmeans takes 1 <= centers <= "
                             f"min(cells, {MAX_CENTERS})")
        ks.append(k)
    return ks


def _batch_pcs(m, d, device):
    """runPCA(t(m), rank=d) of one batch (genes x cells), centred and not scaled: cells x d and the path taken."""
    if device_pca_takes(m.shape[0], m.shape[1], d):
        pca = DevicePCA(m.shape[0], device)
        try:
            pca.add_batch(m, weight=1.0, cos_norm=False)
            pca.fit(d=d)
            return pca.project(0), "device-pca"
        finally:
            pca.close()
    centred = m.T - m.mean(axis=1)
    u, s, _ = np.linalg.svd(centred, full_matrices=False)
    return u[:, :d] * s[:d], "host-svd"


def _sparse_batch_pcs(c, d, device):
    """_batch_pcs for canonical CSC: a one-batch DeviceSparsePCA whose PCA rows are all of c's; where it cannot take the
    shape, c is made dense (refused above DENSIFY_CAP_BYTES) and goes the dense way."""
    if device_pca_takes(c.shape[0], c.shape[1], d):
        pca = DeviceSparsePCA(c.shape[0], None, device)
        try:
            pca.add_batch(c, weight=1.0, cos_norm=False)
            pca.fit(d=d)
            return pca.project(0), "device-sparse-pca"
        finally:
            pca.close()
    obs, path = _batch_pcs(densify([c], "clusterMNN")[0], d, device)
    return obs, "densified: " + path


def _cluster_batches(mats, sub, param, ks, cluster_d, device):
    """.format_clusters, the BlusterParam branch (R/clusterMNN.R:204-220): every batch's labels from kmeans() on its own
    PCs (or on its rows with cluster_d=None), the restriction ignored as in the reference."""
    labels, info = [], []
    for m, k in zip(mats, ks):
        sparse = sp.issparse(m)
        if sparse:
            cur = _csc_rows(m, None if sub is None else sub.astype(np.int64) - 1)
        else:
            cur = np.asarray(m, dtype=np.float64)
            if sub is not None:
                cur = cur[sub - 1]
        d, path = cluster_d, "none"
        if d is not None:
            if d > min(cur.shape):
                warnings.warn(f"'cluster_d' = {d} exceeds min(genes, cells) = {min(cur.shape)} of a batch: clamped",
                              stacklevel=4)
                d = int(min(cur.shape))
            obs, path = (_sparse_batch_pcs if sparse else _batch_pcs)(cur, int(d), device)
        elif sparse:
            obs, path = np.ascontiguousarray(densify([cur], "clusterMNN")[0].T), "densified: none"
        else:
            obs = np.ascontiguousarray(cur.T)
        res = kmeans(obs, k, iter_max=param.iter_max, nstart=param.nstart, seed=param.seed, device=device)
        labels.append(res.cluster)
        info.append({"pca": path, "d": d, "centers": k, "iter": res.iter, "converged": res.converged,
                     "tot_withinss": res.tot_withinss, "start": res.stats["start"], "stage_ms": res.stats["stage_ms"]})
    return labels, info


def _levels(labels, restrict, which):
    """Sorted unique labels of a batch (the order of sumCountsAcrossCells), each cell's 0-based level; every level needs a
    restricted cell."""
    levels, ids = np.unique(labels, return_inverse=True)
    ids = ids.astype(np.int32)
    kept = ids if restrict is None else ids[restrict - 1]
    present = np.zeros(levels.size, dtype=bool)
    present[kept] = True
    if not present.all():
        raise ValueError(f"cluster '{levels[np.flatnonzero(~present)[0]]}' of batch {which} has no cells remaining after "
                         "restriction")
    return levels, ids


def _concat_labels(arrs):
    if len({a.dtype.kind for a in arrs}) == 1:
        return np.concatenate(arrs)
    return np.concatenate([a.astype(object) for a in arrs])


def full_rank_pca(centroids, subset_row=None, correct_all=False):
    """.full_rank_pca (R/clusterMNN.R:171-181): multiBatchPCA(ExactParam, d = sum(ncol) - 1) of the centroid matrices
    (genes x clusters each, all genes).  Centre: the grand mean of the batch means; every batch scaled by 1/sqrt(C_b); an
    exact SVD.  Returns the rotation / centres over the genes used (`rotation_used`, `centers_used`: what the projection
    takes), over the genes reported (`rotation`, `centers`: all genes with correct_all, R/multiBatchPCA.R:401-414), and the
    centroids' coordinates `pcs` (C_b x d each)."""
    G = centroids[0].shape[0]
    sub = None if subset_row is None else np.asarray(subset_row, dtype=np.int64) - 1

    def scale(rows):
        cs = [c if rows is None else c[rows] for c in centroids]
        grand = sum(c.mean(axis=1) for c in cs) / len(cs)
        return cs, grand, np.concatenate([(c - grand[:, None]) / np.sqrt(c.shape[1]) for c in cs], axis=1)

    cs, grand, scaled = scale(sub)
    d = min(sum(c.shape[1] for c in cs) - 1, scaled.shape[0])
    u, s, vt = np.linalg.svd(scaled, full_matrices=False)
    u = np.ascontiguousarray(u[:, :d])
    pcs = [(c - grand[:, None]).T @ u for c in cs]
    rotation, centers = u, grand
    if correct_all and sub is not None:
        left = np.setdiff1d(np.arange(G), sub)
        _, lgrand, lscaled = scale(left)
        rotation = np.zeros((G, d))
        rotation[sub] = u
        rotation[left] = (lscaled @ vt[:d].T) / s[:d]
        centers = np.zeros(G)
        centers[sub] = grand
        centers[left] = lgrand
    return {"rotation_used": u, "centers_used": grand, "rotation": rotation, "centers": centers, "pcs": pcs, "d": d}


def meta_clusters(pairs, nrows):
    """components(make_graph(rbind(left, right), n))$membership (R/clusterMNN.R:162-164): connected components of the
    graph of all MNN pairs over the centroid rows, numbered from 1 by each component's lowest row."""
    parent = np.arange(nrows)

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for left, right in pairs:
        for a, b in zip(np.asarray(left).tolist(), np.asarray(right).tolist()):
            ra, rb = find(a - 1), find(b - 1)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    roots = np.array([find(i) for i in range(nrows)])
    _, first, inverse = np.unique(roots, return_index=True, return_inverse=True)
    rank = np.empty(first.size, dtype=np.int64)
    rank[np.argsort(first)] = np.arange(1, first.size + 1)
    return rank[inverse]


class _ClusterHandle(ResidentHandle):
    """bmx_cluster_t: the batches stay in HBM between centroids() and propagate()."""
    PREFIX = "bmx_cluster"
    STAGES = ("upload", "centroids", "projection", "nearest_median", "smoothing")

    def __init__(self, n_genes, subset, device):
        self.rows = int(n_genes) if subset is None else int(subset.size)
        self.nclusters = []
        super().__init__(n_genes, device, None if subset is None else _lib.i32p(subset),
                         ctypes.c_int32(0 if subset is None else int(subset.size)))

    def add_batch(self, x, ids, n_clusters, restrict, cos_norm, block_bytes=BLOCK_BYTES):
        """x: genes x cells, `ids` each cell's 0-based cluster; see ResidentHandle._upload for block_bytes."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        self._upload(x, block_bytes, _lib.i32p(ids), ctypes.c_int32(int(n_clusters)),
                     None if restrict is None else _lib.i32p(restrict),
                     ctypes.c_int64(-1 if restrict is None else int(restrict.size)), ctypes.c_int32(int(bool(cos_norm))))
        self.nclusters.append(int(n_clusters))

    def centroids(self, b):
        out = np.empty((self.G, self.nclusters[b]), dtype=np.float64, order="F")
        self._call("centroids", ctypes.c_int32(b), _lib.f64p(out))
        return out

    def propagate(self, b, rotation, centers, centroid_pcs, corrected_pcs):
        rotation = _lib.as_f(rotation)
        centers = np.ascontiguousarray(centers, dtype=np.float64)
        cp, cc = _lib.as_f(centroid_pcs), _lib.as_f(corrected_pcs)
        d = int(rotation.shape[1])
        if rotation.shape[0] != self.rows or centers.shape != (self.rows,):
            raise ValueError("'rotation' and 'centers' must cover the genes in use")
        if cp.shape != (self.nclusters[b], d) or cc.shape != cp.shape:
            raise ValueError("the centroids' coordinates must be (number of clusters) x d")
        out = np.empty((self.ncells[b], d), dtype=np.float64, order="F")
        sigma = ctypes.c_double(0.0)
        self._call("propagate", ctypes.c_int32(b), _lib.f64p(rotation), ctypes.c_int32(d), _lib.f64p(centers), _lib.f64p(cp),
                   _lib.f64p(cc), _lib.f64p(out), ctypes.byref(sigma))
        return out, float(sigma.value)


class _ClusterSparseHandle(_ClusterHandle):
    """bmx_cluster_sparse_t: the same over canonical CSC batches (inputs.canonical_csc), kept CSC in HBM."""
    PREFIX = "bmx_cluster_sparse"

    def add_batch(self, c, ids, n_clusters, restrict, cos_norm, block_cells=None):
        """c: canonical CSC, genes x cells.  block_cells: cells per uploaded block (None: SPARSE_BLOCK_CELLS, and without
        that as many as hold about BLOCK_BYTES of stored entries); the results do not depend on it."""
        if block_cells is None:
            block_cells = SPARSE_BLOCK_CELLS
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        self._upload_csc(c, csc_block_width(c, BLOCK_BYTES) if block_cells is None else max(1, int(block_cells)),
                         _lib.i32p(ids), ctypes.c_int32(int(n_clusters)), None if restrict is None else _lib.i32p(restrict),
                         ctypes.c_int64(-1 if restrict is None else int(restrict.size)), ctypes.c_int32(int(bool(cos_norm))),
                         nnz_first=True)
        self.nclusters.append(int(n_clusters))


def _cluster_mnn(mats, restrict, clusters, cos_norm, merge_order, auto_merge, min_batch_skip, subset_row, correct_all,
                 names, device, cluster_d=50):
    """The body of clusterMNN() from .format_clusters on (R/clusterMNN.R:134-164), for a list of batches: all numpy
    arrays, or all scipy.sparse."""
    if len(mats) < 2:
        raise ValueError("at least two batches must be specified")
    sparse = sp.issparse(mats[0])
    G = check_same_rows(mats) if sparse else check_same_dim(mats, byrow=False)
    ncells = [m.shape[1] for m in mats]
    check_restrict_length(restrict, len(mats))
    ks = None
    if isinstance(clusters, KmeansParam):
        ks = _check_clustering(clusters, ncells, cluster_d)
        if sum(ks) - 1 > MAX_DIMS:   # (refused below for any labels: here before a batch is clustered)
            raise ValueError(f"clusterMNN works in sum(number of clusters) - 1 = {sum(ks) - 1} dimensions; the merge engine "
                             f"takes at most {MAX_DIMS}")
    else:
        clusters = _format_clusters(ncells, clusters)
    restrict = restrict_list(restrict, ncells) or [None] * len(mats)
    sub = subset_index(subset_row, G)
    if sub is not None and sub.size == 0:
        raise ValueError("'subset_row' selects no genes")
    clustering = None
    if ks is not None:
        _lib.require_gpu()
        clusters, clustering = _cluster_batches(mats, sub, clusters, ks, cluster_d, device)
    lev = [_levels(c, r, b + 1) for b, (c, r) in enumerate(zip(clusters, restrict))]
    total = sum(lv.size for lv, _ in lev)
    if total - 1 > MAX_DIMS:
        raise ValueError(f"clusterMNN works in sum(number of clusters) - 1 = {total - 1} dimensions; the merge engine takes "
                         f"at most {MAX_DIMS}")
    _lib.require_gpu()
    if sparse:
        mats = [canonical_csc(m)[0] for m in mats]
    h = (_ClusterSparseHandle if sparse else _ClusterHandle)(G, sub, device)
    try:
        for m, (lv, ids), r in zip(mats, lev, restrict):
            h.add_batch(m, ids, lv.size, r, cos_norm)
        cents = [h.centroids(b) for b in range(len(mats))]                                   # :143
        pca = full_rank_pca(cents, sub, correct_all)                                          # :145
        merged = reducedMNN(*pca["pcs"], k=1, merge_order=merge_order, auto_merge=auto_merge,
                            min_batch_skip=min_batch_skip, names=names, device=device)       # :147
        parts, sigma, last = [], [], 0
        for b, p in enumerate(pca["pcs"]):                                                    # .propagate_to_cells
            after = merged.corrected[last:last + p.shape[0]]
            out, s = h.propagate(b, pca["rotation_used"], pca["centers_used"], p, after)
            parts.append(out)
            sigma.append(s)
            last += p.shape[0]
        stage_ms = h.stage_ms()
    finally:
        h.close()
    ends = np.cumsum([p.shape[0] for p in pca["pcs"]])
    cbatch = merged.batch
    info = {"cluster": _concat_labels([lv for lv, _ in lev]), "batch": cbatch,
            "meta": meta_clusters(merged.merge_info.pairs, int(ends[-1]))}
    batch = np.concatenate([np.repeat(cbatch[e - 1:e], m.shape[1]) for e, m in zip(ends, mats)])
    return ClusterMnnResult(corrected=np.concatenate(parts, axis=0), batch=batch, cluster=_concat_labels(clusters),
                            rotation=pca["rotation"], centers=pca["centers"], merge_info=merged.merge_info,
                            sigma=np.asarray(sigma), cluster_info=info,
                            stats={"stage_ms": stage_ms, "merge": merged.stats, "clustering": clustering})


def clusterMNN(*batches, batch=None, restrict=None, clusters, cluster_d=50, cos_norm=True, merge_order=None,
               auto_merge=False, min_batch_skip=0.0, subset_row=None, correct_all=False, device=0) -> ClusterMnnResult:
    """clusterMNN(..., batch=, restrict=, clusters=, cluster.d=, cos.norm=, merge.order=, auto.merge=, min.batch.skip=,
    subset.row=, correct.all=) (R/clusterMNN.R:101-169).  Each batch is genes x cells; `clusters` is a list with one vector
    of labels (integers or strings) per batch, or of length 1 for a single object that `batch=` splits -- or a KmeansParam:
    every batch (of a single object: every piece `batch=` splits off) is then clustered by kmeans() on the first
    `cluster_d` PCs of its `subset_row` rows (cluster_d=None: on those rows themselves), every batch from the param's
    seed; `restrict` plays no part in that, as in the reference.

    The batches are all dense or all scipy.sparse (implicit zeros are zeros); sparse ones stay CSC on the device and the
    result is the dense call's (the module docstring)."""
    batches = unpack_batches(batches)
    if len(batches) == 0:
        raise ValueError("at least two batches must be specified")
    sparse = all_sparse(batches, "clusterMNN")
    mats: List[Any] = list(batches) if sparse else [np.asarray(b) for b in batches]
    if len(mats) > 1:
        return _cluster_mnn(mats, restrict, clusters, cos_norm, merge_order, auto_merge, min_batch_skip, subset_row,
                            correct_all, None, device, cluster_d)
    # one object: divideIntoBatches(byrow=FALSE) and split(clusters[[1]], batch) (:121-132)
    x = mats[0]
    if batch is None:
        raise ValueError("'batch' must be specified if '...' has only one object")  # R/checkInputs.R:128
    if x.ndim != 2 or np.asarray(batch).shape[0] != x.shape[1]:
        raise ValueError("'length(batch)' and 'ncol(x)' are not the same")
    if restrict is not None and len(restrict) != 1:
        raise ValueError("'restrictions' must of length equal to the number of batches")
    also = ()
    if isinstance(clusters, (list, tuple)):
        if len(clusters) != 1:
            raise ValueError("'clusters' must be a list of length 1 when '...' contains one element")
        call = np.asarray(clusters[0])
        if call.ndim != 1 or call.shape[0] != x.shape[1]:
            raise ValueError("corresponding entries of '...' and 'clusters' should have the same number of cells")
        also = (call,)
    elif not isinstance(clusters, KmeansParam):
        raise ValueError("'clusters' must be either a list or a BlusterParam object")
    if sparse:
        x = canonical_csc(x)[0]  # (a format that takes a column mask)
    div = divide_into_batches(x, batch, None if restrict is None else restrict[0], also=also)
    out = _cluster_mnn(div.parts, div.restricted, div.also[0] if also else clusters, cos_norm, merge_order, auto_merge,
                       min_batch_skip, subset_row, correct_all, [str(lv) for lv in div.levels], device, cluster_d)
    reorder = div.reorder
    out.corrected = out.corrected[reorder - 1]  # output[, divided$reorder] (:166-168)
    out.batch = out.batch[reorder - 1]
    out.cluster = out.cluster[reorder - 1]
    return out
