"""fastMNN() front-end for a list of batches (R/fastMNN.R:283-358, `.fast_mnn_list`): cosine normalisation,
multiBatchPCA and the projection on the GPU (`pca="host"` keeps multiBatchPCA on the host, as BASELINE.json's north_star
allows), then the MI355X merge engine.  Batches are genes x cells, as in the reference."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .inputs import all_sparse, check_same_dim, check_same_rows, divide_into_batches, reindex_pairings, unpack_batches
from .multi_batch_pca import _multi_batch_pca_host, _split_rows, cosineNorm, densify, multiBatchPCA, project
from .reduced_mnn import MnnResult, fast_mnn_core


@dataclass
class FastMnnResult:
    """What convertPCsToSCE (R/convertPCsToSCE.R:50-72) is built from: corrected PCs, batch, rotation, merge.info."""
    corrected: np.ndarray
    batch: np.ndarray
    rotation: np.ndarray
    centers: np.ndarray
    merge_info: object
    stats: object = None
    var_explained: np.ndarray = None   # get_variance: d^2 / nbatches and the total (R/multiBatchPCA.R:422-432)
    var_total: float = None

    def reconstructed(self, rows=None, cells=None):
        """The `reconstructed` low-rank assay of convertPCsToSCE (R/convertPCsToSCE.R:60-66), LowRankMatrix(rotation,
        corrected) = rotation %*% t(corrected), realised in numpy for the genes `rows` and the cells `cells` only
        (anything numpy indexes an axis with, 0-based; None: all).  With correct_all the rows are those of the input."""
        rot = self.rotation if rows is None else self.rotation[rows]
        pcs = self.corrected if cells is None else self.corrected[cells]
        return np.atleast_2d(rot) @ np.atleast_2d(pcs).T


def _pca_step(mats, d, weights, cos_norm, device, pca, pca_tol, pca_maxit, subset_row, correct_all, get_variance):
    """cosineNorm + multiBatchPCA + projection (R/fastMNN.R:348-354): (pca record, list of cells x d matrices)."""
    if pca not in ("device", "host"):
        raise ValueError("'pca' should be one of 'device', 'host'")
    if pca == "device":
        rec = multiBatchPCA(*mats, d=d, weights=weights, cos_norm=cos_norm, tol=pca_tol, max_iters=pca_maxit, device=device,
                            subset_row=subset_row, get_all_genes=correct_all, get_variance=get_variance)
        return rec, rec["pcs"]
    if all_sparse(mats, "fastMNN"):   # the host PCA and the projection behind it take dense batches
        mats = densify(mats, "fastMNN")
    l2 = [cosineNorm(m, mode="l2norm", subset_row=subset_row) for m in mats] if cos_norm else None  # R/fastMNN.R:348-351
    rec, rot, cen = _multi_batch_pca_host(mats, d, weights, l2, 65536, subset_row, correct_all, get_variance)  # :353-354
    sub = _split_rows(subset_row, mats[0].shape[0])[0]
    return rec, [project(m if sub is None else m[sub], rot, cen, cos_norm=cos_norm) for m in mats]


def fastMNN(*batches, batch=None, k=20, prop_k=None, restrict=None, cos_norm=True, ndist=3, d=50, weights=None,
            merge_order=None, auto_merge=False, min_batch_skip=0.0, names=None, device=0, pca="device",
            pca_tol=1e-9, pca_maxit=500, subset_row=None, correct_all=False, get_variance=False) -> FastMnnResult:
    """fastMNN(..., batch=, k=, prop.k=, restrict=, cos.norm=, ndist=, d=, weights=, merge.order=, auto.merge=,
    min.batch.skip=, subset.row=, correct.all=, get.variance=) (R/fastMNN.R:283-331): several batches (`.fast_mnn_list`,
    :339-358) or ONE genes x cells object with `batch=` naming each cell's batch (`.fast_mnn_single`, :364-388).

    subset_row (1-based integers or a logical mask): the genes the cosine norms and the PCA are taken over -- the run is
    the run on x[subset_row].  correct_all: the result's rotation and centers cover every gene of the input (the others'
    rotation rows come from multiBatchPCA's get.all.genes), so `reconstructed()` does.  get_variance: `var_explained` and
    `var_total` of the PCA.  Batches that are all scipy.sparse objects (several, or one with `batch=`, whose columns are
    split sparse) stay sparse through the PCA (multiBatchPCA's sparse path); everything after it is unchanged.
    Not taken: d=NA, preserve.single, a character subset.row (there are no row names), deferred, BSPARAM."""
    batches = unpack_batches(batches)
    sparse = all_sparse(batches, "fastMNN")
    if len(batches) == 1:
        x = batches[0].tocsc() if sparse else np.asarray(batches[0], dtype=np.float64)
        return _fast_mnn_single(x, batch, k, prop_k, restrict, cos_norm, ndist, d,
                                weights, merge_order, auto_merge, min_batch_skip, device, pca, pca_tol, pca_maxit,
                                subset_row, correct_all, get_variance)
    if len(batches) < 2:
        raise ValueError("at least two batches must be specified")  # R/fastMNN.R:345
    if sparse:
        mats = list(batches)
        check_same_rows(mats)
    else:
        mats = [np.asarray(b, dtype=np.float64) for b in batches]
        check_same_dim(mats, byrow=False)
    rec, pcs = _pca_step(mats, d, weights, cos_norm, device, pca, pca_tol, pca_maxit, subset_row, correct_all, get_variance)
    out: MnnResult = fast_mnn_core(pcs, k, prop_k, restrict, ndist, merge_order, auto_merge, min_batch_skip, names, device)
    return FastMnnResult(corrected=out.corrected, batch=out.batch, rotation=rec["rotation"], centers=rec["centers"],
                         merge_info=out.merge_info, stats=out.stats, var_explained=rec.get("var_explained"),
                         var_total=rec.get("var_total"))


def _fast_mnn_single(x, batch, k, prop_k, restrict, cos_norm, ndist, d, weights, merge_order, auto_merge,
                     min_batch_skip, device, pca, pca_tol, pca_maxit, subset_row=None, correct_all=False,
                     get_variance=False):
    """.fast_mnn_single (R/fastMNN.R:364-388): the batches are the levels of factor(batch) in sorted order; the PCA sees
    them as separate batches (`.multi_pca_single`, R/multiBatchPCA.R:241-258), the merge engine too
    (divideIntoBatches), and rows and pairs come back in the caller's cell order."""
    if batch is None:
        raise ValueError("'batch' must be specified if '...' has only one object")  # R/checkInputs.R:128
    batch = np.asarray(batch)
    if x.ndim != 2 or batch.shape[0] != x.shape[1]:
        raise ValueError("'length(batch)' and 'ncol(x)' are not the same")  # R/checkInputs.R:131
    levels = sorted(set(batch.tolist()))
    if len(levels) < 2:
        raise ValueError("at least two batches must be specified")
    mats = [x[:, batch == lev] for lev in levels]
    rec, pcs = _pca_step(mats, d, weights, cos_norm, device, pca, pca_tol, pca_maxit, subset_row, correct_all, get_variance)
    # divideIntoBatches(mat, batch, restrict, byrow=TRUE) on the PCs (R/fastMNN.R:379): restrict is ONE subsetting vector
    # over the cells of x (1-based positions or a logical mask)
    r = restrict[0] if isinstance(restrict, (list, tuple)) and len(restrict) == 1 else restrict
    allpcs = np.empty((x.shape[1], pcs[0].shape[1]))
    for lev, pc in zip(levels, pcs):
        allpcs[batch == lev] = pc
    div = divide_into_batches(allpcs, batch, r, byrow=True)
    out = fast_mnn_core(div.parts, k, prop_k, div.restricted, ndist, merge_order, auto_merge, min_batch_skip,
                    [str(lev) for lev in div.levels], device)
    reo = div.reorder                                            # R/fastMNN.R:383-385
    out.merge_info.pairs = reindex_pairings(out.merge_info.pairs, reo)
    return FastMnnResult(corrected=out.corrected[reo - 1], batch=out.batch[reo - 1], rotation=rec["rotation"],
                         centers=rec["centers"], merge_info=out.merge_info, stats=out.stats,
                         var_explained=rec.get("var_explained"), var_total=rec.get("var_total"))
