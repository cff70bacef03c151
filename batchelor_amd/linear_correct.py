"""rescaleBatches() (R/rescaleBatches.R:63-150) and regressBatches() (R/regressBatches.R:93-158): the linear corrections.

Both are per-gene passes over genes x cells FP64 matrices: per-gene statistics over each batch's restricted cells, then one
pass that writes every cell.  The batches are uploaded once (whole or in column blocks), stay in HBM between the two
passes, and the result comes back block by block behind the kernels (csrc/linear_correct.hip, bmx_linear_*).

regressBatches: the reference delegates to ResidualMatrix; the definition used here (man/regressBatches.Rd, the
reference's tests) is, with X genes x cells, D cells x p the design and R the restricted cells,
    coef = argmin || X[:, R] - coef @ D[R, :].T ||,   out = X - coef[:, drop] @ D[:, drop].T,
drop = the columns of D not named in `keep`.  Without a design D has one indicator column per batch, coef is the batch
means and no product is formed.  With a design the host factors D[R, :] (QR) and the device forms both skinny products.

Out of scope (a clear error): sparse and SingleCellExperiment inputs, designs of more than 64 columns, a design whose
restricted rows are not of full column rank (R's pivoted QR would drop columns instead), deferred / BSPARAM.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from . import _lib
from ._handle import ResidentHandle
from .inputs import check_same_dim, check_unique_names, divide_into_batches, restrict_list, subset_index, unpack_batches

MAX_DESIGN_COLUMNS = 64   # BMX_LINEAR_MAX_DESIGN_COLUMNS
BLOCK_BYTES = 1 << 28     # a batch above this size goes to the device in column blocks of about this many bytes
OVERLAP = True            # say what is coming before the upload, so that the per-gene sums run behind it
KEEP_UNLOGGED = False     # rescaleBatches: keep log_base^x - pseudo_count in HBM for the second pass (EXPERIMENTS.md)
RANK_TOL = 1e-7           # relative size of a diagonal entry of the QR's R below which the design is called deficient
STAGES = ("upload", "first_pass", "statistics", "second_pass_kernels", "second_pass_wall")


@dataclass
class LinearCorrectResult:
    """What rescaleBatches() / regressBatches() return."""
    corrected: np.ndarray                      # genes x cells (column-major), cells in the caller's order
    batch: np.ndarray                          # batch id (1-based) or name per cell
    averages: Optional[np.ndarray] = None      # rescaleBatches: genes x batches, mean unlogged value of the restricted cells
    reference: Optional[np.ndarray] = None     # rescaleBatches: genes, the minimum of `averages` over the batches
    coefficients: Optional[np.ndarray] = None  # regressBatches: genes x p (default design: the batch means)
    pcs: Optional[np.ndarray] = None           # regressBatches(d=): cells x d
    stats: Optional[dict] = None               # "stage_ms": see STAGES


def _as_matrices(batches, what):
    mats: List[np.ndarray] = []
    for b in unpack_batches(batches):
        mod = type(b).__module__ or ""
        if mod.startswith("scipy.sparse") or hasattr(b, "tocsr"):
            raise TypeError(f"{what} takes dense matrices: sparse inputs are not supported")
        if hasattr(b, "assays") or hasattr(b, "obsm") or type(b).__name__ == "SingleCellExperiment":
            raise TypeError(f"{what} takes matrices: SingleCellExperiment inputs are not supported")
        m = np.asarray(b)
        if m.dtype == object:
            raise TypeError(f"{what} takes numeric matrices")
        mats.append(m)
    return mats


def _check_names(names, n):
    if names is None:
        return None
    names = [str(v) for v in names]
    if len(names) != n:
        raise ValueError("'names' must have one entry per batch")
    check_unique_names(names)  # R/rescaleBatches.R:140, R/regressBatches.R:117
    return names


def _check_batch(batch, ncells):
    batch = np.asarray(batch)
    if batch.ndim != 1 or batch.shape[0] != ncells:
        raise ValueError("'length(batch)' should be equal to number of cells in '...'")  # R/divideIntoBatches.R:97
    return batch


def _divide(x, batch, restrict):
    """One object split by column: the parts, their restrictions, each divided cell's level, the way back."""
    div = divide_into_batches(x, batch, restrict)
    labels = np.repeat(np.asarray(div.levels), [m.shape[1] for m in div.parts])
    return div.parts, div.restricted or [None] * len(div.parts), labels, div.reorder


def _labels(names, ncells):
    lab = np.arange(1, len(ncells) + 1) if names is None else np.asarray(names)
    return np.repeat(lab, ncells)


class _LinearHandle(ResidentHandle):
    """bmx_linear_t: the batches stay in HBM between the statistics and the pass that writes the result."""
    PREFIX = "bmx_linear"
    STAGES = STAGES

    def expect(self, kind, log_base=2.0, pseudo_count=1.0, keep_unlogged=False):
        _lib.check(_lib.lib().bmx_linear_expect(self._h, ctypes.c_int32(int(kind)), ctypes.c_double(float(log_base)),
                                                ctypes.c_double(float(pseudo_count)),
                                                ctypes.c_int32(int(bool(keep_unlogged)))))

    def add_batch(self, x, restrict, block_bytes=None):
        """x: genes x cells; see ResidentHandle._upload for block_bytes (None: the module's BLOCK_BYTES)."""
        self._upload(x, BLOCK_BYTES if block_bytes is None else block_bytes,
                     None if restrict is None else _lib.i32p(restrict),
                     ctypes.c_int64(-1 if restrict is None else int(restrict.size)))

    def _outs(self):
        out = np.empty((self.G, sum(self.ncells)), dtype=np.float64, order="F")
        ptrs = (ctypes.c_void_p * len(self.ncells))()
        at = 0
        for i, n in enumerate(self.ncells):
            ptrs[i] = out.ctypes.data + at * self.G * 8
            at += n
        return out, ptrs

    def rescale(self, log_base, pseudo_count):
        out, ptrs = self._outs()
        avg = np.empty((self.G, len(self.ncells)), dtype=np.float64, order="F")
        ref = np.empty(self.G, dtype=np.float64)
        _lib.check(_lib.lib().bmx_linear_rescale(self._h, ctypes.c_double(float(log_base)),
                                                 ctypes.c_double(float(pseudo_count)), ptrs, _lib.f64p(avg),
                                                 _lib.f64p(ref)))
        return out, avg, ref

    def regress(self, design=None, w=None, keep=None):
        out, ptrs = self._outs()
        if design is None:
            coef = np.empty((self.G, len(self.ncells)), dtype=np.float64, order="F")
            _lib.check(_lib.lib().bmx_linear_regress(self._h, None, ctypes.c_int32(0), None, None, ctypes.c_int32(0), ptrs,
                                                     _lib.f64p(coef)))
            return out, coef
        design, w = _lib.as_f(design), _lib.as_f(w)
        p = int(design.shape[1])
        keep = np.zeros(0, dtype=np.int32) if keep is None else np.ascontiguousarray(keep, dtype=np.int32)
        coef = np.empty((self.G, p), dtype=np.float64, order="F")
        _lib.check(_lib.lib().bmx_linear_regress(self._h, _lib.f64p(design), ctypes.c_int32(p), _lib.f64p(w),
                                                 _lib.i32p(keep) if keep.size else None, ctypes.c_int32(int(keep.size)),
                                                 ptrs, _lib.f64p(coef)))
        return out, coef

    def fetch(self):
        """The batches as uploaded, straight back (bmx_linear_fetch): the transfer floor of a call."""
        out, ptrs = self._outs()
        _lib.check(_lib.lib().bmx_linear_fetch(self._h, ptrs))
        return out


def _rows(mats, sub):
    return mats if sub is None else [m[sub - 1] for m in mats]


def rescaleBatches(*batches, batch=None, restrict=None, log_base=2, pseudo_count=1, subset_row=None, correct_all=False,
                   names=None, device=0) -> LinearCorrectResult:
    """rescaleBatches(..., batch=, restrict=, log.base=, pseudo.count=, subset.row=, correct.all=)
    (R/rescaleBatches.R:63-150): every batch's unlogged values are scaled down, gene by gene, so that its mean over the
    restricted cells equals the lowest batch mean; the result is logged again.  Each batch is genes x cells of
    log-expression values; one object plus `batch=` is split by column and the result put back in the caller's order.
    `names` plays the role of the argument names of `...`."""
    mats = _as_matrices(batches, "rescaleBatches")
    if len(mats) == 0:
        raise ValueError("at least two batches must be specified")  # R/rescaleBatches.R:107
    G = check_same_dim(mats, byrow=False)
    res = restrict_list(restrict, [m.shape[1] for m in mats]) or [None] * len(mats)
    reorder = None
    if len(mats) == 1:
        if batch is None:
            raise ValueError("'batch' must be specified if '...' has only one object")  # R/divideIntoBatches.R:88
        mats, res, labels, reorder = _divide(mats[0], _check_batch(batch, mats[0].shape[1]), res[0])
    else:
        names = _check_names(names, len(mats))
        labels = _labels(names, [m.shape[1] for m in mats])
    if len(mats) < 2:
        raise ValueError("at least two batches must be specified")
    log_base, pseudo_count = float(log_base), float(pseudo_count)
    if not (np.isfinite(log_base) and log_base > 0 and log_base != 1):
        raise ValueError("'log_base' must be positive, finite and not 1")
    if not np.isfinite(pseudo_count):
        raise ValueError("'pseudo_count' must be finite")
    sub = None if correct_all else subset_index(subset_row, G)  # R/rescaleBatches.R:82-84
    if sub is not None and sub.size == 0:
        raise ValueError("'subset_row' selects no genes")
    mats = _rows(mats, sub)
    _lib.require_gpu()
    h = _LinearHandle(mats[0].shape[0], device)
    try:
        if OVERLAP:
            h.expect(2, log_base, pseudo_count, KEEP_UNLOGGED)
        for m, r in zip(mats, res):
            h.add_batch(m, r)
        out, avg, ref = h.rescale(log_base, pseudo_count)
        stage_ms = h.stage_ms()
    finally:
        h.close()
    if reorder is not None:
        out = np.asfortranarray(out[:, reorder - 1])  # output[, divided$reorder] (R/rescaleBatches.R:89-92)
        labels = labels[reorder - 1]
    return LinearCorrectResult(corrected=out, batch=labels, averages=avg, reference=ref, stats={"stage_ms": stage_ms})


def design_weights(design, restricted_rows):
    """W = pinv(D[R, :]).T (|R| x p) from a QR of the design's restricted rows, so that coef = X[:, R] @ W.  A design whose
    restricted rows are not of full column rank is refused (R's pivoted QR would drop the aliased columns instead)."""
    dr = design if restricted_rows is None else design[restricted_rows]
    p = design.shape[1]
    if dr.shape[0] < p:
        raise ValueError(f"the design's restricted rows are not of full column rank ({dr.shape[0]} rows, {p} columns)")
    q, r = np.linalg.qr(dr)
    diag = np.abs(np.diag(r))
    if not np.all(np.isfinite(diag)) or diag.min() <= RANK_TOL * max(diag.max(), np.finfo(float).tiny):
        raise ValueError("the design's restricted rows are not of full column rank: remove the aliased columns "
                         "(the reference's pivoted QR would drop them)")
    return np.linalg.solve(r, q.T).T  # D_R = Q R  =>  pinv(D_R) = R^-1 Q^T


def regressBatches(*batches, batch=None, design=None, keep=None, restrict=None, subset_row=None, correct_all=False,
                   d=None, names=None, device=0) -> LinearCorrectResult:
    """regressBatches(..., batch=, design=, keep=, restrict=, subset.row=, correct.all=, d=) (R/regressBatches.R:93-158):
    the residuals of a per-gene linear model fitted on the restricted cells, for every cell.  Without a design the model
    has one blocking term per batch (each batch is centred on the mean of its restricted cells).  `design` is cells x p
    over all cells in the order given (p <= 64), `keep` names 1-based columns of it that are not regressed out.  A single
    object with a `design` but no `batch` is taken as one batch (:124-128).  `d`: also return the first d PCs of the
    residuals (multiBatchPCA over the batches)."""
    mats = _as_matrices(batches, "regressBatches")
    if len(mats) == 0:
        raise ValueError("at least two batches must be specified")  # R/regressBatches.R:133
    G = check_same_dim(mats, byrow=False)
    ncells = [m.shape[1] for m in mats]
    res = restrict_list(restrict, ncells) or [None] * len(mats)
    total = sum(ncells)
    reorder = None
    if len(mats) > 1:
        names = _check_names(names, len(mats))
        labels = _labels(names, ncells)
    else:
        if batch is None:
            if design is None:
                raise ValueError("'batch' must be specified if '...' has only one object")  # R/divideIntoBatches.R:88
            labels = np.ones(total, dtype=np.int64)  # :124-128
        else:
            labels = _check_batch(batch, total)
    if design is not None:
        design = np.asarray(design, dtype=np.float64)
        if design.ndim != 2 or design.shape[0] != total:
            raise ValueError("'nrow(design)' should be equal to the total number of cells")  # R/regressBatches.R:145
    elif keep is not None:
        # the default design written out: model.matrix(~0 + factor(batch)) (:143), levels in sorted order
        levels = sorted(set(labels.tolist())) if len(mats) == 1 else None
        ids = np.repeat(np.arange(len(mats)), ncells) if levels is None else np.searchsorted(np.asarray(levels), labels)
        design = np.zeros((total, int(ids.max()) + 1))
        design[np.arange(total), ids] = 1.0
    if design is not None:
        p = design.shape[1]
        if p < 1 or p > MAX_DESIGN_COLUMNS:
            raise ValueError(f"a design has between 1 and {MAX_DESIGN_COLUMNS} columns, not {p}")
        if not np.all(np.isfinite(design)):
            raise ValueError("the design holds values that are not finite")
        if keep is not None:
            keep = np.asarray(keep, dtype=np.int64).ravel()
            if keep.size and (keep.min() < 1 or keep.max() > p):
                raise ValueError("'keep' indices out of range")
            keep = np.unique(keep).astype(np.int32)
    sub = None if correct_all else subset_index(subset_row, G)  # R/regressBatches.R:136-139
    if sub is not None and sub.size == 0:
        raise ValueError("'subset_row' selects no genes")
    if d is not None and int(d) < 1:
        raise ValueError("'d' must be positive")

    if design is None and len(mats) == 1:
        mats, res, labels_out, reorder = _divide(mats[0], labels, res[0])
    else:
        labels_out = labels
    w = None
    if design is not None:
        if all(r is None for r in res):
            rows = None
        else:
            offs = np.concatenate([[0], np.cumsum(ncells)[:-1]])
            rows = np.concatenate([(np.arange(n) if r is None else np.sort(r.astype(np.int64) - 1)) + o
                                   for r, n, o in zip(res, ncells, offs)])
        w = design_weights(design, rows)
    mats = _rows(mats, sub)
    _lib.require_gpu()
    h = _LinearHandle(mats[0].shape[0], device)
    try:
        if OVERLAP and design is None:
            h.expect(1)
        for m, r in zip(mats, res):
            h.add_batch(m, r)
        out, coef = h.regress(design, w, keep)
        stage_ms = h.stage_ms()
    finally:
        h.close()
    if reorder is not None:
        out = np.asfortranarray(out[:, reorder - 1])
        labels_out = labels_out[reorder - 1]
    result = LinearCorrectResult(corrected=out, batch=labels_out, coefficients=coef, stats={"stage_ms": stage_ms})
    if d is not None:
        result.pcs = _residual_pcs(out, labels_out, int(d), subset_index(subset_row, G) if correct_all else None, device)
    return result


def _residual_pcs(corrected, labels, d, sub, device):
    """.multi_pca_single (R/multiBatchPCA.R:470-508) on the residuals: multiBatchPCA over the batches (the genes of
    subset.row when correct.all kept all of them), the cells' coordinates put back in the caller's order."""
    from .multi_batch_pca import multiBatchPCA
    x = corrected if sub is None else corrected[sub - 1]
    levels = sorted(set(labels.tolist()))
    where = [np.flatnonzero(labels == lv) for lv in levels]
    pca = multiBatchPCA(*[x[:, idx] for idx in where], d=d, device=device)
    pcs = np.empty((x.shape[1], pca["pcs"][0].shape[1]))
    for idx, pc in zip(where, pca["pcs"]):
        pcs[idx] = pc
    return pcs
