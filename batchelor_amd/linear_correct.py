"""rescaleBatches() (R/rescaleBatches.R:63-150) and regressBatches() (R/regressBatches.R:93-158): the linear corrections.

Both are per-gene passes over genes x cells FP64 matrices: per-gene statistics over each batch's restricted cells, then one
pass that writes every cell.  The batches are uploaded once (whole or in column blocks), stay in HBM between the two
passes, and the result comes back block by block behind the kernels (csrc/linear_correct.hip, bmx_linear_*).

regressBatches: the reference delegates to ResidualMatrix; the definition used here (man/regressBatches.Rd, the
reference's tests) is, with X genes x cells, D cells x p the design and R the restricted cells,
    coef = argmin || X[:, R] - coef @ D[R, :].T ||,   out = X - coef[:, drop] @ D[:, drop].T,
drop = the columns of D not named in `keep`.  Without a design D has one indicator column per batch, coef is the batch
means and no product is formed.  With a design the host factors D[R, :] (QR) and the device forms both skinny products.

regressBatches(d=): the PCs of the residuals (multiBatchPCA over the batches).  By default the residuals come back to the
host, are split by batch and go to multiBatchPCA.  With deferred=True (the reference's ResidualMatrix with deferred=TRUE)
they are never formed: the residual of batch b is x_b - F E_b^T of rank <= 65 away from the resident x_b, so the subspace
iteration applies its two products to x_b and takes the low-rank term off the two skinny results
(bmx_residual_pca_*).  residuals=False then skips the second pass and its download altogether.

Out of scope (a clear error): sparse and SingleCellExperiment inputs, designs of more than 64 columns, a design whose
restricted rows are not of full column rank (R's pivoted QR would drop columns instead), BSPARAM, deferred=True for one
object with both `design` and `batch` (the resident batch is then the whole object, not the PCA's batches).
"""
from __future__ import annotations

import ctypes
import time
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
    corrected: Optional[np.ndarray]            # genes x cells (column-major), cells in the caller's order; None: residuals=False
    batch: np.ndarray                          # batch id (1-based) or name per cell
    averages: Optional[np.ndarray] = None      # rescaleBatches: genes x batches, mean unlogged value of the restricted cells
    reference: Optional[np.ndarray] = None     # rescaleBatches: genes, the minimum of `averages` over the batches
    coefficients: Optional[np.ndarray] = None  # regressBatches: genes x p (default design: the batch means)
    pcs: Optional[np.ndarray] = None           # regressBatches(d=): cells x d
    pca: Optional[dict] = None                 # regressBatches(d=, deferred=True): rotation, centers, d, iters_used, residual, path
    stats: Optional[dict] = None               # "stage_ms": see STAGES; deferred PCA: "pca_fit_ms"


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


class _ResidualPCA:
    """bmx_residual_pca_t: the PCA of the residuals over the first n_pca_rows rows of a _LinearHandle whose batches are all
    resident.  The wrapper keeps its _LinearHandle alive; close() this one first."""

    def __init__(self, linear, n_pca_rows):
        self.linear, self.n_pca, self.d = linear, int(n_pca_rows), 0
        self._h = ctypes.c_void_p()
        lib = _lib.lib()
        lib.bmx_residual_pca_destroy.argtypes = [ctypes.c_void_p]
        lib.bmx_residual_pca_destroy.restype = None
        _lib.check(lib.bmx_residual_pca_create(ctypes.c_int32(self.n_pca), linear._h, ctypes.byref(self._h)))

    def fit(self, design, w, keep, d, tol, max_iters, iters=None, weights=None):
        """bmx_residual_pca_fit: (coefficients, multiBatchPCA's record of the residuals' first n_pca_rows rows).  iters=N:
        the fixed-count form (N plain subspace steps, no test).  A run that misses tol raises, as DevicePCA.fit."""
        nS, d, lin = self.n_pca, int(d), self.linear
        centers, rotation, sdev = np.zeros(nS), np.zeros((nS, d), order="F"), np.zeros(d)
        used, res = ctypes.c_int32(0), ctypes.c_double(0.0)
        wts = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        if design is None:
            coef = np.empty((lin.G, len(lin.ncells)), dtype=np.float64, order="F")
            dargs = (None, ctypes.c_int32(0), None, None, ctypes.c_int32(0))
        else:
            design, w = _lib.as_f(design), _lib.as_f(w)
            keep = np.zeros(0, dtype=np.int32) if keep is None else np.ascontiguousarray(keep, dtype=np.int32)
            coef = np.empty((lin.G, design.shape[1]), dtype=np.float64, order="F")
            dargs = (_lib.f64p(design), ctypes.c_int32(design.shape[1]), _lib.f64p(w),
                     _lib.i32p(keep) if keep.size else None, ctypes.c_int32(int(keep.size)))
        fixed = iters is not None
        self.d = d
        _lib.check(_lib.lib().bmx_residual_pca_fit(
            self._h, *dargs, None if wts is None else _lib.f64p(wts), ctypes.c_int32(d),
            ctypes.c_double(0.0 if fixed else float(tol)), ctypes.c_int32(int(iters if fixed else max_iters)),
            _lib.f64p(coef), _lib.f64p(centers), _lib.f64p(rotation), _lib.f64p(sdev), ctypes.byref(used),
            ctypes.byref(res)))
        return coef, {"rotation": np.ascontiguousarray(rotation), "centers": centers, "d": sdev,
                      "iters_used": int(used.value), "residual": float("nan") if fixed else float(res.value)}

    def project(self, b):
        out = np.zeros((self.linear.ncells[b], self.d), order="F")
        _lib.check(_lib.lib().bmx_residual_pca_project(self._h, ctypes.c_int32(int(b)), _lib.f64p(out)))
        return np.ascontiguousarray(out)

    def close(self):
        if self._h:
            _lib.lib().bmx_residual_pca_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


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
                   d=None, names=None, device=0, deferred=False, residuals=True, pca_tol=1e-9, pca_maxit=500,
                   pca_iters=None) -> LinearCorrectResult:
    """regressBatches(..., batch=, design=, keep=, restrict=, subset.row=, correct.all=, d=) (R/regressBatches.R:93-158):
    the residuals of a per-gene linear model fitted on the restricted cells, for every cell.  Without a design the model
    has one blocking term per batch (each batch is centred on the mean of its restricted cells).  `design` is cells x p
    over all cells in the order given (p <= 64), `keep` names 1-based columns of it that are not regressed out.  A single
    object with a `design` but no `batch` is taken as one batch (:124-128).  `d`: also return the first d PCs of the
    residuals (multiBatchPCA over the batches).

    deferred=True (with `d`): the PCs come from the batches resident on the device, the residuals being their data less a
    term of rank <= 65 that is never written (module docstring); `pcs` is in the caller's cell order and `pca` holds
    {"rotation", "centers", "d", "iters_used", "residual", "path": "device-deferred"}, over the genes of subset_row where
    correct_all kept all of them.  pca_tol / pca_maxit / pca_iters are multiBatchPCA's tol / max_iters / iters.  The PCA's
    batches are the resident ones: the objects, the parts of one object divided by `batch`, or one object with a `design`
    and no `batch`; one object with both is a ValueError.  A shape the device PCA does not take
    (multi_batch_pca.device_pca_takes) goes the default way and `pca["path"]` says so.  residuals=False (only with
    deferred=True and `d`): the second pass and its download are skipped and `corrected` is None."""
    deferred, residuals = bool(deferred), bool(residuals)
    if deferred and d is None:
        raise ValueError("'deferred=True' needs 'd': it is the PCA of the residuals that is deferred")
    if not residuals and not deferred:
        raise ValueError("'residuals=False' needs 'deferred=True' and 'd': without them the PCs are taken from the residuals")
    if deferred:
        pca_tol = float(pca_tol)
        if not (np.isfinite(pca_tol) and pca_tol > 0):
            raise ValueError("'pca_tol' must be positive and finite")
        if int(pca_maxit) < 1 or (pca_iters is not None and int(pca_iters) < 1):
            raise ValueError("'pca_maxit' and 'pca_iters' must be positive")
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
    if deferred and design is not None and len(mats) == 1 and batch is not None:
        raise ValueError("'deferred=True' takes the batches resident on the device as the PCA's batches: one object with "
                         "both 'design' (or 'keep') and 'batch' stays whole there; pass the batches as separate objects "
                         "or leave 'deferred' off")

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
    # deferred with correct_all: the rows go up as [subset_row; the others], as multiBatchPCA uploads them, so that the PCA
    # rows are a prefix; every gene is independent of the others, so its bits do not depend on where it stands
    order = None
    n_pca = G if sub is None else sub.size
    if deferred and correct_all:
        pca_sub = subset_index(subset_row, G)
        if pca_sub is not None:
            if pca_sub.size == 0:
                raise ValueError("'subset_row' selects no genes")
            first = pca_sub.astype(np.int64) - 1
            rest = np.ones(G, dtype=bool)
            rest[first] = False
            order, n_pca = np.concatenate([first, np.flatnonzero(rest)]), first.size
    mats = _rows(mats, sub) if order is None else [m[order] for m in mats]
    _lib.require_gpu()
    h = _LinearHandle(mats[0].shape[0], device)
    out = pca = pcs = fit_ms = None
    try:
        if OVERLAP and design is None:
            h.expect(1)
        for m, r in zip(mats, res):
            h.add_batch(m, r)
        if deferred:
            from .multi_batch_pca import device_pca_takes
            why = None if device_pca_takes(n_pca, sum(h.ncells), int(d)) else \
                "fewer genes / cells than the device block, or d > 120"
            if why is None:
                rp = _ResidualPCA(h, n_pca)
                try:
                    t0 = time.perf_counter()
                    coef, pca = rp.fit(design, w, keep, int(d), pca_tol, pca_maxit, pca_iters)
                    fit_ms = (time.perf_counter() - t0) * 1e3
                    pca["path"] = "device-deferred"
                    pcs = np.concatenate([rp.project(b) for b in range(len(mats))], axis=0)
                except _lib.BatchelorMI355XError as exc:
                    if "rank below the subspace width" not in str(exc):
                        raise
                    why = "residuals of rank below the device block"
                finally:
                    rp.close()
        if residuals or pca is None:
            out, coef = h.regress(design, w, keep)
        stage_ms = h.stage_ms()
    finally:
        h.close()
    if deferred and pca is None:  # today's route, on the PCA rows of the residuals as uploaded
        pcs, pca = _residual_pcs(out[:n_pca], labels_out, int(d), None, device, tol=pca_tol, max_iters=pca_maxit,
                                 iters=pca_iters)
        pca["path"] = "residuals through the host (" + why + "), then " + pca["path"]
        if not residuals:
            out = None
    if order is not None:  # back to the caller's rows (a row named twice went up twice, with the same result)
        back = np.empty((G, coef.shape[1]), order="F")
        back[order] = coef
        coef = back
        if out is not None:
            back = np.empty((G, out.shape[1]), order="F")
            back[order] = out
            out = back
    if reorder is not None:
        out = None if out is None else np.asfortranarray(out[:, reorder - 1])
        if pcs is not None:
            pcs = pcs[reorder - 1]
        labels_out = labels_out[reorder - 1]
    result = LinearCorrectResult(corrected=out, batch=labels_out, coefficients=coef, stats={"stage_ms": stage_ms})
    if deferred:
        result.pcs, result.pca = pcs, pca
        if fit_ms is not None:
            result.stats["pca_fit_ms"] = fit_ms  # host wall time of bmx_residual_pca_fit (coefficients and PCA)
    elif d is not None:
        result.pcs = _residual_pcs(out, labels_out, int(d), subset_index(subset_row, G) if correct_all else None, device)[0]
    return result


def _residual_pcs(corrected, labels, d, sub, device, **fit):
    """.multi_pca_single (R/multiBatchPCA.R:470-508) on the residuals: multiBatchPCA over the batches (the genes of
    subset.row when correct.all kept all of them), the cells' coordinates put back in the order of `labels`; and
    multiBatchPCA's record without its "pcs".  fit: multiBatchPCA's tol / max_iters / iters."""
    from .multi_batch_pca import multiBatchPCA
    x = corrected if sub is None else corrected[sub - 1]
    levels = sorted(set(labels.tolist()))
    where = [np.flatnonzero(labels == lv) for lv in levels]
    pca = multiBatchPCA(*[x[:, idx] for idx in where], d=d, device=device, **fit)
    parts = pca.pop("pcs")
    pcs = np.empty((x.shape[1], parts[0].shape[1]))
    for idx, pc in zip(where, parts):
        pcs[idx] = pc
    return pcs, pca
