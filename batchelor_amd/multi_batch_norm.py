"""multiBatchNorm() (R/multiBatchNorm.R:88-280): per-batch size factors rescaled so that the batches' average counts agree,
then log-normalized values.  The function the other corrections' inputs come from.

The counts (genes x cells) are uploaded once, whole or in column blocks, and stay in HBM.  Library sizes and the
per-gene sums run behind the upload; the pairwise median ratios, the choice of the reference batch and the rescaling
are taken on the device; one elementwise pass writes the values, which come back block by block behind the kernels
(csrc/multi_batch_norm.hip, bmx_norm_*).  scuttle's helpers are used as include/batchelor_mi355x.h states them:
    size factors  given / mean(given), or lib / mean(lib) with lib the column sums over subset_row; all finite and > 0
    averages      rowMeans(t(t(x) / sf)) over subset_row
    values        log2(x / sf + pseudo_count), the size factors never re-centred (center.size.factors=FALSE)

Sparse counts: batches that are scipy.sparse matrices or arrays (all of a call, or none) are brought to canonical CSC on the
host -- duplicates summed, rows ascending, float64 values, int32 rows -- and stay CSC in HBM (bmx_norm_sparse_*).  The
per-gene sums take their terms in the dense path's order with the zeros left out, so with the same size factors every
statistic equals the dense path's bit for bit.  Values are computed for the stored entries only (a stored zero is a value
like any other): where a zero maps to 0.0 -- log=False, or log2(pseudo_count) == 0 on the device -- `logcounts` is CSC with
the pattern of the canonical input, otherwise it is dense as R's is, filled with the device's image of a zero.

Out of scope (a clear error where it can be reached): SingleCellExperiment inputs (TypeError), hence altExp handling;
sparse and dense batches in one call (TypeError); integer or float32 storage on the device (inputs are converted to FP64
as elsewhere); logNormCounts
arguments other than `log` and `pseudo_count` in norm_args (`downsample`, `transform`, `size.factors`, ...: ValueError);
handing the result to fastMNN without a copy to the host; batches that do not fit in HBM together (the allocation fails
with BatchelorMI355XError).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Union

import numpy as np
import scipy.sparse as sp

from . import _lib
from ._handle import ResidentHandle
from .inputs import (all_sparse, canonical_csc, check_same_dim, check_same_rows, csc_block_width, divide_into_batches,
                     subset_index, unpack_batches)
from .inputs import csc_blocks  # noqa: F401  (the helper's old import path)
from .linear_correct import _as_matrices, _check_batch, _check_names

BLOCK_BYTES = 1 << 28   # a batch above this size goes to the device in column blocks of about this many bytes
CHUNK = 256             # cells per chunk of the device's per-gene sums: block widths are multiples of it
STAGES = ("upload", "statistics", "ratios", "output_kernels", "output_wall")
NORM_ARGS = ("log", "pseudo_count")


@dataclass
class MultiBatchNormResult:
    """What multiBatchNorm() returns."""
    logcounts: Union[list, np.ndarray]     # per batch genes x cells, or one matrix in the caller's cell order (column-major);
                                           # sparse counts: CSC where a zero stays 0.0, dense otherwise
    size_factors: Union[list, np.ndarray]  # the size factors the values were divided by, same shape
    batch: np.ndarray                      # per batch its id (1-based), name or level; one object kept whole: per cell
    averages: np.ndarray                   # |subset_row| x batches
    ratios: np.ndarray                     # batches x batches, [i, j] = median(averages[:, j] / averages[:, i])
    reference: object                      # the batch every other is scaled to: 1-based index, name or level
    stats: Optional[dict] = None           # "stage_ms": see STAGES


class _NormHandle(ResidentHandle):
    """bmx_norm_t: the counts stay in HBM between the statistics, the ratio stage and the pass that writes the values."""
    PREFIX = "bmx_norm"
    STAGES = STAGES

    def __init__(self, n_genes, device, stat_rows=None):
        rows = None if stat_rows is None else np.ascontiguousarray(stat_rows, dtype=np.int32)
        super().__init__(n_genes, device, None if rows is None else _lib.i32p(rows),
                         ctypes.c_int64(-1 if rows is None else int(rows.size)))
        self.n_stat = self.G if rows is None else int(rows.size)

    def add_batch(self, x, size_factors=None, block_bytes=None):
        """x: genes x cells.  A blocked upload gives the bits of a whole one for any block width; the widths are still
        rounded to whole chunks so that every block's per-gene sums can start behind the next block's copy."""
        bb = BLOCK_BYTES if block_bytes is None else block_bytes
        per = max(1, int(bb) // (8 * self.G))
        per = max(CHUNK, per // CHUNK * CHUNK)
        sf = None if size_factors is None else np.ascontiguousarray(size_factors, dtype=np.float64)
        self._upload(x, per * 8 * self.G, None if sf is None else _lib.f64p(sf))

    def run(self, min_mean, log, pseudo_count):
        N, B = sum(self.ncells), len(self.ncells)
        out = np.empty((self.G, N), dtype=np.float64, order="F")
        ptrs = (ctypes.c_void_p * B)()
        at = 0
        for i, n in enumerate(self.ncells):
            ptrs[i] = out.ctypes.data + at * self.G * 8
            at += n
        sf = np.empty(N, dtype=np.float64)
        ave = np.empty((self.n_stat, B), dtype=np.float64, order="F")
        ratios = np.empty((B, B), dtype=np.float64)
        smallest = ctypes.c_int32(0)
        self._call("run", ctypes.c_double(float(min_mean)), ctypes.c_int32(int(bool(log))),
                   ctypes.c_double(float(pseudo_count)), ptrs, _lib.f64p(sf), _lib.f64p(ave), _lib.f64p(ratios),
                   ctypes.byref(smallest))
        return out, sf, ave, ratios, int(smallest.value)


class _SparseNormHandle(ResidentHandle):
    """bmx_norm_sparse_t: _NormHandle for counts kept as CSC in HBM."""
    PREFIX = "bmx_norm_sparse"
    STAGES = STAGES

    def __init__(self, n_genes, device, stat_rows=None):
        rows = None if stat_rows is None else np.ascontiguousarray(stat_rows, dtype=np.int32)
        super().__init__(n_genes, device, None if rows is None else _lib.i32p(rows),
                         ctypes.c_int64(-1 if rows is None else int(rows.size)))
        self.n_stat = self.G if rows is None else int(rows.size)
        self.nnz = []

    def add_batch(self, c, size_factors=None, block_bytes=None):
        """c: canonical CSC, genes x cells.  The blocks are whole chunks of cells, as many as hold about block_bytes of
        stored entries (12 bytes each) at the batch's mean density."""
        per = csc_block_width(c, BLOCK_BYTES if block_bytes is None else block_bytes)
        per = max(CHUNK, per // CHUNK * CHUNK)
        sf = None if size_factors is None else np.ascontiguousarray(size_factors, dtype=np.float64)
        self._upload_csc(c, per, None if sf is None else _lib.f64p(sf))
        self.nnz.append(int(c.nnz))

    def run(self, min_mean, log, pseudo_count):
        N, B = sum(self.ncells), len(self.ncells)
        outs = [np.empty(k, dtype=np.float64) for k in self.nnz]
        ptrs = (ctypes.c_void_p * B)(*[o.ctypes.data for o in outs])
        sf = np.empty(N, dtype=np.float64)
        ave = np.empty((self.n_stat, B), dtype=np.float64, order="F")
        ratios = np.empty((B, B), dtype=np.float64)
        smallest, zero = ctypes.c_int32(0), ctypes.c_double(0.0)
        self._call("run", ctypes.c_double(float(min_mean)), ctypes.c_int32(int(bool(log))),
                   ctypes.c_double(float(pseudo_count)), ptrs, _lib.f64p(sf), _lib.f64p(ave), _lib.f64p(ratios),
                   ctypes.byref(smallest), ctypes.byref(zero))
        return outs, float(zero.value), sf, ave, ratios, int(smallest.value)


def _check_size_factors(sf, n):
    sf = np.asarray(sf, dtype=np.float64)
    if sf.ndim != 1 or sf.shape[0] != n:
        raise ValueError("'size_factors' must hold one value per cell of its batch")
    if not np.all(np.isfinite(sf) & (sf > 0)):
        raise ValueError("size factors should be positive")
    return sf


def multiBatchNorm(*batches, batch=None, size_factors=None, norm_args=None, min_mean=1, subset_row=None,
                   normalize_all=False, preserve_single=True, names=None, device=0) -> MultiBatchNormResult:
    """multiBatchNorm(..., batch=, norm.args=, min.mean=, subset.row=, normalize.all=, preserve.single=)
    (R/multiBatchNorm.R:88-171).  Each batch is a genes x cells matrix of counts, all dense or all scipy.sparse (see the
    module's text for what a sparse call returns); one object plus `batch=` is split by column (levels sorted).
    `size_factors`: one vector per batch (one vector over all cells for a single object), in
    place of sizeFactors(); None: library sizes over `subset_row`.  `norm_args`: `log` (default True) and `pseudo_count`
    (default 1).  `names` plays the role of the argument names of `...`.  With one object and preserve_single the result
    is one matrix and one vector in the caller's cell order, otherwise lists with one entry per batch."""
    sparse = all_sparse(unpack_batches(batches), "multiBatchNorm")
    mats = [b.tocsc() for b in unpack_batches(batches)] if sparse else _as_matrices(batches, "multiBatchNorm")
    if len(mats) == 0:
        raise ValueError("at least one matrix of counts must be supplied")  # R/multiBatchNorm.R:118
    G = check_same_rows(mats) if sparse else check_same_dim(mats, byrow=False)
    norm_args = dict(norm_args or {})
    for key in norm_args:
        if key not in NORM_ARGS:
            raise ValueError(f"'norm_args' takes {' and '.join(NORM_ARGS)} only, not '{key}'")
    log, pseudo_count = bool(norm_args.get("log", True)), float(norm_args.get("pseudo_count", 1))
    if not np.isfinite(pseudo_count):
        raise ValueError("'pseudo_count' must be finite")
    min_mean = float(min_mean)
    if np.isnan(min_mean):
        raise ValueError("'min_mean' must be a number")
    sub = subset_index(subset_row, G)
    if sub is not None and sub.size == 0:
        raise ValueError("'subset_row' selects no genes")

    reorder = None
    if len(mats) == 1:
        if batch is None:
            raise ValueError("'batch' must be specified if '...' has only one object")  # R/multiBatchNorm.R:102
        batch = _check_batch(batch, mats[0].shape[1])
        sfs = None if size_factors is None else _check_size_factors(size_factors, mats[0].shape[1])
        div = divide_into_batches(mats[0], batch, also=() if sfs is None else (sfs,))
        mats, labels, reorder = div.parts, list(div.levels), div.reorder
        sfs = [None] * len(mats) if sfs is None else div.also[0]
    else:
        preserve_single = False  # R/multiBatchNorm.R:120
        names = _check_names(names, len(mats))
        labels = list(range(1, len(mats) + 1)) if names is None else names
        if size_factors is None:
            sfs = [None] * len(mats)
        else:
            if len(size_factors) != len(mats):
                raise ValueError("'size_factors' must have one vector per batch")
            sfs = [None if s is None else _check_size_factors(s, m.shape[1]) for s, m in zip(size_factors, mats)]
    for m in mats:
        if m.shape[1] == 0:
            raise ValueError("every batch needs at least one cell")

    stat_rows = None
    if sub is not None:
        if normalize_all:
            stat_rows = sub                      # values for every row, statistics over subset_row
        else:
            mats = [m[sub - 1] for m in mats]    # R/multiBatchNorm.R:146-148, :162-164
    if sparse:  # (a batch that is still the caller's object lends its index arrays: the result gets copies of them)
        given = {id(b) for b in unpack_batches(batches)}
        mats, owned = zip(*[(c, own or id(m) not in given) for m in mats for c, own in [canonical_csc(m)]])
    _lib.require_gpu()
    h = (_SparseNormHandle if sparse else _NormHandle)(mats[0].shape[0], device, stat_rows)
    try:
        for m, s in zip(mats, sfs):
            h.add_batch(m, s)
        if sparse:
            values, zero, sf, ave, ratios, smallest = h.run(min_mean, log, pseudo_count)
        else:
            out, sf, ave, ratios, smallest = h.run(min_mean, log, pseudo_count)
        stage_ms = h.stage_ms()
    finally:
        h.close()

    if sparse and zero == 0.0:  # a zero stays a zero: the result keeps the pattern
        parts = [sp.csc_matrix((v, m.indices if o else m.indices.copy(), m.indptr if o else m.indptr.copy()), shape=m.shape)
                 for v, m, o in zip(values, mats, owned)]
        out = None
    elif sparse:                # dense, as R's: the image of a zero everywhere, the stored entries scattered in
        out = np.full((mats[0].shape[0], sum(m.shape[1] for m in mats)), zero, dtype=np.float64, order="F")
        at = 0
        for v, m in zip(values, mats):
            out[m.indices, at + np.repeat(np.arange(m.shape[1]), np.diff(m.indptr))] = v
            at += m.shape[1]

    if out is None:
        edges = np.concatenate([[0], np.cumsum([m.shape[1] for m in mats])])
        if reorder is not None and preserve_single:
            logcounts = sp.hstack(parts, format="csc")[:, reorder - 1]
            size_out, labels_out = sf[reorder - 1], batch
        else:
            logcounts, labels_out = parts, np.asarray(labels)
            size_out = [sf[a:b] for a, b in zip(edges[:-1], edges[1:])]
    elif reorder is not None and preserve_single:
        logcounts = np.asfortranarray(out[:, reorder - 1])  # sizeFactors(sce) <- all.sf[reorder] (:150-152)
        size_out = sf[reorder - 1]
        labels_out = batch
    else:
        edges = np.concatenate([[0], np.cumsum([m.shape[1] for m in mats])])
        logcounts = [out[:, a:b] for a, b in zip(edges[:-1], edges[1:])]
        size_out = [sf[a:b] for a, b in zip(edges[:-1], edges[1:])]
        labels_out = np.asarray(labels)
    return MultiBatchNormResult(logcounts=logcounts, size_factors=size_out, batch=labels_out, averages=ave, ratios=ratios,
                                reference=labels[smallest - 1], stats={"stage_ms": stage_ms})
