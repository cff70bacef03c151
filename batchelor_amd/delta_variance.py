"""mnnDeltaVariance() (R/mnnDeltaVariance.R:95-201): the diagnostic that reads a correction's MNN pairs back.

For every merge step and gene: the mean of the paired cells' (uncorrected) values and the variance of their deltas.  The
hot path is a gather -- every pair reads two whole gene vectors -- so the batches are uploaded once, stay in HBM, and the
statistics of all steps come back in one download (csrc/delta_variance.hip, bmx_delta_*).  The host keeps what needs no
device: the validation of the pairs, the subset.row / compute.all bookkeeping, the trend and the combination over steps.

The batches are all dense or all scipy.sparse (any format, matrix or array: what multiBatchNorm returns for sparse counts
goes straight in).  Sparse ones are made canonical CSC on the host and stay CSC in HBM (bmx_delta_sparse_*): the pair
passes walk the stored entries only, as R/mnnDeltaVariance.R:185-201 does over SVT_SparseMatrix blocks.

scran::fitTrendVar is third-party code outside the reference and is not re-implemented: `trend_fit` takes its place.

Out of scope (a clear error): SingleCellExperiment inputs; a mixture of sparse and dense batches; batches that do not
fit in free HBM, dense or as CSC (restrict the genes with `subset_row`: there is no streaming by gene block).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Callable, List, NamedTuple, Optional

import numpy as np
import scipy.sparse as sp

from . import _lib
from ._handle import ResidentHandle
from .inputs import (all_sparse, canonical_csc, check_same_dim, check_same_rows, check_unique_names, csc_block_width,
                     subset_index, unpack_batches)
from .linear_correct import _as_matrices, _rows  # (_as_matrices: inputs.unpack_batches + the sparse / SCE refusals)

BLOCK_BYTES = 1 << 28  # a batch above this size goes to the device in column blocks of about this many bytes
SPARSE_BLOCK_CELLS = None  # cells per uploaded block of a CSC batch; None: about BLOCK_BYTES of stored entries
STAGES = ("upload", "norms", "pair_passes", "reductions", "run_wall")
FIELDS = ("mean", "total", "trend", "adjusted")


def gene_tile():
    """Genes a workgroup of the pair passes owns (bmx_dev_get "delta_gene_tile"; needs no device)."""
    return _lib.dev_get("delta_gene_tile")


def sparse_gene_tile():
    """Genes a workgroup of the CSC handle's pair passes owns (bmx_dev_get "delta_sparse_gene_tile"; needs no device)."""
    return _lib.dev_get("delta_sparse_gene_tile")


def pair_chunk():
    """Pairs of one step a workgroup of the pair passes walks (bmx_dev_get "delta_pair_chunk"; needs no device)."""
    return _lib.dev_get("delta_pair_chunk")


@dataclass
class DeltaStepTable:
    """One merge step's statistics, a value per gene of `gene_index`."""
    mean: np.ndarray
    total: np.ndarray
    trend: Optional[np.ndarray] = None
    adjusted: Optional[np.ndarray] = None


@dataclass
class MnnDeltaVarianceResult:
    """What mnnDeltaVariance() returns: the reference's DataFrame, column by column."""
    mean: np.ndarray                                 # mean over the pairs of the two cells' mean
    total: np.ndarray                                # variance of the deltas
    trend: Optional[np.ndarray] = None               # None without `trend_fit`
    adjusted: Optional[np.ndarray] = None            # total - trend; None without `trend_fit`
    per_step: Optional[List[DeltaStepTable]] = None  # per.step: one table per merge step when more than one was given
    npairs: Optional[np.ndarray] = None              # pairs per merge step (the weights of the combination)
    gene_index: Optional[np.ndarray] = None          # 1-based row of the inputs behind every value
    stats: Optional[dict] = None                     # "stage_ms": see STAGES


# ---------------------------------------------------------------------------------------------- host side, no device
def _is_vector(v):
    if isinstance(v, np.ndarray):
        return v.ndim == 1
    return isinstance(v, (list, tuple, range)) and all(np.ndim(e) == 0 for e in v)


def _index_vector(v):
    a = np.asarray(v)
    if a.size == 0:
        return np.zeros(0, dtype=np.int64)
    if a.ndim != 1:
        raise ValueError("'pairs' holds one vector of left and one of right cells per merge step")
    if a.dtype.kind not in "iu":
        if a.dtype.kind != "f" or not np.all(a == np.round(a)):
            raise ValueError("'pairs' must hold integer cell indices")
    return a.astype(np.int64)


def check_pairs(pairs, ncells):
    """`pairs` as a list of (left, right) int32 arrays, one entry per merge step.  A single (left, right) is one step (:131-133).
    The indices are 1-based columns of the `ncells` cells of all batches side by side."""
    if pairs is None:
        raise ValueError("'pairs' must be specified")
    if not isinstance(pairs, (list, tuple)):
        raise ValueError("'pairs' is a (left, right) pair of index vectors or a list of them")
    if len(pairs) == 2 and _is_vector(pairs[0]) and _is_vector(pairs[1]):
        pairs = [pairs]
    if len(pairs) == 0:
        raise ValueError("'pairs' must hold at least one merge step")
    out = []
    for step in pairs:
        if not isinstance(step, (list, tuple)) or len(step) != 2:
            raise ValueError("'pairs' holds one vector of left and one of right cells per merge step")
        left, right = _index_vector(step[0]), _index_vector(step[1])
        if left.size != right.size:
            raise ValueError("'left' and 'right' of a merge step differ in length")
        for v in (left, right):
            if v.size and (v.min() < 1 or v.max() > ncells):
                raise ValueError("'pairs' indices out of range")
        out.append((np.ascontiguousarray(left, dtype=np.int32), np.ascontiguousarray(right, dtype=np.int32)))
    return out


class GenePlan(NamedTuple):
    rows: Optional[np.ndarray]         # 1-based rows of the inputs that go to the device; None = all
    norm_genes0: Optional[np.ndarray]  # 0-based uploaded rows the cosine norms are taken over; None = all of them
    fit_rows0: Optional[np.ndarray]    # 0-based uploaded rows the trend is fitted on; None = all of them
    gene_index: np.ndarray             # 1-based row of the inputs behind every uploaded row


def plan_genes(subset_row, compute_all, G):
    """:113-119: without compute.all the subset is taken first and then forgotten; with it every gene is kept and the
    subset only restricts the cosine norms (:122) and the trend fit (:155-157)."""
    sub = subset_index(subset_row, G)
    if sub is None:
        return GenePlan(None, None, None, np.arange(1, G + 1))
    if sub.size == 0:
        raise ValueError("'subset_row' selects no genes")
    if not compute_all:
        return GenePlan(sub, None, None, sub.astype(np.int64))
    zero = np.ascontiguousarray(sub - 1, dtype=np.int32)
    return GenePlan(None, zero, zero, np.arange(1, G + 1))


def step_table(mean, total, npairs, trend_fit=None, fit_rows0=None):
    """:154-162 for one step: the trend is fitted on the `fit_rows0` genes and evaluated on all of them.  A step with
    fewer than two pairs has no variances to fit: its trend is NaN (it gets no weight in the combination)."""
    if trend_fit is None:
        return DeltaStepTable(mean=mean, total=total)
    if npairs < 2:
        trend = np.full(mean.shape, np.nan)
    else:
        fm, ft = (mean, total) if fit_rows0 is None else (mean[fit_rows0], total[fit_rows0])
        trend = np.asarray(trend_fit(fm, ft)(mean), dtype=np.float64)
        if trend.shape != mean.shape:
            raise ValueError("the fitted trend must return one value per gene")
    return DeltaStepTable(mean=mean, total=total, trend=trend, adjusted=total - trend)


def combine_steps(tables, npairs):
    """scran::combineBlocks(ave.fields=, equiweight=FALSE, weights=npairs, valid=npairs >= 2) (:167-172): every field is
    sum_i P_i value_i / sum_i P_i over the steps with at least two pairs; NaN when there is none."""
    npairs = np.asarray(npairs, dtype=np.int64)
    valid = np.flatnonzero(npairs >= 2)
    out = {}
    for f in FIELDS:
        first = getattr(tables[0], f)
        if first is None:
            out[f] = None
            continue
        if valid.size == 0:
            out[f] = np.full(first.shape, np.nan)
            continue
        if valid.size == 1:  # (the weighted mean of one step is that step: no P v / P rounding)
            out[f] = getattr(tables[valid[0]], f).copy()
            continue
        acc = np.zeros(first.shape)
        for i in valid:
            acc += float(npairs[i]) * getattr(tables[i], f)
        out[f] = acc / float(npairs[valid].sum())
    return out


# ---------------------------------------------------------------------------------------------- the device side
class _DeltaHandle(ResidentHandle):
    """bmx_delta_t: the batches stay in HBM; one run gives the statistics of every merge step."""
    PREFIX = "bmx_delta"
    STAGES = STAGES

    def add_batch(self, x, block_bytes=None):
        self._upload(x, BLOCK_BYTES if block_bytes is None else block_bytes)

    def run(self, steps, cos_norm=False, norm_genes0=None):
        S = len(steps)
        lp = (ctypes.c_void_p * S)(*[l.ctypes.data for l, _ in steps])
        rp = (ctypes.c_void_p * S)(*[r.ctypes.data for _, r in steps])
        counts = np.asarray([l.size for l, _ in steps], dtype=np.int64)
        mean = np.empty((self.G, S), dtype=np.float64, order="F")
        total = np.empty((self.G, S), dtype=np.float64, order="F")
        ng = 0 if norm_genes0 is None else int(norm_genes0.size)
        self._call("run", ctypes.c_int32(int(bool(cos_norm))), None if norm_genes0 is None else _lib.i32p(norm_genes0),
                   ctypes.c_int32(ng), ctypes.c_int32(S), lp, rp, counts.ctypes.data_as(_lib.c_i64p), _lib.f64p(mean),
                   _lib.f64p(total))
        return mean, total


class _DeltaSparseHandle(_DeltaHandle):
    """bmx_delta_sparse_t: the same over canonical CSC batches (inputs.canonical_csc), kept CSC in HBM."""
    PREFIX = "bmx_delta_sparse"

    def add_batch(self, c, block_cells=None):
        if block_cells is None:
            block_cells = SPARSE_BLOCK_CELLS
        self._upload_csc(c, csc_block_width(c, BLOCK_BYTES) if block_cells is None else max(1, int(block_cells)))


def csc_batches(mats, rows=None):
    """scipy.sparse batches as canonical CSC; `rows` (1-based, in any order) are taken from each on the host and the result
    is made canonical again."""
    out = [canonical_csc(m)[0] for m in mats]
    return out if rows is None else [canonical_csc(c[np.asarray(rows, dtype=np.int64) - 1])[0] for c in out]


def device_statistics(mats, steps, cos_norm=False, norm_genes0=None, device=0):
    """The device's part of a call: `mats` genes x cells matrices with the same rows -- all numpy arrays, or all canonical
    CSC (csc_batches) --, `steps` what check_pairs() returns.  Returns mean and total, [genes x steps] each, as the kernels
    leave them (a step with one pair still has its mean), and the stage times."""
    _lib.require_gpu()
    h = (_DeltaSparseHandle if sp.issparse(mats[0]) else _DeltaHandle)(mats[0].shape[0], device)
    try:
        for m in mats:
            h.add_batch(m)
        mean, total = h.run(steps, cos_norm, norm_genes0)
        return mean, total, h.stage_ms()
    finally:
        h.close()


def mnnDeltaVariance(*batches, pairs=None, cos_norm=False, subset_row=None, compute_all=False,
                     trend_fit: Optional[Callable] = None, names=None, device=0) -> MnnDeltaVarianceResult:
    """mnnDeltaVariance(..., pairs=, cos.norm=, subset.row=, compute.all=) (R/mnnDeltaVariance.R:95-201).

    Each batch is genes x cells of (uncorrected) log-expression values; the batches are all dense or all scipy.sparse
    (implicit zeros are zeros: sparse logcounts as multiBatchNorm returns them).  `pairs` is one (left, right) pair of equal-length
    1-based index vectors or a list of them, one entry per merge step, over the cells of the batches side by side in the
    order given: what fastMNN(...).merge_info.pairs and mnnCorrect(...).merge_info.pairs hold.  Per step, `total` is the
    variance of x[, left] - x[, right] across the pairs and `mean` the mean of the two cells' means; the steps are
    combined with their numbers of pairs as weights, steps with fewer than two pairs left out (NaN if none remains).

    `trend_fit` stands in for scran::fitTrendVar, which is not re-implemented: a callable (mean, total) -> callable(mean)
    -> trend, applied per step (on the `subset_row` genes when `compute_all` is set).  Without it `trend` and `adjusted`
    are None.  `names` plays the role of the argument names of `...`."""
    sparse = all_sparse(unpack_batches(batches), "mnnDeltaVariance")
    mats = list(unpack_batches(batches)) if sparse else _as_matrices(batches, "mnnDeltaVariance")
    if len(mats) == 0:
        raise ValueError("at least one batch must be specified")
    G = check_same_rows(mats) if sparse else check_same_dim(mats, byrow=False)
    if names is not None:
        names = [str(v) for v in names]
        if len(names) != len(mats):
            raise ValueError("'names' must have one entry per batch")
        check_unique_names(names)
    steps = check_pairs(pairs, sum(m.shape[1] for m in mats))
    plan = plan_genes(subset_row, compute_all, G)
    if trend_fit is not None and not callable(trend_fit):
        raise ValueError("'trend_fit' must be callable")
    mats = csc_batches(mats, plan.rows) if sparse else _rows(mats, plan.rows)
    mean, total, stage_ms = device_statistics(mats, steps, cos_norm, plan.norm_genes0, device)
    npairs = np.asarray([l.size for l, _ in steps], dtype=np.int64)
    tables = [step_table(np.ascontiguousarray(mean[:, i]), np.ascontiguousarray(total[:, i]), int(npairs[i]), trend_fit,
                         plan.fit_rows0) for i in range(len(steps))]
    comb = combine_steps(tables, npairs)
    return MnnDeltaVarianceResult(mean=comb["mean"], total=comb["total"], trend=comb["trend"], adjusted=comb["adjusted"],
                                  per_step=tables if len(tables) > 1 else None, npairs=npairs,
                                  gene_index=plan.gene_index, stats={"stage_ms": stage_ms})
