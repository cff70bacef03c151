"""modelGeneVar(), combineVar() and getTopHVGs(): the per-gene variance modelling that quickCorrect()
(R/quickCorrect.R:87-114) runs between multiBatchNorm and the correction.

The three functions belong to scran, which is neither part of the reference nor re-implemented here.  What they compute
is stated in their docstrings below; THESE STATEMENTS ARE ASSUMPTIONS ABOUT SCRAN, written from its documentation, and
tests/model_gene_var_ref.py restates them in numpy:
    modelGeneVar   per gene the mean and the sample variance (denominator n - 1) of the log-values over the cells of a
                   block; a trend fitted to (mean, total) splits `total` into `tech` and `bio`; blocks are combined by
                   combineVar, blocks with fewer than two cells left out
    combineVar     per gene the average of every field over the tables, unweighted (equiweight) or weighted by the cells
    getTopHVGs     the genes with the largest `bio` (or `total`) above a threshold, by decreasing value
scran::fitTrendVar is not re-implemented (as in delta_variance.py): `trend_fit` takes its place, and without it there is
no `tech` / `bio`.  p-values and FDR columns are not computed.

The hot path is the mean and variance: a streaming reduction over genes x cells, on the device (csrc/gene_var.hip,
bmx_genevar_* / bmx_genevar_sparse_*).  A batch passes through two block buffers and never has to fit in HBM; chunks of
256 cells at fixed positions are reduced in two sweeps and merged in order, so the results do not depend on the block
width, and a batch's statistics do not depend on what was uploaded before it.  Sparse input stays CSC.

Out of scope: reading the counts a multiBatchNorm handle already holds (the values are uploaded again); handing the
chosen rows to the PCA handle on the device; SingleCellExperiment inputs (TypeError).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Callable, List, Optional

import numpy as np
import scipy.sparse as sp

from . import _lib
from ._handle import ResidentHandle
from .inputs import canonical_csc, csc_block_width, divide_into_batches, subset_index
from .linear_correct import _as_matrices, _check_batch

BLOCK_BYTES = 1 << 28   # a batch above this size goes to the device in column blocks of about this many bytes
CHUNK = 256             # cells per chunk of the device's reductions: block widths are multiples of it
STAGES = ("upload", "kernels", "run_wall")
FIELDS = ("mean", "total", "tech", "bio")


def chunk():
    """Cells per chunk of the reductions (bmx_dev_get "genevar_chunk"; needs no device)."""
    return _lib.dev_get("genevar_chunk")


def gene_tile():
    """Genes a workgroup of the sparse handle's kernel owns (bmx_dev_get "genevar_gene_tile"; needs no device)."""
    return _lib.dev_get("genevar_gene_tile")


@dataclass
class GeneVarTable:
    """What modelGeneVar() and combineVar() return: scran's DataFrame, column by column, a value per gene."""
    mean: np.ndarray
    total: np.ndarray
    tech: Optional[np.ndarray] = None            # the trend at `mean`; None without `trend_fit`
    bio: Optional[np.ndarray] = None             # total - tech; None without `trend_fit`
    per_block: Optional[List["GeneVarTable"]] = None  # the tables that were combined
    n_cells: int = 0                             # cells behind the statistics (combined: of all tables that count)
    gene_index: Optional[np.ndarray] = None      # 1-based row of the input behind every value
    stats: Optional[dict] = None                 # "stage_ms": see STAGES


class _GeneVarHandle(ResidentHandle):
    """bmx_genevar_t: dense batches stream through two block buffers."""
    PREFIX = "bmx_genevar"
    STAGES = STAGES

    def add_batch(self, x, block_bytes=None):
        """x: genes x cells.  The block widths are whole chunks (the library refuses others): every blocking gives the
        bits of a whole upload."""
        bb = BLOCK_BYTES if block_bytes is None else block_bytes
        per = max(1, int(bb) // (8 * self.G))
        per = max(CHUNK, per // CHUNK * CHUNK)
        self._upload(x, per * 8 * self.G)

    def run(self):
        B = len(self.ncells)
        mean = np.empty((self.G, B), dtype=np.float64, order="F")
        total = np.empty((self.G, B), dtype=np.float64, order="F")
        self._call("run", _lib.f64p(mean), _lib.f64p(total))
        return mean, total


class _SparseGeneVarHandle(_GeneVarHandle):
    """bmx_genevar_sparse_t: the same for canonical CSC batches."""
    PREFIX = "bmx_genevar_sparse"

    def add_batch(self, c, block_bytes=None):
        """c: canonical CSC, genes x cells.  The blocks are whole chunks of cells, as many as hold about block_bytes of
        stored entries at the batch's mean density."""
        per = csc_block_width(c, BLOCK_BYTES if block_bytes is None else block_bytes)
        per = max(CHUNK, per // CHUNK * CHUNK)
        self._upload_csc(c, per)


def device_statistics(mats, device=0, block_bytes=None):
    """The device's part: `mats` genes x cells matrices with the same rows, all dense or all canonical CSC.  Returns mean
    and total, [genes x batches] each (a batch of one cell has total NaN), and the stage times."""
    _lib.require_gpu()
    sparse = sp.issparse(mats[0])
    h = (_SparseGeneVarHandle if sparse else _GeneVarHandle)(mats[0].shape[0], device)
    try:
        for m in mats:
            h.add_batch(m, block_bytes)
        mean, total = h.run()
        return mean, total, h.stage_ms()
    finally:
        h.close()


def _table(mean, total, n_cells, trend_fit, gene_index, stats=None):
    tech = bio = None
    if trend_fit is not None:
        if n_cells < 2:
            tech = np.full(mean.shape, np.nan)
        else:
            tech = np.asarray(trend_fit(mean, total)(mean), dtype=np.float64)
            if tech.shape != mean.shape:
                raise ValueError("the fitted trend must return one value per gene")
        bio = total - tech
    return GeneVarTable(mean=mean, total=total, tech=tech, bio=bio, n_cells=int(n_cells), gene_index=gene_index,
                        stats=stats)


def combineVar(*tables, equiweight=True) -> GeneVarTable:
    """scran::combineVar(...) as assumed here: per gene, every field of FIELDS is averaged over the tables -- unweighted,
    or weighted by `n_cells` with equiweight=False.  Tables with fewer than two cells have no variance and are left out
    (all such: every field is NaN).  A field is None when any table lacks it.  `per_block` holds the inputs."""
    if len(tables) == 1 and isinstance(tables[0], (list, tuple)):
        tables = tuple(tables[0])
    if len(tables) == 0:
        raise ValueError("at least one table must be supplied")
    G = tables[0].mean.shape[0]
    for t in tables:
        if t.mean.shape[0] != G:
            raise ValueError("tables to combine must have the same number of genes")
    valid = [t for t in tables if t.n_cells >= 2]
    out = {}
    for f in FIELDS:
        if any(getattr(t, f) is None for t in tables):
            out[f] = None
        elif not valid:
            out[f] = np.full(G, np.nan)
        elif len(valid) == 1:   # (the average of one table is that table: no w v / w rounding)
            out[f] = np.array(getattr(valid[0], f), dtype=np.float64)
        else:
            acc, wsum = np.zeros(G), 0.0
            for t in valid:     # in the order given
                w = 1.0 if equiweight else float(t.n_cells)
                acc += w * getattr(t, f)
                wsum += w
            out[f] = acc / wsum
    return GeneVarTable(mean=out["mean"], total=out["total"], tech=out["tech"], bio=out["bio"], per_block=list(tables),
                        n_cells=sum(t.n_cells for t in valid), gene_index=tables[0].gene_index)


def getTopHVGs(table, var_field=None, n=None, prop=None, var_threshold=0):
    """scran::getTopHVGs(stats, var.field=, n=, prop=, var.threshold=) as assumed here.  var_field defaults to "bio" when
    the table has it, else "total".  The genes whose value is greater than var_threshold are kept (None: every gene that
    is not NaN; NaN is never kept) and ordered by decreasing value, ties by ascending index; with `n` and / or `prop` the
    first max(n, round(prop * number of genes)) of them remain.  Returns 1-based indices into the rows the table was
    computed from (`gene_index`)."""
    if var_field is None:
        var_field = "bio" if table.bio is not None else "total"
    if var_field not in FIELDS or getattr(table, var_field) is None:
        raise ValueError(f"the table has no field '{var_field}'")
    v = np.asarray(getattr(table, var_field), dtype=np.float64)
    keep = ~np.isnan(v)
    if var_threshold is not None:
        keep &= np.greater(v, float(var_threshold), where=keep, out=np.zeros(v.shape, dtype=bool))
    idx = np.flatnonzero(keep)
    idx = idx[np.argsort(-v[idx], kind="stable")]  # (stable: ties stay in ascending index)
    if n is not None or prop is not None:
        top = 0
        if n is not None:
            top = max(top, int(n))
        if prop is not None:
            top = max(top, int(round(float(prop) * v.size)))
        idx = idx[:top]
    gene_index = np.arange(1, v.size + 1) if table.gene_index is None else np.asarray(table.gene_index)
    return gene_index[idx].astype(np.int64)


def _prepare(x, who):
    """x as a dense matrix or as canonical CSC."""
    if sp.issparse(x):
        return canonical_csc(x)[0]
    return _as_matrices((x,), who)[0]


def modelGeneVar(x, block=None, subset_row=None, trend_fit: Optional[Callable] = None, equiweight=True, device=0,
                 block_bytes=None) -> GeneVarTable:
    """scran::modelGeneVar(x, block=, subset.row=, equiweight=) as assumed here, without p-values.  x: genes x cells of
    log-values, dense or scipy.sparse (kept CSC on the device).  Per gene `mean` and `total`, the sample variance.
    `block`: one label per cell; the levels (sorted) are modelled on their own in one device call and combined by
    combineVar over those with at least two cells.  `subset_row` (1-based integers or a mask): only these rows go to the
    device, `gene_index` names them.  `trend_fit` stands in for scran::fitTrendVar: a callable (mean, total) ->
    callable(mean) -> trend, fitted per block; tech = trend(mean), bio = total - tech; without it both are None."""
    m = _prepare(x, "modelGeneVar")
    if m.ndim != 2:
        raise ValueError("'x' must be a genes x cells matrix")
    if trend_fit is not None and not callable(trend_fit):
        raise ValueError("'trend_fit' must be callable")
    G, n = m.shape
    sub = subset_index(subset_row, G)
    if sub is not None and sub.size == 0:
        raise ValueError("'subset_row' selects no genes")
    if G == 0:
        raise ValueError("'x' has no genes")
    gene_index = np.arange(1, G + 1) if sub is None else sub.astype(np.int64)
    if sub is not None:
        m = m[sub - 1]
    if block is None:
        if n < 2:
            raise ValueError("need at least two cells to compute a variance")
        parts = [m]
    else:
        parts = divide_into_batches(m, _check_batch(block, n)).parts
        if not any(p.shape[1] >= 2 for p in parts):
            raise ValueError("no block has at least two cells")
    if sp.issparse(m):
        parts = [canonical_csc(p)[0] for p in parts]
    mean, total, stage_ms = device_statistics(parts, device, block_bytes)
    stats = {"stage_ms": stage_ms}
    tables = [_table(np.ascontiguousarray(mean[:, i]), np.ascontiguousarray(total[:, i]), p.shape[1], trend_fit,
                     gene_index, stats) for i, p in enumerate(parts)]
    if block is None:
        return tables[0]
    out = combineVar(*tables, equiweight=equiweight)
    out.stats = stats
    return out
