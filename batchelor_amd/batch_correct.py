"""The workflow layer of the reference: batchCorrect() with its *Param classes (R/batchCorrect.R:65-98,
R/BatchelorParam.R), noCorrect() (R/noCorrect.R:45-76), intersectRows() (R/intersectRows.R:53-80) and quickCorrect()
(R/quickCorrect.R:66-120), which chains intersectRows, multiBatchNorm, per-batch variance modelling, the choice of
highly variable genes and batchCorrect.

Everything here is host-side dispatch; the device work is in the functions that are called.  Matrices have no row names,
so the functions that need them (intersectRows, quickCorrect) take `row_names`, one sequence of strings per batch.

Stated deviation: scran's trend is not re-implemented (model_gene_var.py), so without a `trend_fit` in model_var_args
quickCorrect ranks the genes by `total`, which is getTopHVGs(var.field="total").

Out of scope: SingleCellExperiment inputs, hence `assay.type`, correctExperiments, applyMultiSCE and convertPCsToSCE;
handing the rows chosen to the PCA handle device to device (the log-values go back to the host between the steps).
"""
from __future__ import annotations

import inspect
from dataclasses import dataclass
from typing import Optional

import numpy as np
import scipy.sparse as sp

from .fast_mnn import fastMNN
from .inputs import all_sparse, check_same_dim, check_same_rows, check_unique_names, subset_index, unpack_batches
from .linear_correct import _as_matrices, _check_batch, regressBatches, rescaleBatches
from .mnn_correct import mnnCorrect
from .model_gene_var import GeneVarTable, combineVar, getTopHVGs, modelGeneVar
from .multi_batch_norm import multiBatchNorm

# what batchCorrect() itself hands to the target: not a PARAM's to set
_DISPATCH_ARGS = ("batches", "batch", "restrict", "subset_row", "correct_all", "names", "device")
MODEL_VAR_ARGS = ("trend_fit", "equiweight")


@dataclass
class NoCorrectResult:
    """What noCorrect() returns: the `merged` assay and the `batch` column of the reference's SingleCellExperiment."""
    corrected: object    # genes x cells: column-major dense, or CSC when the batches were sparse
    batch: np.ndarray    # per cell its batch: 1-based id, name, or the caller's `batch`


def noCorrect(*batches, batch=None, subset_row=None, correct_all=False, names=None) -> NoCorrectResult:
    """noCorrect(..., batch=, subset.row=, correct.all=) (R/noCorrect.R:45-76): the batches side by side, uncorrected; the
    rows of subset_row only, unless correct_all.  One object keeps its own `batch`.  `names` plays the role of the
    argument names of `...`.  Host only."""
    mats = unpack_batches(batches)
    if len(mats) == 0:
        raise ValueError("at least one batch must be specified")
    sparse = all_sparse(mats, "noCorrect")
    if sparse:
        mats = [m.tocsc() for m in mats]
        G = check_same_rows(mats)
    else:
        mats = _as_matrices(mats, "noCorrect")
        G = check_same_dim(mats, byrow=False)
    sub = subset_index(subset_row, G)
    if not correct_all and sub is not None:
        mats = [m[sub - 1] for m in mats]  # :55-59
    if len(mats) == 1:
        if batch is None:
            raise ValueError("'batch' must be specified if '...' has only one object")  # R/divideIntoBatches.R:88
        labels = _check_batch(batch, mats[0].shape[1])
        out = mats[0]
    else:
        labels = np.repeat(np.arange(1, len(mats) + 1), [m.shape[1] for m in mats])
        if names is not None:
            names = [str(v) for v in names]
            if len(names) != len(mats):
                raise ValueError("'names' must have one entry per batch")
            check_unique_names(names)  # :68-70
            labels = np.asarray(names)[labels - 1]
        out = sp.hstack(mats, format="csc") if sparse else np.concatenate(mats, axis=1)
    out = sp.csc_matrix(out) if sparse else np.asfortranarray(out, dtype=np.float64)
    return NoCorrectResult(corrected=out, batch=labels)


class BatchelorParam:
    """A holder of keyword arguments for one correction function: as.list(PARAM) is `self.args`.  A name the function does
    not take, or one that batchCorrect() sets itself, is refused at construction."""
    TARGET = None

    def __init__(self, **kwargs):
        target = type(self).TARGET
        known = [p for p in inspect.signature(target).parameters if p not in _DISPATCH_ARGS]
        for key in kwargs:
            if key in _DISPATCH_ARGS:
                raise ValueError(f"'{key}' is an argument of batchCorrect(), not of {type(self).__name__}")
            if key not in known:
                raise ValueError(f"{target.__name__}() takes no argument '{key}' (it takes {', '.join(known) or 'none'})")
        self.args = dict(kwargs)

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{k}={v!r}' for k, v in self.args.items())})"


class FastMnnParam(BatchelorParam):
    """FastMnnParam(...): batchCorrect() calls fastMNN()."""
    TARGET = staticmethod(fastMNN)


class ClassicMnnParam(BatchelorParam):
    """ClassicMnnParam(...): batchCorrect() calls mnnCorrect()."""
    TARGET = staticmethod(mnnCorrect)


class RescaleParam(BatchelorParam):
    """RescaleParam(...): batchCorrect() calls rescaleBatches()."""
    TARGET = staticmethod(rescaleBatches)


class RegressParam(BatchelorParam):
    """RegressParam(...): batchCorrect() calls regressBatches()."""
    TARGET = staticmethod(regressBatches)


class NoCorrectParam(BatchelorParam):
    """NoCorrectParam(): batchCorrect() calls noCorrect()."""
    TARGET = staticmethod(noCorrect)


def batchCorrect(*batches, batch=None, restrict=None, subset_row=None, correct_all=False, PARAM, names=None, device=0):
    """batchCorrect(..., batch=, restrict=, subset.row=, correct.all=, PARAM=) (R/batchCorrect.R:65-98): the function PARAM
    stands for, called with these arguments and PARAM's own; returns what it returns.  NoCorrectParam drops `restrict`
    (:96), and noCorrect runs on the host, so `device` is dropped with it.  RegressParam(d=50, deferred=True, residuals=False)
    returns the PCs of the residuals without forming them (regressBatches)."""
    if not isinstance(PARAM, (FastMnnParam, ClassicMnnParam, RescaleParam, RegressParam, NoCorrectParam)):
        raise TypeError("'PARAM' must be a FastMnnParam, ClassicMnnParam, RescaleParam, RegressParam or NoCorrectParam")
    combined = dict(batch=batch, subset_row=subset_row, correct_all=correct_all, names=names)
    if not isinstance(PARAM, NoCorrectParam):
        combined.update(restrict=restrict, device=device)
    combined.update(PARAM.args)
    return type(PARAM).TARGET(*unpack_batches(batches), **combined)


def intersectRows(*batches, row_names, subset_row=None, keep_all=False):
    """intersectRows(..., subset.row=, keep.all=) (R/intersectRows.R:53-80).  row_names: one sequence of strings per batch,
    the names of its rows.  Every batch is cut to the universe -- the names all batches share, in the first batch's order
    -- and then, unless keep_all, to subset_row: names of the universe, or (only when no batch had to be cut) 1-based
    indices or a mask.  Returns (batches, names): the batches and the names of their rows."""
    mats = list(unpack_batches(batches))
    if len(mats) == 0:
        raise ValueError("at least one batch must be specified")
    if row_names is None or len(row_names) != len(mats):
        raise ValueError("'row_names' must hold one sequence of names per batch")
    all_genes = [[str(v) for v in r] for r in row_names]
    for m, r in zip(mats, all_genes):
        if m.shape[0] != len(r):
            raise ValueError("'row_names' must name every row of its batch")
    common = set(all_genes[0]).intersection(*map(set, all_genes[1:]))
    universe, seen = [], set()
    for g in all_genes[0]:   # (intersect() keeps the first argument's order and drops duplicates)
        if g in common and g not in seen:
            universe.append(g)
            seen.add(g)
    if len(universe) == 0:
        raise ValueError("no genes remaining in the intersection")  # :58-60
    non_same = False
    for i, (m, r) in enumerate(zip(mats, all_genes)):
        if r != universe:
            non_same = True
            first = {}
            for j, g in enumerate(r):
                first.setdefault(g, j)
            mats[i] = m[np.asarray([first[g] for g in universe], dtype=np.int64)]
    rows = universe
    if subset_row is not None:
        s = np.asarray(subset_row)
        character = s.dtype.kind in "US" or (s.dtype == object and all(isinstance(v, str) for v in s.tolist()))
        if non_same and not character:
            raise ValueError("only character 'subset.row' is allowed when '...' have different rownames")  # :71-73
        if not keep_all:
            if character:
                at = {g: j for j, g in enumerate(universe)}
                missing = [v for v in s.tolist() if v not in at]
                if missing:
                    raise ValueError("subscript out of bounds: 'subset_row' names rows that are not in the intersection")
                idx = np.asarray([at[v] for v in s.tolist()], dtype=np.int64)
            else:
                idx = subset_index(subset_row, len(universe)).astype(np.int64) - 1
            mats = [m[idx] for m in mats]
            rows = [universe[j] for j in idx]
    return mats, rows


@dataclass
class QuickCorrectResult:
    """What quickCorrect() returns."""
    dec: GeneVarTable            # the variance modelling the genes were chosen by
    hvgs: np.ndarray             # 1-based rows (of the universe) used for the correction
    corrected: object            # what batchCorrect() returned
    universe: Optional[list]     # the row names after intersectRows; None without `row_names`


def quickCorrect(*batches, batch=None, restrict=None, correct_all=True, PARAM=None, multi_norm_args=None,
                 precomputed=None, model_var_args=None, hvg_args=None, row_names=None, names=None,
                 device=0) -> QuickCorrectResult:
    """quickCorrect(..., batch=, restrict=, correct.all=, PARAM=, multi.norm.args=, precomputed=, model.var.args=,
    hvg.args=) (R/quickCorrect.R:66-120).  The batches are genes x cells COUNTS, all dense or all scipy.sparse; one object
    needs `batch=`.  In order: intersectRows (when `row_names` is given), multiBatchNorm(preserve_single=True,
    **multi_norm_args), modelGeneVar per batch and combineVar (one object: modelGeneVar(block=batch)) or the `precomputed`
    tables, one per object; getTopHVGs(**hvg_args), default n=5000; batchCorrect on the log-values with the chosen rows.
    model_var_args: `trend_fit` and `equiweight`.  PARAM defaults to FastMnnParam().

    Sparse counts whose zero stays a zero come out of multiBatchNorm as CSC and go into the sparse variance handle and
    into fastMNN or mnnCorrect (ClassicMnnParam) as they are; where multiBatchNorm returns dense values
    (pseudo_count != 1) the dense path is taken.  What rescaleBatches and regressBatches refuse of sparse input, they
    refuse here.  With PARAM=RegressParam(d=50, deferred=True, residuals=False) the PCs over the chosen rows come from the
    device-resident log-values and no residual of any gene is formed or downloaded (regressBatches)."""
    PARAM = FastMnnParam() if PARAM is None else PARAM
    multi_norm_args = dict(multi_norm_args or {})
    model_var_args = dict(model_var_args or {})
    hvg_args = {"n": 5000} if hvg_args is None else dict(hvg_args)
    for key in model_var_args:
        if key not in MODEL_VAR_ARGS:
            raise ValueError(f"'model_var_args' takes {' and '.join(MODEL_VAR_ARGS)} only, not '{key}'")
    mats = list(unpack_batches(batches))
    if len(mats) == 0:
        raise ValueError("at least one batch must be specified")
    universe = None
    if row_names is not None:
        mats, universe = intersectRows(*mats, row_names=row_names)
    single = len(mats) == 1
    if precomputed is not None:
        precomputed = list(precomputed)
        if len(precomputed) != len(mats):  # :100-102, :105-107
            raise ValueError("'length(precomputed)' is not the same as the number of objects in '...'")
        for t in precomputed:
            if t.mean.shape[0] != mats[0].shape[0]:
                raise ValueError("a 'precomputed' table must have one row per gene of the batches")

    normed = multiBatchNorm(*mats, batch=batch, preserve_single=True, names=names, device=device, **multi_norm_args)
    logcounts = [normed.logcounts] if single else list(normed.logcounts)

    if precomputed is not None:
        dec = precomputed[0] if single else combineVar(*precomputed)
    elif single:
        dec = modelGeneVar(logcounts[0], block=batch, device=device, **model_var_args)
    else:
        fit = {k: v for k, v in model_var_args.items() if k == "trend_fit"}
        dec = combineVar(*[modelGeneVar(m, device=device, **fit) for m in logcounts])
    hvgs = getTopHVGs(dec, **hvg_args)
    corrected = batchCorrect(*logcounts, batch=batch, restrict=restrict, correct_all=correct_all, subset_row=hvgs,
                             PARAM=PARAM, names=names, device=device)
    return QuickCorrectResult(dec=dec, hvgs=hvgs, corrected=corrected, universe=universe)
