"""CPU restatement of rescaleBatches() (R/rescaleBatches.R:63-150) and regressBatches() (R/regressBatches.R:93-158) in
numpy, written from the R text.  A helper module of the linear-correction tests (not a conftest); it imports nothing from
the package under test.  Batches are genes x cells, indices 1-based, None = NULL."""
from __future__ import annotations

import numpy as np


def _index(r):
    return None if r is None else np.asarray(r, dtype=np.int64) - 1


def unlog(x, log_base, pseudo_count):
    """.unlog, "ANY" method (R/rescaleBatches.R:157-159): log.base^x - pseudo.count."""
    return np.power(float(log_base), x) - pseudo_count


def relog(x, log_base, pseudo_count):
    """.relog (R/rescaleBatches.R:172-174): log(x + pseudo.count, log.base).  R's log(x, base) is log2 for base 2, log10
    for base 10 and log(x) / log(base) otherwise (arithmetic.c, logbase)."""
    v = x + pseudo_count
    if log_base == 2:
        return np.log2(v)
    if log_base == 10:
        return np.log10(v)
    return np.log(v) / np.log(log_base)


def rescale_batches(batches, log_base=2, pseudo_count=1, subset_row=None, restrict=None):
    """.rescale_batches (R/rescaleBatches.R:103-150).  Returns (corrected genes x all cells, averages genes x batches,
    reference)."""
    if len(batches) < 2:
        raise ValueError("at least two batches must be specified")                     # :106-108
    sub = _index(subset_row)
    un = []
    for b in batches:                                                                   # :111-116
        b = np.asarray(b, dtype=np.float64)
        if sub is not None:
            b = b[sub]
        un.append(unlog(b, log_base, pseudo_count))
    averages = []
    for b, cur in enumerate(un):                                                        # :118-125
        r = None if restrict is None else _index(restrict[b])
        averages.append((cur if r is None else cur[:, r]).mean(axis=1))
    reference = np.minimum.reduce(averages)                                             # :128 (pmin)
    out = []
    for cur, ave in zip(un, averages):                                                  # :129-133
        with np.errstate(divide="ignore", invalid="ignore"):
            rescale = reference / ave
        rescale[~np.isfinite(rescale)] = 0.0
        out.append(relog(cur * rescale[:, None], log_base, pseudo_count))
    return np.concatenate(out, axis=1), np.stack(averages, axis=1), reference


def divide_by_column(x, batch, restrict=None):
    """divideIntoBatches(byrow=FALSE) (R/divideIntoBatches.R:36-84)."""
    batch = np.asarray(batch)
    levels = sorted(set(batch.tolist()))
    mask = None
    if restrict is not None:
        mask = np.zeros(x.shape[1], dtype=bool)
        r = np.asarray(restrict)
        if r.dtype == bool:
            mask[:] = r
        else:
            mask[r.astype(np.int64) - 1] = True
    parts, rparts = [], (None if mask is None else [])
    reorder = np.zeros(x.shape[1], dtype=np.int64)
    last = 0
    for lv in levels:
        keep = batch == lv
        parts.append(x[:, keep])
        if mask is not None:
            cr = np.flatnonzero(mask[keep]) + 1
            if cr.size == 0:
                raise ValueError("no cells remaining in a batch after restriction")    # :71-73
            rparts.append(cr)
        n = int(keep.sum())
        reorder[keep] = last + np.arange(1, n + 1)
        last += n
    return parts, rparts, levels, reorder


def rescale(batches, batch=None, restrict=None, log_base=2, pseudo_count=1, subset_row=None, correct_all=False):
    """rescaleBatches() (R/rescaleBatches.R:63-96): corrected genes x cells in the caller's order, and the batch of
    every cell."""
    reorder = None
    if len(batches) == 1:                                                               # :76-81
        x = np.asarray(batches[0], dtype=np.float64)
        batches, restrict, levels, reorder = divide_by_column(x, batch, None if restrict is None else restrict[0])
        labels = np.repeat(np.asarray(levels), [b.shape[1] for b in batches])
    else:
        labels = np.repeat(np.arange(1, len(batches) + 1), [np.asarray(b).shape[1] for b in batches])
    if correct_all:                                                                     # :82-84
        subset_row = None
    out, _, _ = rescale_batches(batches, log_base, pseudo_count, subset_row, restrict)
    if reorder is not None:                                                             # :88-91
        out, labels = out[:, reorder - 1], labels[reorder - 1]
    return out, labels


def residuals(x, design, keep=None, restrict=None, solver="lstsq"):
    """ResidualMatrix(t(x), design, keep=, restrict=), transposed back (man/regressBatches.Rd; the reference's
    tests/testthat/test-regress-batch.R): the coefficients are fitted by least squares on the restricted cells, and the
    columns of the design that are not in `keep` are regressed out of every cell.  x genes x cells, design cells x p.
    solver "qr": an explicit Householder QR solve instead of numpy.linalg.lstsq (the tests measure one against the
    other to size their tolerance)."""
    x = np.asarray(x, dtype=np.float64)
    design = np.asarray(design, dtype=np.float64)
    r = _index(restrict)
    dr = design if r is None else design[r]
    xr = x if r is None else x[:, r]
    if solver == "lstsq":
        coef = np.linalg.lstsq(dr, xr.T, rcond=None)[0].T      # genes x p
    else:
        q, rr = np.linalg.qr(dr)
        coef = np.linalg.solve(rr, q.T @ xr.T).T
    drop = np.ones(design.shape[1], dtype=bool)
    if keep is not None:
        drop[np.asarray(keep, dtype=np.int64) - 1] = False
    return x - coef[:, drop] @ design[:, drop].T, coef


def regress(batches, batch=None, design=None, keep=None, restrict=None, subset_row=None, correct_all=False,
            solver="lstsq"):
    """regressBatches() up to the residuals (R/regressBatches.R:97-151): corrected genes x cells in the caller's order,
    the batch of every cell, the coefficients."""
    batches = [np.asarray(b, dtype=np.float64) for b in batches]
    if len(batches) > 1:                                                                # :110-122
        combined = np.concatenate(batches, axis=1)
        ncells = [b.shape[1] for b in batches]
        labels = np.repeat(np.arange(1, len(batches) + 1), ncells)
        if restrict is not None:
            offs = np.concatenate([[0], np.cumsum(ncells)[:-1]])
            restrict = np.concatenate([(np.arange(1, n + 1) if r is None else np.asarray(r, dtype=np.int64)) + o
                                       for r, n, o in zip(restrict, ncells, offs)])
    elif len(batches) == 1:                                                             # :123-131
        combined = batches[0]
        if batch is None:
            if design is None:
                raise ValueError("'batch' must be specified if '...' has only one object")
            batch = np.ones(combined.shape[1], dtype=np.int64)
        labels = np.asarray(batch)
        if restrict is not None:
            restrict = restrict[0]
            if restrict is not None and np.asarray(restrict).dtype == bool:
                restrict = np.flatnonzero(restrict) + 1
    else:
        raise ValueError("at least two batches must be specified")                     # :133
    if not correct_all and subset_row is not None:                                      # :136-139
        combined = combined[_index(subset_row)]
    if design is None:                                                                  # :141-143 model.matrix(~0 + factor(batch))
        levels = np.asarray(sorted(set(labels.tolist())))
        design = (labels[:, None] == levels[None, :]).astype(np.float64)
    elif np.asarray(design).shape[0] != combined.shape[1]:                              # :144-146
        raise ValueError("'nrow(design)' should be equal to the total number of cells")
    out, coef = residuals(combined, design, keep, restrict, solver)                     # :148-150
    return out, labels, coef
