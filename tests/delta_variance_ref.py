"""CPU restatement of mnnDeltaVariance() (R/mnnDeltaVariance.R:95-201) in numpy, written from the R text.  A helper module
of the delta-variance tests (not a conftest); it imports nothing from the package under test.  Batches are genes x cells,
indices 1-based, None = NULL.  Everything is computed in float64, or in numpy.longdouble with `longdouble=True` (what the
tests take their error bounds from)."""
from __future__ import annotations

import warnings

import numpy as np

FIELDS = ("mean", "total", "trend", "adjusted")


def _index(r):
    return None if r is None else np.asarray(r, dtype=np.int64) - 1


def cosine_l2(x, subset_row=None):
    """cosineNorm(x, mode="l2norm", subset.row=) (R/cosineNorm.R:53-68): sqrt(colSums(x[subset.row, ]^2))."""
    if subset_row is not None:
        x = x[_index(subset_row)]
    return np.sqrt((x * x).sum(axis=0))


def apply_cosine_norm(x, l2):
    """.apply_cosine_norm (R/cosineNorm.R:79-82): columns over pmax(1e-8, l2)."""
    return x / np.maximum(x.dtype.type(1e-8), l2)[None, :]


def prepare(batches, pairs, cos_norm=False, subset_row=None, compute_all=False, longdouble=False):
    """:110-142: the common matrix restricted to the cells in pairs, the pairs re-indexed into it, and the subset that is
    still in force (None unless compute.all).  `pairs`: a list of (left, right)."""
    dt = np.longdouble if longdouble else np.float64
    x = [np.asarray(b, dtype=dt) for b in batches]
    if subset_row is not None:                                                          # :113-119
        if not compute_all:
            x = [y[_index(subset_row)] for y in x]
            subset_row = None
    if cos_norm:                                                                        # :121-126
        l2 = [cosine_l2(y, subset_row) for y in x]
        ml2 = np.mean(np.asarray([v.mean() for v in l2], dtype=dt))
        l2 = [v / ml2 for v in l2]
        x = [apply_cosine_norm(y, v) for y, v in zip(x, l2)]
    x = np.concatenate(x, axis=1)                                                       # :128
    cols = [np.asarray(v, dtype=np.int64) for p in pairs for v in p]                    # :135-137
    universe = np.unique(np.concatenate(cols)) if cols else np.zeros(0, dtype=np.int64)
    x = x[:, universe - 1]
    remapped = [(np.searchsorted(universe, np.asarray(l, dtype=np.int64)) + 1,          # :139-142 (match)
                 np.searchsorted(universe, np.asarray(r, dtype=np.int64)) + 1) for l, r in pairs]
    return x, remapped, subset_row


def compute_mnn_variance(block, pairs):
    """.compute_mnn_variance (:189-201): per step rowVars(b1 - b2) -- the mean of the deltas first, then the centred
    squares over P - 1 -- and (rowMeans(b1) + rowMeans(b2)) / 2."""
    all_vars, all_means = [], []
    nan = block.dtype.type(np.nan)
    for left, right in pairs:
        b1, b2 = block[:, _index(left)], block[:, _index(right)]                        # :194-195
        P = b1.shape[1]
        delta = b1 - b2
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)                             # (no pairs: NaN, as in R)
            if P >= 2:
                centre = delta.mean(axis=1)
                all_vars.append(((delta - centre[:, None]) ** 2).sum(axis=1) / (P - 1))  # :196
            else:
                all_vars.append(np.full(block.shape[0], nan))                           # rowVars of one column is NA
            if P >= 1:
                all_means.append((b1.mean(axis=1) + b2.mean(axis=1)) / 2)               # :197
            else:
                all_means.append(np.full(block.shape[0], nan))
    return all_vars, all_means


def combine_blocks(tables, npairs):
    """scran::combineBlocks(ave.fields=, geometric=FALSE, equiweight=FALSE, weights=npairs, valid=npairs >= 2) (:167-172):
    the weighted mean of every field over the valid steps; NaN without one."""
    npairs = np.asarray(npairs, dtype=np.int64)
    valid = [i for i in range(len(tables)) if npairs[i] >= 2]
    out = {}
    for f in FIELDS:
        if tables[0].get(f) is None:
            out[f] = None
        elif not valid:
            out[f] = np.full_like(tables[0][f], np.nan)
        else:
            w = npairs[valid].astype(tables[0][f].dtype)
            out[f] = sum(wi * tables[i][f] for wi, i in zip(w, valid)) / w.sum()
    return out


def mnn_delta_variance(batches, pairs, cos_norm=False, subset_row=None, compute_all=False, trend_fit=None,
                       longdouble=False):
    """mnnDeltaVariance() (:95-183).  `pairs`: a (left, right) pair or a list of them.  `trend_fit` stands in for
    scran::fitTrendVar: (mean, total) -> callable(mean) -> trend; None leaves trend and adjusted out.  Returns a dict with
    the combined fields, "per_step" (a list of dicts, always) and "npairs"."""
    if len(pairs) == 2 and np.ndim(pairs[0]) == 1 and np.ndim(pairs[1]) == 1:           # :131-133
        pairs = [pairs]
    x, remapped, subset_row = prepare(batches, pairs, cos_norm, subset_row, compute_all, longdouble)
    xvar, xmean = compute_mnn_variance(x, remapped)                                     # :145
    npairs = [len(l) for l, _ in pairs]                                                 # :167
    tables = []
    for i in range(len(pairs)):                                                         # :148-165
        t = {"mean": xmean[i], "total": xvar[i], "trend": None, "adjusted": None}
        if trend_fit is not None:
            if npairs[i] >= 2:
                sel = slice(None) if subset_row is None else _index(subset_row)         # :155-157
                t["trend"] = np.asarray(trend_fit(xmean[i][sel], xvar[i][sel])(xmean[i]))
            else:
                t["trend"] = np.full_like(xmean[i], np.nan)
            t["adjusted"] = t["total"] - t["trend"]                                     # :162
        tables.append(t)
    out = combine_blocks(tables, npairs)
    out["per_step"] = tables
    out["npairs"] = np.asarray(npairs, dtype=np.int64)
    return out


def literal(batches, pairs, cos_norm=False, subset_row=None, compute_all=False):
    """The same numbers by a per-gene, per-pair Python loop over the concatenated matrix, no universe and no vector
    arithmetic: what the restatement is checked against."""
    x = [np.asarray(b, dtype=np.float64) for b in batches]
    if subset_row is not None and not compute_all:
        x = [y[_index(subset_row)] for y in x]
        subset_row = None
    if cos_norm:
        rows = range(x[0].shape[0]) if subset_row is None else [int(g) - 1 for g in subset_row]
        l2 = [[float(np.sqrt(sum(y[g, c] * y[g, c] for g in rows))) for c in range(y.shape[1])] for y in x]
        ml2 = sum(sum(v) / len(v) for v in l2) / len(l2)
        x = [np.stack([y[:, c] / max(1e-8, v[c] / ml2) for c in range(y.shape[1])], axis=1) for y, v in zip(x, l2)]
    x = np.concatenate(x, axis=1)
    G = x.shape[0]
    out = []
    for left, right in pairs:
        P = len(left)
        mean, total = np.full(G, np.nan), np.full(G, np.nan)
        for g in range(G):
            if P >= 1:
                sl = sum(x[g, int(l) - 1] for l in left)
                sr = sum(x[g, int(r) - 1] for r in right)
                mean[g] = (sl / P + sr / P) / 2
            if P >= 2:
                d = [x[g, int(l) - 1] - x[g, int(r) - 1] for l, r in zip(left, right)]
                m = sum(d) / P
                total[g] = sum((v - m) ** 2 for v in d) / (P - 1)
        out.append({"mean": mean, "total": total})
    return out
