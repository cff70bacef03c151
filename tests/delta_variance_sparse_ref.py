"""CPU restatement of the sparse mnnDeltaVariance() algorithm (csrc/delta_variance.hip, DeltaSparse) in float64 numpy: the
order of operations of the device, not of R.  A helper module of the sparse delta-variance tests (not a conftest); it
imports nothing from the package under test.

Batches are scipy.sparse CSC, genes x cells, canonical (rows ascending, no duplicates; stored zeros are entries); pairs are
1-based columns of the batches side by side.  Per merge step the pairs are cut into chunks of `chunk` at fixed positions:
  pass 1  per chunk and gene, s_l x_left and s_r x_right are added in pair order over the STORED entries only;
          the chunk sums are added in ascending order; mean = (sum_l / P + sum_r / P) / 2, mdelta = sum_l / P - sum_r / P.
  pass 2  per chunk and gene, for every pair in order where at least one of the two cells stores the gene,
          ((s_l x_l - s_r x_r) - mdelta)^2 is added (a cell that stores nothing there counts as 0) and the pair counted as
          touched; the chunk's sum is that plus ((pairs in chunk - touched) * mdelta) * mdelta; the chunk sums are added
          in ascending order and divided by P - 1.
With cos_norm, s = 1 / max(1e-8, l2 / ml2), l2 a cell's norm over its stored entries in the norm genes.

`fault` plants a mistake, for the tests that show the bounds can be left: "no-zero-term" drops the implicit-zero term,
"squared-separately" squares a gene's left and right entry on their own."""
from __future__ import annotations

import numpy as np


def dense_and_pattern(c):
    """A CSC batch as (values with 0 where nothing is stored, whether an entry is stored)."""
    c = c.tocsc()
    x = np.zeros(c.shape, dtype=np.float64)
    stored = np.zeros(c.shape, dtype=bool)
    cols = np.repeat(np.arange(c.shape[1]), np.diff(c.indptr))
    x[c.indices, cols] = c.data
    stored[c.indices, cols] = True
    return x, stored


def scales(xs, storeds, norm_rows0=None):
    """1 / pmax(1e-8, l2 / ml2) per cell of the batches side by side; norm_rows0: 0-based rows (a row named twice counts
    twice), None = all."""
    l2 = []
    for x, st in zip(xs, storeds):
        v = np.where(st, x, 0.0)
        if norm_rows0 is not None:
            v = v[np.asarray(norm_rows0, dtype=np.int64)]
        l2.append(np.sqrt((v * v).sum(axis=0)))
    ml2 = np.mean([v.mean() for v in l2])
    return np.concatenate([1.0 / np.maximum(1e-8, v / ml2) for v in l2])


def sparse_delta_variance(batches, pairs, chunk, cos_norm=False, subset_row=None, compute_all=False, fault=None):
    """Per step a dict with "mean" and "total" (NaN below one / two pairs), as the device leaves them."""
    parts = [dense_and_pattern(b) for b in batches]
    xs, sts = [p[0] for p in parts], [p[1] for p in parts]
    norm_rows0 = None
    if subset_row is not None:
        rows0 = np.asarray(subset_row, dtype=np.int64) - 1
        if compute_all:
            norm_rows0 = rows0
        else:
            xs, sts = [x[rows0] for x in xs], [s[rows0] for s in sts]
    x, st = np.concatenate(xs, axis=1), np.concatenate(sts, axis=1)
    G = x.shape[0]
    s = scales(xs, sts, norm_rows0) if cos_norm else np.ones(x.shape[1])
    out = []
    for left, right in pairs:
        l, r = np.asarray(left, dtype=np.int64) - 1, np.asarray(right, dtype=np.int64) - 1
        P = len(l)
        edges = list(range(0, P, chunk))
        sum_l, sum_r = np.zeros(G), np.zeros(G)
        for b in edges:
            pl, pr = np.zeros(G), np.zeros(G)
            for p in range(b, min(P, b + chunk)):
                pl += np.where(st[:, l[p]], s[l[p]] * x[:, l[p]], 0.0)
                pr += np.where(st[:, r[p]], s[r[p]] * x[:, r[p]], 0.0)
            sum_l += pl
            sum_r += pr
        with np.errstate(invalid="ignore", divide="ignore"):
            ml, mr = sum_l / np.float64(P), sum_r / np.float64(P)
        mean, md = (ml + mr) / 2.0, ml - mr
        total = np.zeros(G)
        for b in edges:
            e = min(P, b + chunk)
            sq, touched = np.zeros(G), np.zeros(G)
            for p in range(b, e):
                sl_, sr_ = st[:, l[p]], st[:, r[p]]
                vl = np.where(sl_, s[l[p]] * x[:, l[p]], 0.0)
                vr = np.where(sr_, s[r[p]] * x[:, r[p]], 0.0)
                if fault == "squared-separately":
                    sq += np.where(sl_, (vl - md) ** 2, 0.0) + np.where(sr_, ((0.0 - vr) - md) ** 2, 0.0)
                    touched += sl_.astype(np.float64) + sr_.astype(np.float64)
                    continue
                any_ = sl_ | sr_
                d = (vl - vr) - md
                sq += np.where(any_, d * d, 0.0)
                touched += any_
            zero_term = 0.0 if fault == "no-zero-term" else (((e - b) - touched) * md) * md
            total += sq + zero_term
        total = total / (P - 1) if P >= 2 else np.full(G, np.nan)
        if P < 1:
            mean = np.full(G, np.nan)
        out.append({"mean": mean, "total": total})
    return out
