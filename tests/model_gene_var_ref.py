"""What batchelor_amd.model_gene_var is taken to compute, restated in numpy's long double, the allowances its device results
are held to, and the data of the quickCorrect tests.  Nothing here needs the library or a device.

The statements about scran (assumptions, as in the module under test):
  mean_var      per gene the mean over the cells and the sample variance, sum((x - mean)^2) / (n - 1); NaN for one cell
  combine_var   per gene the average of a field over the tables with at least two cells, unweighted or weighted by cells
  top_hvgs      the genes whose value is > threshold (None: not NaN), by decreasing value, ties by ascending index, the
                first max(n, round(prop * genes)); 1-based through gene_index

The allowances.  u = 2^-53, gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, 3.1), n
cells, K = ceil(n / 256) chunks.  They follow from the lengths of the device's sums and are not fitted to its results; the
long-double restatement's own error (u_L = 2^-64 in sums of n terms) is below u / 1000 for the n used and is not counted.

  mean    A chunk's sum adds at most 256 terms one after the other (gamma_255 on sum |x|) and is divided once.  A merge,
          m = mA + (delta * nB) / n, rounds four times; every rounded quantity is bounded by chunk means, which enter the
          result with their share of the cells, so each merge adds at most 4 u mean(|x|).  With K - 1 merges:
              |mean - exact| <= gamma_(256 + 4 K) * mean(|x|).
  total   M2 = sum (x - m)^2 is a sum of non-negative terms, so every rounding is RELATIVE to M2: per chunk the
          subtraction, the square and the 255 additions (258), per merge seven more in (M2A + M2B) + delta^2 nA nB / n;
          the sparse kernel's zeros * m * m adds three:  gamma_(262 + 7 K) * M2.
          The means' errors enter too.  Inside a chunk, deviations from a mean that is off by e give M2 + cnt e^2: second
          order.  Between chunks the merge uses delta = mB - mA of two COMPUTED means, off by at most
              E = 2 gamma_(256 + 4 K) max|x|      (a chunk's mean is only bounded by the largest value, not by mean|x|),
          and delta enters as w delta^2 with w = nA nB / n <= nB:  w (2 |delta| E + E^2), FIRST order in E.  (The issue
          this module was written for names only a second-order term; the host check of the merge arithmetic,
          csrc/gene_var_host_check.cpp, met the first-order one at 5000 cells of 1e6 + N(0, 1).)  Over the merges,
          sum w delta^2 <= M2 (a between-chunk sum of squares) and sum w <= n, so by Cauchy-Schwarz
          sum w |delta| <= sqrt(M2 n), and with the chunks' own cnt e^2 <= n E^2 / 4:
              |M2 - exact| <= gamma_(262 + 7 K) M2 + 2 sqrt(M2 n) E + 2 n E^2,
          divided by n - 1 for `total`.
The one-pass form sum(x^2) / n - mean^2 loses |x|^2 u instead: `one_pass_total` shows it outside these allowances on
values far from zero.
"""
from __future__ import annotations

import functools

import numpy as np

CHUNK = 256
U = 2.0 ** -53
LD = np.longdouble


def gamma(k):
    return k * U / (1.0 - k * U)


def mean_var(x):
    """x: genes x cells (dense).  Returns (mean, total) in long double."""
    x = np.asarray(x, dtype=np.float64).astype(LD)
    n = x.shape[1]
    mean = x.sum(axis=1) / LD(n)
    if n < 2:
        return mean, np.full(x.shape[0], np.nan, dtype=LD)
    dev = x - mean[:, None]
    return mean, (dev * dev).sum(axis=1) / LD(n - 1)


def allowances(x):
    """(mean allowance, total allowance) per gene for the device's statistics of x (genes x cells, n >= 2)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[1]
    K = -(-n // CHUNK)
    ax = np.abs(x)
    g_mean = gamma(256 + 4 * K)
    mean_allow = g_mean * ax.mean(axis=1)
    E = 2.0 * g_mean * ax.max(axis=1)
    mean, total = mean_var(x)
    m2 = (total * LD(n - 1)).astype(np.float64)
    total_allow = (gamma(262 + 7 * K) * m2 + 2.0 * np.sqrt(m2 * n) * E + 2.0 * n * E * E) / (n - 1)
    return mean_allow, total_allow


def one_pass_total(x):
    """The form the kernels must not use, in float64: (sum x^2 - (sum x)^2 / n) / (n - 1)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[1]
    return ((x * x).sum(axis=1) - x.sum(axis=1) ** 2 / n) / (n - 1)


def combine_var(fields, n_cells, equiweight=True):
    """fields: one array per table.  The average over the tables with at least two cells; NaN if there is none."""
    valid = [i for i, c in enumerate(n_cells) if c >= 2]
    if not valid:
        return np.full(np.asarray(fields[0]).shape, np.nan, dtype=LD)
    w = [LD(1) if equiweight else LD(n_cells[i]) for i in valid]
    acc = sum(wi * np.asarray(fields[i]).astype(LD) for wi, i in zip(w, valid))
    return acc / sum(w)


def top_hvgs(values, n=None, prop=None, var_threshold=0, gene_index=None):
    v = np.asarray(values, dtype=np.float64)
    cand = [i for i in range(v.size) if not np.isnan(v[i]) and (var_threshold is None or v[i] > var_threshold)]
    cand.sort(key=lambda i: (-v[i], i))
    if n is not None or prop is not None:
        counts = ([] if n is None else [int(n)]) + ([] if prop is None else [int(round(prop * v.size))])
        cand = cand[:max(counts)]
    gi = np.arange(1, v.size + 1) if gene_index is None else np.asarray(gene_index)
    return gi[np.asarray(cand, dtype=np.int64)].astype(np.int64)


# ------------------------------------------------------------------------------------------ the data of the GPU tests
def gaussian(G, n, seed, offset=0.0, scale=1.0):
    rng = np.random.Generator(np.random.PCG64(7100 + seed))
    return np.asfortranarray(offset + scale * rng.standard_normal((G, n)))


def sparse_case(G, n, seed, empty_cell=False, density=0.2):
    """A dense genes x cells matrix with the shapes the CSC kernel can go wrong on, and the mask of its stored positions:
    gene 0 empty, explicit zeros, and the last gene stored in every cell -- or, with empty_cell, cell 1 without an entry."""
    rng = np.random.Generator(np.random.PCG64(7300 + seed + 1000 * empty_cell))
    stored = rng.random((G, n)) < density
    x = np.where(stored, rng.standard_normal((G, n)) + 2.0, 0.0)
    x[stored & (rng.random((G, n)) < 0.1)] = 0.0   # stored, but zero
    stored[0, :] = False
    if empty_cell:
        stored[:, 1] = False
    else:
        stored[G - 1, :] = True
        x[G - 1, :] = np.where(x[G - 1, :] == 0.0, 1.5, x[G - 1, :])
        x[G - 1, n - 1] = 0.0   # a stored zero in the full gene
    x[~stored] = 0.0
    return np.asfortranarray(x), stored


def to_csc(x, stored):
    """The CSC matrix with exactly the entries of `stored` (explicit zeros kept)."""
    import scipy.sparse as sp
    G, n = x.shape
    indptr = np.concatenate([[0], np.cumsum(stored.sum(axis=0))]).astype(np.int64)
    rows, cols = np.nonzero(stored.T)[1], np.nonzero(stored.T)[0]
    m = sp.csc_matrix((x[rows, cols], rows.astype(np.int32), indptr), shape=(G, n))
    assert m.has_sorted_indices
    return m


QUICK_SEED = 1
QUICK_SIZES = (300, 260)
QUICK_GENES = 400
QUICK_N = 150


@functools.lru_cache(maxsize=None)
def quick_counts(seed=QUICK_SEED):
    """Two count batches from a low-rank plus Poisson model with a planted batch shift: genes x cells."""
    rng = np.random.Generator(np.random.PCG64(7500 + seed))
    G, rank = QUICK_GENES, 4
    load = rng.standard_normal((G, rank)) * (rng.random((G, 1)) < 0.5)   # half the genes carry structure
    base = rng.normal(1.0, 0.8, size=(G, 1))
    shift = 0.7 * rng.standard_normal((G, 1)) * (rng.random((G, 1)) < 0.3)
    out = []
    for b, n in enumerate(QUICK_SIZES):
        z = rng.standard_normal((rank, n))
        depth = rng.uniform(0.6, 1.6, size=(1, n))
        rate = np.exp(base + 0.6 * load @ z + b * shift) * depth
        out.append(np.asfortranarray(rng.poisson(rate).astype(np.float64)))
    for m in out:
        m.setflags(write=False)
    return tuple(out)


def quick_choice(logcounts, n=QUICK_N):
    """The restatement's quickCorrect without a trend for a list of log-value batches: per-batch variances, their
    unweighted average, the top n.  Returns (hvgs, combined total, the gap between the n-th and (n + 1)-th value, the
    largest allowance of the combined total)."""
    totals, allows = [], []
    for m in logcounts:
        totals.append(mean_var(m)[1])
        allows.append(allowances(m)[1])
    comb = combine_var(totals, [m.shape[1] for m in logcounts]).astype(np.float64)
    allow = np.max(np.mean(allows, axis=0)) + 4 * U * np.max(comb)   # (the average's own roundings)
    order = np.sort(comb)[::-1]
    return top_hvgs(comb, n=n), comb, float(order[n - 1] - order[n]), float(allow)
