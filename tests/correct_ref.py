"""The four row operations of a fastMNN merge step restated in numpy long double, written from the R text the oracle cites:
.center_along_batch_vector (R/fastMNN.R:626-640), .compute_tricube_average (R/utils_tricube.R:1-27) under
.tricube_weighted_correction (R/fastMNN.R:599-608), .average_correction (R/fastMNN.R:567-580) and one term of
.compute_perbatch_var (R/fastMNN.R:651-658).  A helper module of tests/test_cpu_correct_ref.py and
tests/test_gpu_correct_forms.py (not a conftest); it imports nothing from the package under test and holds no kNN: the
tricube average takes its neighbour lists as given.  Every function returns long double; the callers round to double.
R conventions are kept: cells x dims, 1-based indices, None = NULL."""
import math

import numpy as np

LD = np.longdouble


def has_extended_precision():
    """At least the 64-bit mantissa of x87 extended precision (eps 2^-63): 2048 times finer than double."""
    return np.finfo(LD).eps <= 2.0 ** -63


def _ld(a):
    return np.asarray(a, dtype=LD)


def center_along_batch_vector(mat, batch_vec, restrict=None):
    """x + (mean_restrict(x.v^) - x.v^) v^ (R/fastMNN.R:630-639).  A zero batch vector gives 0 / 0 = NaN everywhere."""
    x, v = _ld(mat), _ld(batch_vec)
    with np.errstate(invalid="ignore", divide="ignore"):
        vhat = v / np.sqrt(np.sum(v * v))
        loc = (x * vhat).sum(axis=1)
        central = loc.mean() if restrict is None else loc[np.asarray(restrict, dtype=np.int64) - 1].mean()
        return x + np.outer(central - loc, vhat)


def tricube_average(vals, indices, distances, ndist=3):
    """R/utils_tricube.R:5-20 from GIVEN neighbours: indices [n x k] 1-based into the rows of vals, distances ascending.
    bandwidth = pmax(1e-8, ndist * distance at place ceiling(k / 2)); weights (1 - min(rel, 1)^3)^3 over their row sum; the
    weighted sum in neighbour order.  No neighbours: zeros (:22-23).  A row whose weights are all 0 is 0 / 0 = NaN."""
    vals, dist = _ld(vals), _ld(distances)
    indices = np.asarray(indices, dtype=np.int64)
    n, k = indices.shape
    out = np.zeros((n, vals.shape[1]), dtype=LD)
    if k == 0:
        return out
    middle = int(math.ceil(k / 2))
    bandwidth = np.maximum(LD(1e-8), dist[:, middle - 1] * LD(ndist))
    rel = np.minimum(dist / bandwidth[:, None], LD(1))
    tricube = (1 - rel ** 3) ** 3
    with np.errstate(invalid="ignore", divide="ignore"):
        weight = tricube / tricube.sum(axis=1)[:, None]
        for j in range(k):
            out = out + vals[indices[:, j] - 1] * weight[:, j][:, None]
    return out


def tricube_weighted_correction(curdata, correction, indices, distances, ndist=3):
    """R/fastMNN.R:606-607 with the result of queryKNN(query=curdata, X=curdata[in.mnn,], k=min(k, length(in.mnn))) given."""
    return _ld(curdata) + tricube_average(correction, indices, distances, ndist=ndist)


def average_correction(refdata, mnn1, curdata, mnn2):
    """R/fastMNN.R:571-579: the mean of refdata[l] - curdata[r] over the partners l of every paired right cell r, the right
    cells ascending.  Returns (averaged [U x d], second [U] 1-based)."""
    ref, cur = _ld(refdata), _ld(curdata)
    mnn1 = np.asarray(mnn1, dtype=np.int64)
    mnn2 = np.asarray(mnn2, dtype=np.int64)
    second = np.unique(mnn2)
    out = np.zeros((second.size, cur.shape[1]), dtype=LD)
    for u, r in enumerate(second):
        partners = mnn1[mnn2 == r]
        out[u] = (ref[partners - 1] - cur[r - 1]).sum(axis=0) / LD(partners.size)
    return out, second.astype(np.int32)


def total_variance(data):
    """sum(colVars(data)) (R/fastMNN.R:655), two passes: the column means, then the squared deviations over n - 1.
    One row: 0 / 0 = NaN, as colVars gives NA."""
    x = _ld(data)
    n = x.shape[0]
    dev = x - x.mean(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return ((dev * dev).sum(axis=0) / LD(n - 1)).sum()


def one_pass_variance(data, pivot=None):
    """The one-pass form in DOUBLE, as a device pass accumulates it: sums of t = x - pivot and of t^2 per column, then
    (sum t^2 - (sum t)^2 / n) / (n - 1), summed over the columns.  pivot None: no shift at all.  Only there to show which
    inputs tell a shifted pass from an unshifted one (tests/test_cpu_correct_ref.py)."""
    x = np.asarray(data, dtype=np.float64)
    n = x.shape[0]
    t = x if pivot is None else x - np.asarray(pivot, dtype=np.float64)
    a, b = t.sum(axis=0), (t * t).sum(axis=0)
    return float(((b - a * a / n) / (n - 1)).sum())
