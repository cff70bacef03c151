"""multiBatchNorm() in plain numpy: R/multiBatchNorm.R:88-280 with scuttle's librarySizeFactors, calculateAverage and
logNormCounts(center.size.factors=FALSE) written out.  The steps are in the order the reference takes them."""
import numpy as np

from batchelor_amd.inputs import divide_into_batches, subset_index, unpack_batches

RATIO_ERROR = "median ratio of averages between batches is not finite"
SF_ERROR = "size factors should be positive"


def batch_statistics(x, sf, sub):
    """.compute_batch_statistics (:226-234): the centred size factors and the averages over the rows of `sub` (0-based)."""
    xs = x if sub is None else x[sub]
    if sf is None:
        lib = xs.sum(axis=0)
        sf = lib / np.mean(lib)
    else:
        sf = np.asarray(sf, dtype=np.float64)
        sf = sf / np.mean(sf)
    if not np.all(np.isfinite(sf) & (sf > 0)):
        raise ValueError(SF_ERROR)
    ave = (1.0 / xs.shape[1]) * (xs / sf).sum(axis=1)
    return sf, ave


def median(v):
    """The middle order statistic, or the mean of the two middle ones; NaN if any value is."""
    if np.isnan(v).any():
        return np.nan
    s = np.sort(v)
    k = s.size
    with np.errstate(invalid="ignore"):
        return s[k // 2] if k % 2 else (s[k // 2 - 1] + s[k // 2]) / 2


def grand_mean(first, second):
    fs, ss = np.sum(first), np.sum(second)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (first / fs + second / ss) / 2 * (fs + ss) / 2


def rescale_size_factors(aves, min_mean):
    """.rescale_size_factors (:237-280): the ratios (B x B), the 0-based reference batch and the rescaling."""
    B = len(aves)
    ratios = np.ones((B, B))
    for first in range(B - 1):
        for second in range(first + 1, B):
            f, s = aves[first], aves[second]
            keep = grand_mean(f, s) >= min_mean
            kf, ks = f[keep], s[keep]
            if kf.size == 0:
                raise ValueError(RATIO_ERROR)
            with np.errstate(divide="ignore", invalid="ignore"):
                r1, r2 = median(ks / kf), median(kf / ks)
            if not np.isfinite(r1) or r1 == 0 or not np.isfinite(r2) or r2 == 0:
                raise ValueError(RATIO_ERROR)
            ratios[first, second] = r1
            ratios[second, first] = r2
    smallest = int(np.argmin(ratios.min(axis=0)))
    return ratios, smallest, ratios[:, smallest].copy()


def normalize(x, sf, log=True, pseudo_count=1.0):
    v = x / sf
    return np.log2(v + pseudo_count) if log else v


def multi_batch_norm(*batches, batch=None, size_factors=None, log=True, pseudo_count=1.0, min_mean=1.0, subset_row=None,
                     normalize_all=False, preserve_single=True):
    """Returns a dict: logcounts, size_factors (lists, or one matrix / vector for a single object kept whole), averages
    (|S| x B), ratios (B x B), reference (0-based), levels (single object)."""
    mats = [np.asarray(b, dtype=np.float64) for b in unpack_batches(batches)]
    G = mats[0].shape[0]
    sub = subset_index(subset_row, G)
    sub0 = None if sub is None else sub.astype(np.int64) - 1
    reorder = levels = None
    if len(mats) == 1:
        if batch is None:
            raise ValueError("'batch' must be specified if '...' has only one object")
        also = () if size_factors is None else (np.asarray(size_factors, dtype=np.float64),)
        div = divide_into_batches(mats[0], np.asarray(batch), also=also)
        mats, reorder, levels = div.parts, div.reorder, div.levels
        sfs = [None] * len(mats) if size_factors is None else div.also[0]
    else:
        preserve_single = False
        sfs = [None] * len(mats) if size_factors is None else list(size_factors)
    stats = [batch_statistics(m, s, sub0) for m, s in zip(mats, sfs)]
    aves = [a for _, a in stats]
    ratios, smallest, rescaling = rescale_size_factors(aves, min_mean)
    sf_out = [sf / r for (sf, _), r in zip(stats, rescaling)]
    rows = slice(None) if (sub0 is None or normalize_all) else sub0
    logcounts = [normalize(m[rows], s, log, pseudo_count) for m, s in zip(mats, sf_out)]
    out = {"averages": np.stack(aves, axis=1), "ratios": ratios, "reference": smallest, "levels": levels}
    if reorder is not None and preserve_single:
        out["logcounts"] = np.concatenate(logcounts, axis=1)[:, reorder - 1]
        out["size_factors"] = np.concatenate(sf_out)[reorder - 1]
    else:
        out["logcounts"], out["size_factors"] = logcounts, sf_out
    return out
