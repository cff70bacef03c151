"""mnnDeltaVariance() without a GPU: the numpy restatement (tests/delta_variance_ref.py) against a literal per-gene,
per-pair loop; the refusals, raised before a device is asked for; the host-side bookkeeping (pair validation, subset.row /
compute.all, the weighted combination); and the inputs and error bounds that tests/test_gpu_delta_variance.py uses, with
the check that the float64 restatement itself stays inside those bounds on every one of them.

The bounds are derived, not measured.  With u = 2^-53 and the numpy.longdouble restatement as the exact value, a two-pass
variance of P terms in FP64 is within 8 P u total of it in any summation order, and the mean within
4 P u mean_p(|x_left| + |x_right|) / 2; the inputs keep |mean delta| / sd delta <= 1e4 and P <= 1e4, so the second-order
term of the variance bound is negligible."""
import functools

import numpy as np
import pytest

from tests import delta_variance_ref as ref
from tests.test_cpu_inputs import ROWS, NAMES, SUBSET, _refused

U = 2.0 ** -53
G_LABELS = ["1", "7", "T-1", "T", "T+1", "2T+1"]
P_LABELS = ["0", "1", "2", "3", "C-1", "C", "C+1", "3C+5"]
SIZES = (40, 600, 251)   # three batches of unequal size


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from batchelor_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def tile_and_chunk():
    """The gene-tile width and the pair-chunk length the kernels use, asked of the library (no device needed)."""
    from batchelor_amd import delta_variance as dv
    return dv.gene_tile(), dv.pair_chunk()


def resolve(label):
    T, C = tile_and_chunk()
    return int(eval(label.replace("2T", "2*T").replace("3C", "3*C"), {"T": T, "C": C}))


# ---------------------------------------------------------------------------------------------- inputs
def make_batches(G, sizes, seed, shift=1.0):
    """Positive values with population structure and a batch effect (the shape of the mnnCorrect tests' data), rounded to
    multiples of 2^-12.  The bounds cover the order of the sums; they do not cover the rounding of a delta x_left - x_right
    that is large against the spread of the deltas, which no order of summation can undo (with two or three pairs some
    gene always has such deltas).  On this grid a delta is exact in FP64, so the bounds hold for every gene and P; the
    cos_norm cases and the offset case, whose values leave the grid, use enough pairs for the bounds to hold there too
    (test_float64_restatement_stays_inside_the_bounds)."""
    rng = np.random.default_rng(seed)
    base = rng.normal(size=(G, 4))
    out = []
    for i, n in enumerate(sizes):
        lat = rng.normal(size=(4, n))
        x = np.abs(base @ lat + rng.normal(scale=0.3, size=(G, n)) + shift * i * rng.normal(size=(G, 1)))
        out.append(np.round(x * 4096.0) / 4096.0)
    return out


def cross_pairs(P, sizes, seed, avoid=()):
    """P pairs sorted by left cell, the right cell always in a later batch than the left: every combination of batches
    occurs.  1-based columns of the batches side by side; `avoid`: 1-based columns that stay unpaired."""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(sizes)])
    combos = [(a, b) for a in range(len(sizes)) for b in range(a + 1, len(sizes))]
    left, right = np.zeros(P, dtype=np.int64), np.zeros(P, dtype=np.int64)
    for p in range(P):
        a, b = combos[p % len(combos)]
        while True:
            l, r = off[a] + rng.integers(sizes[a]) + 1, off[b] + rng.integers(sizes[b]) + 1
            if l not in avoid and r not in avoid:
                break
        left[p], right[p] = l, r
    order = np.argsort(left, kind="stable")
    return left[order].astype(np.int32), right[order].astype(np.int32)


class Case:
    def __init__(self, batches, pairs, **kwargs):
        self.batches, self.pairs, self.kwargs = batches, pairs, kwargs   # pairs: a list of (left, right)


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of the GPU tests by name, built once."""
    T, C = tile_and_chunk()
    if name.startswith("shape:"):
        _, g, p = name.split(":")
        G, P = resolve(g), resolve(p)
        return Case(make_batches(G, SIZES, 1000 + G), [cross_pairs(P, SIZES, 2000 + P)])
    if name == "left-run":   # one left cell in 20 consecutive pairs, across a group of four and a chunk edge
        left, right = cross_pairs(C + 40, SIZES, 31)
        left = left.copy()
        left[C - 9:C + 11] = left[C - 9]
        right = right.copy()
        right[C - 9:C + 11] = sum(SIZES[:2]) + np.arange(1, 21)     # (twenty cells of the last batch)
        return Case(make_batches(T + 1, SIZES, 32), [(left, right)])
    if name in ("same-pair-twice", "only-one-pair-twice"):
        left, right = cross_pairs(C if name == "same-pair-twice" else 2, SIZES, 41)
        left, right = left.copy(), right.copy()
        left[1], right[1] = left[0], right[0]
        return Case(make_batches(T + 1, SIZES, 42), [(left, right)])
    if name in ("cos-zero-cell-paired", "cos-zero-cell-unpaired"):
        B = make_batches(T + 1, SIZES, 51)
        zero = SIZES[0] + 7                                          # 1-based column, in the second batch
        B[1][:, 6] = 0.0
        if name == "cos-zero-cell-paired":
            left, right = cross_pairs(C + 1, SIZES, 52)
            right = right.copy()
            right[np.flatnonzero(left <= SIZES[0])[:3]] = zero       # three pairs from the first batch to it
        else:
            left, right = cross_pairs(C + 1, SIZES, 52, avoid=(zero,))
        return Case(B, [(left, right)], cos_norm=True)
    if name.startswith("subset"):                                    # subset[-all][-cos][:number of genes]
        G = 2 * T + 1
        n_sub = int(name.split(":")[1]) if ":" in name else T + 44
        sub = np.random.default_rng(61).permutation(G)[:n_sub] + 1   # shuffled
        return Case(make_batches(G, SIZES, 62), [cross_pairs(C + 1, SIZES, 63)], subset_row=sub,
                    compute_all="-all" in name, cos_norm="-cos" in name)
    if name == "offset":     # the second batch is the first plus 1e4 per gene, with unit noise
        rng = np.random.default_rng(71)
        first = make_batches(T + 1, (300,), 72)[0]
        sizes = (300, 300)
        return Case([first, first + 1e4 + rng.normal(size=first.shape)], [cross_pairs(3 * C + 5, sizes, 73)])
    if name == "three-steps":
        return Case(make_batches(T + 1, SIZES, 81), [cross_pairs(C + 1, SIZES, 82), cross_pairs(3 * C + 5, SIZES, 83),
                                                    cross_pairs(7, SIZES, 84)])
    if name == "three-steps-one-pair":   # a step that gets no weight
        return Case(make_batches(7, SIZES, 85), [cross_pairs(C + 1, SIZES, 86), cross_pairs(1, SIZES, 87),
                                                 cross_pairs(9, SIZES, 88)])
    raise KeyError(name)


SHAPE_CASES = [f"shape:{g}:{p}" for g in G_LABELS for p in P_LABELS]
OTHER_CASES = ["left-run", "same-pair-twice", "only-one-pair-twice", "cos-zero-cell-paired", "cos-zero-cell-unpaired",
               "subset", "subset-all", "subset-cos", "subset-all-cos", "offset", "three-steps", "three-steps-one-pair"]


# ---------------------------------------------------------------------------------------------- bounds
class Bounds:
    """Per step: the longdouble restatement's mean and total and what FP64 may differ from them by."""
    def __init__(self, batches, pairs, **kwargs):
        sel = {k: kwargs.get(k) for k in ("cos_norm", "subset_row", "compute_all")}
        sel = {"cos_norm": bool(sel["cos_norm"]), "subset_row": sel["subset_row"], "compute_all": bool(sel["compute_all"])}
        self.exact = ref.mnn_delta_variance(batches, pairs, longdouble=True, **sel)
        x, remapped, _ = ref.prepare(batches, pairs, longdouble=True, **sel)
        self.steps = []
        for (l, r), t in zip(remapped, self.exact["per_step"]):
            P = len(l)
            mag = (np.abs(x[:, l - 1]).mean(axis=1) + np.abs(x[:, r - 1]).mean(axis=1)) / 2 if P else np.zeros(x.shape[0])
            self.steps.append({"P": P, "mean": t["mean"], "total": t["total"], "tol_mean": 4 * P * U * mag,
                               "tol_total": 8 * P * U * t["total"]})

    def worst(self, i, mean, total):
        """Step i: the largest |value - exact| / allowance over all genes, for the mean and for the total (0 where both
        are exact, inf where the allowance is 0 and the value differs).  Asserts the NaNs are where they belong."""
        s = self.steps[i]
        out = []
        for got, want, tol, least in ((mean, s["mean"], s["tol_mean"], 1), (total, s["total"], s["tol_total"], 2)):
            got = np.asarray(got)
            assert got.shape == want.shape and got.dtype == np.float64
            if s["P"] < least:
                assert np.all(np.isnan(got)), "fewer pairs than the statistic needs: NaN"
                out.append(0.0)
                continue
            assert not np.any(np.isnan(got))
            err = np.abs(got.astype(np.longdouble) - want)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(err == 0, 0.0, err / tol)
            out.append(float(ratio.max()))
        return tuple(out)


@functools.lru_cache(maxsize=None)
def bounds(name):
    c = case(name)
    return Bounds(c.batches, c.pairs, **c.kwargs)


def one_pass_total(x, left, right):
    """sum delta^2 - (sum delta)^2 / P over P - 1 in float64: what the offset case is there to catch."""
    d = x[:, left - 1] - x[:, right - 1]
    P = d.shape[1]
    return ((d * d).sum(axis=1) - d.sum(axis=1) ** 2 / P) / (P - 1)


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("kw", [dict(), dict(cos_norm=True), dict(subset_row=[5, 2, 7]), dict(subset_row=[5, 2, 7], compute_all=True),
                                dict(cos_norm=True, subset_row=[5, 2, 7]), dict(cos_norm=True, subset_row=[5, 2, 7], compute_all=True)],
                         ids=lambda kw: "-".join(sorted(kw)) or "plain")
def test_restatement_matches_a_literal_loop(kw):
    sizes = (5, 9, 6)
    B = make_batches(7, sizes, 3)
    B[1][:, 2] = 0.0
    pairs = [cross_pairs(11, sizes, 4), cross_pairs(1, sizes, 5), cross_pairs(0, sizes, 6), cross_pairs(2, sizes, 7)]
    got = ref.mnn_delta_variance(B, pairs, **kw)
    want = ref.literal(B, pairs, **kw)
    for i, (g, w) in enumerate(zip(got["per_step"], want)):
        for f in ("mean", "total"):
            assert np.array_equal(np.isnan(g[f]), np.isnan(w[f])), (i, f)
            # both float64, at most 11 terms a sum: a few ulps of the terms' magnitude (values and deltas are O(1))
            np.testing.assert_allclose(g[f], w[f], rtol=1e-12, atol=1e-14, err_msg=f"step {i} {f}")
    assert got["npairs"].tolist() == [11, 1, 0, 2]
    w = np.array([11.0, 2.0])
    for f in ("mean", "total"):
        np.testing.assert_allclose(got[f], (w[0] * want[0][f] + w[1] * want[3][f]) / w.sum(), rtol=1e-12, atol=1e-14)
    single = ref.mnn_delta_variance(B, pairs[0], **kw)               # one (left, right) is one step (:131-133)
    assert len(single["per_step"]) == 1 and np.array_equal(single["per_step"][0]["total"], got["per_step"][0]["total"])


@pytest.mark.parametrize("name", SHAPE_CASES + OTHER_CASES)
def test_float64_restatement_stays_inside_the_bounds(built, name):
    c, b = case(name), bounds(name)
    f64 = ref.mnn_delta_variance(c.batches, c.pairs, **c.kwargs)
    for i, t in enumerate(f64["per_step"]):
        em, et = b.worst(i, t["mean"], t["total"])
        print(f"{name} step {i} P={b.steps[i]['P']}: float64 restatement error / allowance: mean {em:.3g}, total {et:.3g}")
        assert em <= 1.0 and et <= 1.0
    for s in b.steps:   # what keeps the bound's second-order term negligible
        assert s["P"] <= 10_000


def test_offset_case_catches_a_one_pass_variance(built):
    c, b = case("offset"), bounds("offset")
    x = np.concatenate(c.batches, axis=1)
    left, right = c.pairs[0]
    d = x[:, left - 1] - x[:, right - 1]
    ratio = np.abs(d.mean(axis=1)) / d.std(axis=1, ddof=1)
    em, et = b.worst(0, b.steps[0]["mean"].astype(np.float64), one_pass_total(x, left, right))
    print(f"offset case: |mean delta| / sd delta up to {ratio.max():.4g}; one-pass variance error / allowance {et:.3g}")
    assert ratio.max() <= 1e4 and ratio.min() > 1e3
    assert et > 1.0


# ---------------------------------------------------------------------------------------------- refusals
RNG = np.random.default_rng(909)
A, B2 = RNG.normal(size=(12, 9)), RNG.normal(size=(12, 11))
OK = ([1, 2], [10, 20])
REFUSED = [
    ((A, B2), {"pairs": ([0, 2], [10, 20])}, "'pairs' indices out of range"),
    ((A, B2), {"pairs": ([1, 2], [10, 21])}, "'pairs' indices out of range"),
    ((A, B2), {"pairs": [OK, ([1], [21])]}, "'pairs' indices out of range"),
    ((A, B2), {"pairs": ([1, 2, 3], [10, 20])}, "differ in length"),
    ((A, B2), {"pairs": []}, "at least one merge step"),
    ((A, B2), {}, "'pairs' must be specified"),
    ((A, B2), {"pairs": ([1.5, 2], [10, 20])}, "integer"),
    ((A, B2[:5]), {"pairs": OK}, ROWS),
    ((A, B2), {"pairs": OK, "subset_row": [0, 1]}, SUBSET),
    ((A, B2), {"pairs": OK, "subset_row": []}, "selects no genes"),
    ((A, B2), {"pairs": OK, "names": ["a", "a"]}, NAMES),
    ((), {"pairs": OK}, "at least one batch"),
]


@pytest.mark.parametrize("args,kwargs,msg", REFUSED, ids=[str(i) for i in range(len(REFUSED))])
def test_refused_before_a_device_is_asked_for(built, args, kwargs, msg):
    _refused("mnnDeltaVariance", args, kwargs, msg)


def test_sparse_and_sce_inputs_are_refused(built):
    import batchelor_amd as bx

    class FakeSparse:
        def tocsr(self):
            return self

    class SingleCellExperiment:
        assays = {}

    for bad, word in ((FakeSparse(), "sparse"), (SingleCellExperiment(), "SingleCellExperiment")):
        with pytest.raises(TypeError, match=word):
            bx.mnnDeltaVariance(A, bad, pairs=OK)


def test_the_library_refuses_bad_arguments_without_a_device(built):
    """bmx_delta_run's own checks need a handle, which needs a device; what can be asked without one is asked here."""
    import ctypes
    L = built.lib()
    for name in ("create", "destroy", "begin_batch", "add_block", "run", "stage_ms"):
        assert hasattr(L, f"bmx_delta_{name}"), name
    T, C = tile_and_chunk()
    assert T >= 64 and T % 2 == 0 and C >= 4
    h = ctypes.c_void_p()
    assert L.bmx_delta_create(ctypes.c_int32(0), ctypes.c_int32(0), ctypes.byref(h)) != 0
    assert b"at least one gene" in L.bmx_last_error()
    assert L.bmx_delta_begin_batch(None, ctypes.c_int64(3)) != 0 and b"null handle" in L.bmx_last_error()


# ---------------------------------------------------------------------------------------------- host-side bookkeeping
def test_check_pairs(built):
    from batchelor_amd import delta_variance as dv
    one = dv.check_pairs(([3, 1], [4, 20]), 20)
    assert len(one) == 1 and one[0][0].dtype == np.int32 and one[0][0].tolist() == [3, 1] and one[0][1].tolist() == [4, 20]
    many = dv.check_pairs([(np.array([3, 1]), np.array([4, 20])), ([], []), (np.array([2.0]), np.array([5], dtype=np.int64))], 20)
    assert [l.size for l, _ in many] == [2, 0, 1] and all(l.dtype == np.int32 and r.dtype == np.int32 for l, r in many)
    two_steps_of_two = dv.check_pairs([([1, 2], [3, 4]), ([5, 6], [7, 8])], 20)
    assert len(two_steps_of_two) == 2


def test_plan_genes(built):
    from batchelor_amd import delta_variance as dv
    p = dv.plan_genes(None, False, 6)
    assert p.rows is None and p.norm_genes0 is None and p.fit_rows0 is None and p.gene_index.tolist() == [1, 2, 3, 4, 5, 6]
    p = dv.plan_genes([5, 2], False, 6)      # subset first, then forgotten (:113-119)
    assert p.rows.tolist() == [5, 2] and p.norm_genes0 is None and p.fit_rows0 is None and p.gene_index.tolist() == [5, 2]
    p = dv.plan_genes([5, 2], True, 6)       # every gene kept: the subset restricts the norms and the fit
    assert p.rows is None and p.norm_genes0.tolist() == [4, 1] and p.norm_genes0.dtype == np.int32
    assert p.fit_rows0.tolist() == [4, 1] and p.gene_index.tolist() == [1, 2, 3, 4, 5, 6]
    p = dv.plan_genes(np.array([False, True, True, False, False, False]), True, 6)
    assert p.norm_genes0.tolist() == [1, 2]


def test_compute_all_fits_on_the_subset_and_gives_every_gene_a_value(built):
    from batchelor_amd import delta_variance as dv
    G = 10
    mean, total = np.arange(G, dtype=float), np.arange(G, dtype=float) ** 2
    plan = dv.plan_genes([8, 3, 5], True, G)
    seen = []

    def trend_fit(m, t):
        seen.append((m.copy(), t.copy()))
        slope = t.sum() / m.sum()
        return lambda at: slope * at

    t = dv.step_table(mean, total, 12, trend_fit, plan.fit_rows0)
    assert len(seen) == 1 and seen[0][0].tolist() == [7.0, 2.0, 4.0] and seen[0][1].tolist() == [49.0, 4.0, 16.0]
    slope = (49.0 + 4.0 + 16.0) / 13.0
    assert t.trend.shape == (G,) and np.array_equal(t.trend, slope * mean) and np.array_equal(t.adjusted, total - slope * mean)
    none = dv.step_table(mean, total, 12)
    assert none.trend is None and none.adjusted is None
    lone = dv.step_table(mean, np.full(G, np.nan), 1, trend_fit, plan.fit_rows0)   # nothing to fit on
    assert len(seen) == 1 and np.all(np.isnan(lone.trend)) and np.all(np.isnan(lone.adjusted))


def test_combination_weights(built):
    from batchelor_amd import delta_variance as dv
    rng = np.random.default_rng(5)
    npairs = [30, 1, 7]
    tabs = [dv.DeltaStepTable(mean=rng.normal(size=4), total=rng.random(4), trend=rng.random(4), adjusted=rng.normal(size=4))
            for _ in npairs]
    tabs[1].total[:] = np.nan                                        # the step with one pair has no variance ...
    tabs[1].adjusted[:] = np.nan
    got = dv.combine_steps(tabs, npairs)
    want = ref.combine_blocks([{f: getattr(t, f) for f in ref.FIELDS} for t in tabs], npairs)
    for f in ref.FIELDS:                                             # ... and gets no weight
        np.testing.assert_allclose(got[f], (30 * getattr(tabs[0], f) + 7 * getattr(tabs[2], f)) / 37, rtol=1e-15)
        np.testing.assert_allclose(got[f], want[f], rtol=1e-15)
    none = dv.combine_steps(tabs[:2], [1, 0])
    assert all(np.all(np.isnan(none[f])) and none[f].shape == (4,) for f in ref.FIELDS)
    bare = dv.combine_steps([dv.DeltaStepTable(mean=np.ones(3), total=np.ones(3))], [5])
    assert bare["trend"] is None and bare["adjusted"] is None and bare["mean"].tolist() == [1, 1, 1]
