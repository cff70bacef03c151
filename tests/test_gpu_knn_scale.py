"""The exact kNN outside unit scale (inputs: tests/knn_scale_cases.py, held to their preconditions by
tests/test_cpu_knn_scale_cases.py).  Every answer of query_knn, find_knn and find_mutual_nn rests on "the candidate pass was
accurate to within pass_eps, so the FP64 certificate of knn_refine proves the top k"; pass_eps is a relative bound, and the
code around it has special cases that exist only because data need not be of unit size.  The bar is the usual one: indices equal
to the oracle's, distances bitwise.  Nothing is asserted about time.

Counts: _left_tier1() is test_gpu_knn_f16_mfma_shape.py's (the counters "knn_exact_fallbacks" + "knn_tier2_queries").  Where a
count is compared with the count at e = 0 the comparison is an equality, and it is derived, not measured: s is a power of two,
so the fp16 images of 2^e X are those of X bit for bit, the margins and the cut work in scaled units, and every term of the
certificate scales by exactly 2^(2e) -- the same queries fail it."""
import numpy as np
import pytest

from tests import knn_scale_cases as C
from tests.find_knn_ref import find_knn_ref

pytestmark = pytest.mark.gpu
SHAPES = (0, 1)


@pytest.fixture(scope="module")
def nb():
    from batchelor_amd import neighbors
    return neighbors


@pytest.fixture(scope="module")
def nat():
    from batchelor_amd import natives
    return natives


def _counters():
    from batchelor_amd import _lib
    return np.array([_lib.dev_get("knn_exact_fallbacks"), _lib.dev_get("knn_tier2_queries")])


def _left_tier1():
    return int(_counters().sum())


def _ran_shape():
    from batchelor_amd import _lib
    return _lib.dev_get("knn_mfma_shape")


def _query(nb, X, Q, k, rows, what):
    """One query_knn against the oracle's rows; returns what the counters moved by: (exact fall-backs, handed to tier 2)."""
    before = _counters()
    idx, dist = nb.query_knn(X, Q, k)
    moved = _counters() - before
    print(what, "exact fall-backs / tier-2 queries:", moved)
    assert np.array_equal(idx, rows[0]), what
    assert np.array_equal(dist, rows[1]), what
    return moved


_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _base_rows(oracle, name, k):
    X, Q = getattr(C, name)()
    return _cached((name, k), lambda: (X, Q, oracle.query_knn(X, Q, k)))


def _scaled_rows(oracle, name, k, e):
    """(2^e X, 2^e Q, rows): the oracle's rows of the scaled input, which are the base's with the distances times 2^e."""
    X, Q, (bi, bd) = _base_rows(oracle, name, k)
    Xe, Qe = C.scaled((X, Q), e)
    rows = oracle.query_knn(Xe, Qe, k)
    assert np.array_equal(rows[0], bi) and np.array_equal(rows[1], np.ldexp(bd, e))
    return Xe, Qe, rows


# ---- case 1: power-of-two scales, tier 1 -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("k", [20, 36])
def test_powers_of_two_tier1(oracle, nb, dev, k, shape):
    """pass_scale's exponent, s2inv applied as 1 / s^2, the margins in scaled units: the rows of 2^e X are those of X, and
    exactly as many queries leave the fp16 tier as at e = 0 (where test_gpu_knn_f16_mfma_shape.py's 5 % cap applies)."""
    dev("mfma_shape", shape)
    X, Q, rows = _scaled_rows(oracle, "base", k, 0)
    at0 = _query(nb, X, Q, k, rows, ("e", 0, k, shape))
    assert _ran_shape() == shape
    assert at0.sum() <= 0.05 * C.NQ
    for e in C.EXPONENTS:
        Xe, Qe, rows = _scaled_rows(oracle, "base", k, e)
        left = _query(nb, Xe, Qe, k, rows, ("e", e, k, shape))
        assert _ran_shape() == shape
        assert np.array_equal(left, at0), (e, left, at0)


# ---- case 2: the same through tier 2 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,tier", [("base", 20, 2), ("base_wide", 30, 0)])
def test_powers_of_two_tier2(oracle, nb, dev, name, k, tier):
    """The split-bf16 tier alone (forced at d = 50; the natural first tier at d = 70, k = 30).  It is unscaled: inside its
    exponent window (pass_window, knn_select.hpp) every f32 value of the pass scales by exactly 2^(2e) and so does the
    certificate; at e = +-80 the data are outside the window and only the rows are promised (test_two_clusters_*)."""
    if tier:
        dev("knn_tier", tier)
    X, Q, rows = _scaled_rows(oracle, name, k, 0)
    at0 = _query(nb, X, Q, k, rows, (name, 0))
    assert at0.sum() <= 0.05 * C.NQ
    for e in (-12, 12, 40):
        Xe, Qe, rows = _scaled_rows(oracle, name, k, e)
        left = _query(nb, Xe, Qe, k, rows, (name, e))
        assert np.array_equal(left, at0), (e, left, at0)
    for e in (-80, 80):
        Xe, Qe, rows = _scaled_rows(oracle, name, k, e)
        _query(nb, Xe, Qe, k, rows, (name, e))


# ---- case 3: general position ------------------------------------------------------------------------------------------
def _general_inputs():
    X, Q = C.base()
    out = [("x%g" % f, X * f, Q * f) for f in C.FACTORS]
    out += [(name, Xo, Qo) for name, (Xo, Qo) in C.offsets().items()]
    out += [("2^%d" % e,) + tuple(C.scaled((X, Q), e)) for e in (-80, 80)]
    return out


GENERAL = ["x1e-06", "x0.001", "x10000", "x1e+06", "all+1e4", "col11+1e6", "2^-80", "2^80"]


def _general(name):
    table = _cached("general", lambda: {n: (X, Q) for n, X, Q in _general_inputs()})
    assert sorted(table) == sorted(GENERAL)
    return table[name]


@pytest.mark.parametrize("name", GENERAL)
def test_general_position_query_knn(oracle, nb, name):
    """Factors that are no powers of two, and offsets that the centring must absorb (a wrong centre shows as every query
    falling back): the oracle's rows of the same data, with the fp16 tier doing the work."""
    X, Q = _general(name)
    left = _query(nb, X, Q, 20, oracle.query_knn(X, Q, 20), name)
    assert left.sum() <= 0.05 * C.NQ, (name, left)


@pytest.mark.parametrize("name", GENERAL)
def test_general_position_find_knn(oracle, nb, name):
    X, _ = _general(name)
    ri, rd = find_knn_ref(oracle, X, 20)
    before = _left_tier1()
    idx, dist = nb.find_knn(X, 20)
    left = _left_tier1() - before
    print(name, "left tier 1:", left)
    assert np.array_equal(idx, ri) and np.array_equal(dist, rd), name
    assert left <= 0.05 * C.NR, (name, left)


@pytest.mark.parametrize("name", GENERAL)
def test_general_position_mutual_nn(oracle, nat, name):
    """findMutualNN plain and as the merges run it (mnn_average_correction: the second search is seeded, pairs.hip's
    seed_from_lists rounds each seed up to f32 -- at 2^-80 through the f32 subnormals, at 2^80 to +inf)."""
    X, Q = _general(name)
    of, os_ = oracle.find_mutual_nn(X, Q, 20, 20)
    assert of.size > 0
    before = _left_tier1()
    f, s = nat.find_mutual_nn(X, Q, 20, 20)
    assert np.array_equal(f, of) and np.array_equal(s, os_), name
    f, s, _, _ = nat.mnn_average_correction(X, Q, 20)
    assert np.array_equal(f, of) and np.array_equal(s, os_), name
    left = _left_tier1() - before
    print(name, "left tier 1:", left)
    assert left <= 0.05 * (2 * (C.NR + C.NQ)), (name, left)


# ---- case 4: beyond the f32 window of the unscaled tier ----------------------------------------------------------------
@pytest.mark.parametrize("tier", [0, 2])
@pytest.mark.parametrize("e", [-80, 80])
def test_two_clusters_beyond_the_window_of_the_unscaled_tier(oracle, nb, dev, e, tier):
    """d = 70, k = 30: the split-bf16 tier is the first tier, unscaled, its norms (float)|r'|^2 and its products f32.  At 2^-80
    the norms are 0 and every product underflows: the pass's values carry no information, `kth < tmin + |q~|^2 - eps` is about
    `kth < |q - centre|^2`, and for the first cluster's queries a list from the first 40 rows satisfies it while being wrong
    (tests/test_cpu_knn_scale_cases.py).  At 2^80 the norms are +inf and every value NaN.  The contract: outside the window in
    which pass_eps holds for the unscaled pass every query fails the certificate and goes on -- so at 2^-80 all 256 reach the
    exact search.

    Before pass_window existed (measured on the MI355X; MEASUREMENTS.md, "kNN outside unit scale"): at 2^-80 the 192 queries of
    the first cluster were certified with rows that were not their neighbours and only the 64 of the second reached the exact
    search, with the default tiers and with "knn_tier" = 2 alike; at 2^80 all 256 failed the certificate already."""
    if tier:
        dev("knn_tier", tier)
    X, Q, _ = C.two_clusters()
    Xe, Qe = C.scaled((X, Q), e)
    left = _query(nb, Xe, Qe, C.CLUSTER_K, oracle.query_knn(Xe, Qe, C.CLUSTER_K), ("clusters", e, tier))
    if e < 0:
        assert left[0] == Q.shape[0] and left[1] == 0, left  # one tier: all of its queries in the exact search


# ---- case 5: far queries -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("k", [1, 20])
def test_far_queries(oracle, nb, dev, k, shape):
    """A query whose -2 q' s leaves the fp16 range gets a NaN norm and fails the certificate whatever the pass collects
    (prep_rows_f16<1>, knn_prep.hip); its neighbours in the wave, in the lane (16x16x32: queries j and j + 16) and in the
    workgroup must not notice.  d = 50 has two tiers, so "knn_tier2_queries" moves by exactly the number that left the fp16
    tier: at ratios beyond 32752 / 24 that is at least the moved queries."""
    dev("mfma_shape", shape)
    X, Q0 = C.base()
    n_moved = len(C.FAR_POSITIONS)
    for ratio in C.FAR_RATIOS:
        Q = C.far_queries(X, Q0, ratio)
        left = _query(nb, X, Q, k, oracle.query_knn(X, Q, k), ("far", ratio, k, shape))
        assert _ran_shape() == shape
        if ratio > C.POISONED_ABOVE:
            assert left[1] >= n_moved, (ratio, left)
        assert left[1] <= 0.05 * C.NQ + n_moved, (ratio, left)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("no_margin", [0, 1])
def test_far_queries_with_an_open_threshold(oracle, nb, dev, no_margin, shape):
    """test_far_queries cannot tell whether the NaN norm does anything: there half of the references get a value of -inf from the
    query's overflowed image, the lists fill, the threshold drops to -inf and the certificate fails by itself.  Here only 25
    references do (k <= 25 < KS): the list never fills, the threshold stays at +inf, nothing counts as rejected, and without the
    NaN norm `kth < +inf` certifies the 20 nearest of those 25 rows, which are not the query's neighbours
    (tests/test_cpu_knn_scale_cases.py).  With the margin cut and, through the testing hook, with the KS-th-best cut alone."""
    dev("mfma_shape", shape)
    dev("no_margin", no_margin)
    X, Q, _ = C.one_sided_far_queries()
    left = _query(nb, X, Q, C.ONE_SIDED_K, oracle.query_knn(X, Q, C.ONE_SIDED_K), ("one-sided", no_margin, shape))
    assert _ran_shape() == shape
    assert left[1] >= len(C.FAR_POSITIONS), left


# ---- case 6: one far reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [10, 20])
@pytest.mark.parametrize("row", C.FAR_REFERENCES)
def test_one_far_reference(oracle, nb, dev, row, e):
    """One reference 2^10 / 2^20 times as far out as the others: the scale follows it, and at 2^20 the ordinary cells' scaled
    coordinates are fp16 subnormals -- the eps_den term of pass_eps.  Rows only: the margin grows with the largest norm, so
    nothing is promised about which tier answers."""
    X, Q = C.base()
    X = C.far_reference(X, row, e)
    rows = oracle.query_knn(X, Q, 20)
    for shape in SHAPES:
        dev("mfma_shape", shape)
        _query(nb, X, Q, 20, rows, ("far reference", row, e, shape))


# ---- case 7: degenerate norms ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", C.DEGENERATE_FACTORS)
def test_equal_references(oracle, nb, factor):
    """500 references all equal to one row: the largest centred norm is 0 (at 1e170: beyond 1e150), pass_scale's scale = 1
    branch.  Every distance of a query is a tie, and ties go to the lower row."""
    X, Q = C.equal_references(factor)
    for k in (1, 20):
        rows = oracle.query_knn(X, Q, k)
        assert np.array_equal(rows[0], np.tile(np.arange(1, k + 1), (C.NQ, 1)))
        _query(nb, X, Q, k, rows, ("equal references", factor, k))


def test_equal_queries(oracle, nb):
    X, Q = C.equal_queries()
    _query(nb, X, Q, 20, oracle.query_knn(X, Q, 20), "equal queries")


# ---- case 8: the partitioned search at scale ---------------------------------------------------------------------------
@pytest.mark.parametrize("e", [-40, 40])
def test_partitioned_search(oracle, nb, e):
    """k = 50: four partitions of 750 rows at k = 36 each, merged exactly (knn_large_k.hip).  Fewer exact fall-backs than
    queries: the partitions did the work."""
    Xe, Qe, rows = _scaled_rows(oracle, "base_large_k", 50, e)
    left = _query(nb, Xe, Qe, 50, rows, ("k = 50", e))
    assert left[0] < Qe.shape[0], left
