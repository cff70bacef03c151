"""The inputs of tests/knn_scale_cases.py are what tests/test_gpu_knn_scale.py assumes of them, shown with the oracle alone --
so that a failure of the GPU tests is the library's.  The figures printed here (-s) are the ones the GPU tests rest on."""
import numpy as np
import pytest

from tests import knn_scale_cases as C


def _same_rows_scaled(oracle, X, Q, k, exps):
    bi, bd = oracle.query_knn(X, Q, k)
    for e in exps:
        Xe, Qe = C.scaled((X, Q), e)
        assert np.array_equal(np.ldexp(Xe, -e), X) and np.array_equal(np.ldexp(Qe, -e), Q), e  # nothing left the normal range
        i, dd = oracle.query_knn(Xe, Qe, k)
        assert np.array_equal(i, bi), (k, e)
        assert np.array_equal(dd, np.ldexp(bd, e)), (k, e)


@pytest.mark.parametrize("k", [20, 36])
def test_reference_is_equivariant_under_powers_of_two(oracle, k):
    X, Q = C.base()
    _same_rows_scaled(oracle, X, Q, k, C.EXPONENTS)


def test_reference_is_equivariant_wide_rows(oracle):
    X, Q = C.base_wide()
    _same_rows_scaled(oracle, X, Q, 30, (-80, -12, 12, 40, 80))


def test_reference_is_equivariant_large_k(oracle):
    X, Q = C.base_large_k()
    _same_rows_scaled(oracle, X, Q, 50, (-40, 40))


def test_reference_is_equivariant_two_clusters(oracle):
    X, Q, _ = C.two_clusters()
    _same_rows_scaled(oracle, X, Q, C.CLUSTER_K, (-80, 80))


def test_general_position_inputs_keep_their_neighbours_apart(oracle):
    # factors and offsets change the mantissas, so the rows need not be the base's: the GPU tests take the oracle's rows of the
    # scaled data.  What they do need: the offset inputs still resolve the neighbours (no coordinate lost to the offset)
    X, Q = C.base()
    bi, _ = oracle.query_knn(X, Q, 20)
    for name, (Xo, Qo) in C.offsets().items():
        i, dd = oracle.query_knn(Xo, Qo, 20)
        same = (i == bi).mean()
        print(f"offset {name}: {same:.4f} of the base's entries unchanged, smallest distance {dd.min():.3f}")
        assert same > 0.99 and dd.min() > 1.0, name


def test_far_queries_lie_on_the_side_of_the_window_the_tests_assume():
    X, Q = C.base()
    moved = np.zeros(C.NQ, dtype=bool)
    moved[list(C.FAR_POSITIONS)] = True
    assert C.far_ratio(X, Q)[~moved].max() < 3  # the base's own queries are nowhere near
    for ratio in C.FAR_RATIOS:
        r = C.far_ratio(X, C.far_queries(X, Q, ratio))
        print(f"far queries at {ratio}: ratios {r[moved].min():.1f} .. {r[moved].max():.1f}; the others at most {r[~moved].max():.2f}")
        assert np.allclose(r[moved], ratio, rtol=1e-12)
        assert (r[moved] > C.POISONED_ABOVE).all() or (r[moved] < C.CLEAN_BELOW).all(), ratio
        assert (r[~moved] < C.CLEAN_BELOW).all()
    assert [(ratio > C.POISONED_ABOVE) for ratio in C.FAR_RATIOS] == [False, False, True, True]
    assert C.POISONED_ABOVE > 1364 and C.CLEAN_BELOW < 683


def test_one_sided_far_queries_offer_a_wrong_list_that_an_open_threshold_accepts(oracle):
    X, Q, side = C.one_sided_far_queries()
    k, n = C.ONE_SIDED_K, C.ONE_SIDED_N
    moved = list(C.FAR_POSITIONS)
    c, rmax = C.ref_centre_and_norm(X)
    assert side.sum() == n and k <= n < 32  # 32: the fp16 tier's list for k <= 20
    assert np.array_equal((X[:, C.FAR_COLUMN] - c[C.FAR_COLUMN]) > 0, side)
    # the centred coordinates of the column, times the scale (largest norm into (24, 48]), are not flushed by fp16 (2^-24)
    tiny = np.abs(X[:, C.FAR_COLUMN] - c[C.FAR_COLUMN]).min() * 24 / rmax
    assert tiny > 4 * 2.0 ** -24
    r = C.far_ratio(X, Q)
    assert (r[moved] > C.POISONED_ABOVE).all() and (np.delete(r, moved) < 3).all()
    oi, _ = oracle.query_knn(X, Q[moved], k)
    li, _ = oracle.query_knn(X[side], Q[moved], k)
    wrong = np.flatnonzero(side)[li - 1] + 1  # the list the 25 rows give
    in_side = side[oi - 1].sum(axis=1)
    print(f"one-sided far queries: ratio {r[moved].min():.0f}, smallest scaled |coordinate| {tiny:.2e} (fp16 step 5.96e-08), "
          f"true neighbours among the {n} rows: {in_side.tolist()} of {k}")
    assert (in_side < k / 2).all()
    assert (np.sort(wrong, axis=1) != np.sort(oi, axis=1)).any(axis=1).all()


def _device_centre(X):
    """colsum_partial / colsum_final of knn.hip for at most 16 384 rows: blocks of 256 rows, four interleaved partial sums a
    block, the blocks in order, times fl(1 / n)."""
    n, d = X.shape
    total = np.zeros(d)
    for r0 in range(0, n, 256):
        part = [np.zeros(d) for _ in range(4)]
        for r in range(r0, min(n, r0 + 256)):
            part[(r - r0) % 4] = part[(r - r0) % 4] + X[r]
        total = total + ((part[0] + part[1]) + (part[2] + part[3]))
    return total * (1.0 / n)


@pytest.mark.parametrize("factor", C.DEGENERATE_FACTORS)
def test_equal_references_take_the_unit_scale_branch(factor):
    X, Q = C.equal_references(factor)
    assert (X == X[0]).all() and X.shape == (500, C.D)
    with np.errstate(over="ignore", invalid="ignore"):
        centred = (X - _device_centre(X)).astype(np.float32).astype(np.float64)
        rm = np.sqrt((centred ** 2).sum(axis=1).max())
    print(f"equal references x {factor:g}: largest centred norm {rm:g}")
    if factor == 1.0:
        assert rm == 0.0
    assert not (rm > 1e-150) or not (rm < 1e150)  # pass_scale returns 1
    # every distance of a query is a tie: the rows are 1 .. k
    assert np.isfinite(X).all() and np.isfinite(Q).all()


def test_equal_queries():
    X, Q = C.equal_queries()
    assert (Q == Q[0]).all() and Q.shape == (C.NQ, C.D)


def test_two_clusters_offer_a_wrong_list_that_a_degenerate_certificate_accepts(oracle):
    X, Q, second = C.two_clusters()
    k, first = C.CLUSTER_K, C.CLUSTER_LIST
    assert np.array_equal(np.flatnonzero(np.arange(3000) % 4 == 3), np.flatnonzero(X[:, 0] > 0))
    oi, od = oracle.query_knn(X, Q, k)
    li, ld = oracle.query_knn(X[:first], Q, k)  # the best list the first 40 rows can give
    centre = X.mean(axis=0)
    to_centre = np.sqrt(((Q - centre) ** 2).sum(axis=1))
    own = ((X[:first, 0] > 0)[None, :] == second[:, None]).sum(axis=1)
    # queries of the first cluster (three in four): 30 of the first 40 rows are their own cluster's, those are not their k
    # nearest, and the k-th of them is far closer than the centre -- `kth < |q - centre|^2` holds for a list that is wrong
    a = ~second
    assert a.sum() == 192
    assert (own[a] >= k).all()
    assert (np.sort(li[a], axis=1) != np.sort(oi[a], axis=1)).any(axis=1).all()
    assert (ld[a, k - 1] < to_centre[a]).all()
    print(f"first cluster: k-th of the first {first} rows at {ld[a, k - 1].min():.3f} .. {ld[a, k - 1].max():.3f}, true k-th at "
          f"{od[a, k - 1].min():.3f} .. {od[a, k - 1].max():.3f}, centre at {to_centre[a].min():.3f} .. {to_centre[a].max():.3f}")
    # queries of the second cluster: rows r % 4 == 3 put only 10 of their own among the first 40, so the k-th of those rows
    # is across the gap and farther than the centre -- for them the degenerate certificate fails, as it should
    b = second
    assert (own[b] == 10).all() and (ld[b, k - 1] > to_centre[b]).all()
    print(f"second cluster: k-th of the first {first} rows at {ld[b, k - 1].min():.3f} .. {ld[b, k - 1].max():.3f}, centre at "
          f"{to_centre[b].min():.3f} .. {to_centre[b].max():.3f}")
    # no exact ties among the true neighbours: the rows are unique
    assert (np.diff(od, axis=1) > 0).all()
