"""The two MFMA shapes of the fp16 candidate sweep (knn_f16.hip, knn_topk_f16's last template parameter): 0 = 32x32x16, one
accumulator per 32 x 32 tile, a lane holds 16 values of one query; 1 = 16x16x32, four 16 x 16 blocks per tile (reference half
a, query half b), a lane holds four values of each block: two queries, references 16 a + 4 (lane >> 4) + i.  The testing hook
"mfma_shape" forces either.  Everything goes through the public searches; the bar is the usual one -- indices equal to the
oracle's, distances bitwise -- and the fp16 tier must have done the work: at most 5 % of a case's queries may leave it
(counters "knn_exact_fallbacks" + "knn_tier2_queries": what profile_detail reports of an engine, here of the engine behind the
single-primitive entry points).  A wrong fragment order or tag decode does not survive the exact re-rank as a wrong distance
but as a missing neighbour or as queries that fail their certificate, so both are asserted.

Shape 1 exists for an even number of k-steps (NS = 2, 4, 6, 8; d + 3 columns in steps of 16); lists of 48 (k in 21..36) up to
NS = 4."""
import numpy as np
import pytest

from tests.conftest import synth_batches

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


def _left_tier1():
    from batchelor_amd import _lib
    return _lib.dev_get("knn_exact_fallbacks") + _lib.dev_get("knn_tier2_queries")


def _ran_shape():
    from batchelor_amd import _lib
    return _lib.dev_get("knn_mfma_shape")


def _check(nb, dev, shape, oracle_rows, X, Q, k, what=None):
    """One search with the shape forced, against the oracle's rows: the rows, that the forced shape is the one that ran, and
    that the fp16 tier did the work."""
    oi, od = oracle_rows
    dev("mfma_shape", shape)
    before = _left_tier1()
    idx, dist = nb.query_knn(X, Q, k)
    left = _left_tier1() - before
    assert _ran_shape() == shape, (shape, what)
    assert np.array_equal(idx, oi), (shape, what)
    assert np.array_equal(dist, od), (shape, what)
    assert left <= 0.05 * Q.shape[0], (shape, what, left)
    return idx, dist


@pytest.fixture(scope="module")
def positions():
    """4 224 references (33 slots of four tiles), d = 50 (NS = 4), 256 queries (one workgroup, 8 consumer waves).  Query q of
    wave w is an exact copy of reference 32 T + ((7 q + 3 w + s) mod 32): over s = 0..31 every query of a wave meets every
    row of tile T, i.e. every (lane, a, b, i) of the 16 x 16 blocks and every (lane, group, i) of the 32 x 32 tile."""
    (X,) = synth_batches(31, [4224], 50)
    T = 77  # second tile of a slot's first pair
    q, w = np.meshgrid(np.arange(32), np.arange(8))
    base = (7 * q + 3 * w).ravel()  # [wave][query of the wave]
    return X, T, base


def test_every_position_of_a_tile(oracle, nb, dev, positions):
    X, T, base = positions
    for s in range(32):
        target = 32 * T + (base + s) % 32
        Q = X[target].copy()
        rows = oracle.query_knn(X, Q, 20)
        assert np.array_equal(rows[0][:, 0], target + 1) and not rows[1][:, 0].any()
        for shape in SHAPES:
            idx, dist = _check(nb, dev, shape, rows, X, Q, 20, s)
            assert np.array_equal(idx[:, 0], target + 1), (shape, s)  # the copy, at exactly its row
            assert not dist[:, 0].any(), (shape, s)


def test_both_queries_of_a_lane_spill_in_one_tile(oracle, nb, dev):
    # queries j and j + 16 of a wave are the same cell, for all j: whatever survives for one survives for the other, in the
    # same tile, from the same lane (shape 1), into two lists
    X, Q = synth_batches(32, [4223, 256], 50)
    Q = Q.reshape(8, 2, 16, 50)
    Q[:, 1] = Q[:, 0]
    Q = Q.reshape(256, 50)
    rows = oracle.query_knn(X, Q, 20)
    for shape in SHAPES:
        _check(nb, dev, shape, rows, X, Q, 20)


def test_survivors_in_both_reference_halves_of_a_block(oracle, nb, dev):
    # rows 16 .. 31 of every tile repeat rows 0 .. 15: every neighbour comes twice, 16 rows apart -- the same lane, the same
    # register, both reference halves (shape 1: blocks a = 0 and a = 1; shape 0: groups u and u + 2); equal distances go by row
    X, Q = synth_batches(33, [4224, 256], 50)
    X = X.reshape(132, 2, 16, 50)
    X[:, 1] = X[:, 0]
    X = X.reshape(4224, 50)
    rows = oracle.query_knn(X, Q, 20)
    assert np.array_equal(rows[0][:, 1::2], rows[0][:, 0::2] + 16)
    for shape in SHAPES:
        _check(nb, dev, shape, rows, X, Q, 20)


@pytest.mark.parametrize("d", [29, 50, 61, 93, 125])  # NS = 2, 4, 4 (all 64 columns in use), 6, 8
def test_shapes(oracle, nb, dev, d):
    # references: whole slots / a ragged last tile; queries: one, a ragged wave, one past a workgroup, a second workgroup;
    # k = 36 takes the lists of 48, which the fp16 tier has up to NS = 4
    for nr in (4096, 4223):
        X, Qall = synth_batches(34, [nr, 300], d)
        for nq in (1, 255, 257, 300):
            Q = Qall[:nq]
            for k in (1, 20, 36):
                if k == 36 and d > 61:
                    continue
                rows = oracle.query_knn(X, Q, k)
                for shape in SHAPES:
                    _check(nb, dev, shape, rows, X, Q, k, (nr, nq, k))


@pytest.mark.parametrize("d,k", [(50, 20), (29, 36), (93, 20)])
def test_split_sample(oracle, nb, dev, d, k):
    # the threshold sample split into ranges (a search with few query blocks): every range leaves its lanes' lists, the
    # k-th smallest of their union is the threshold (sample_merge_kernel)
    X, Q = synth_batches(35, [4223, 300], d)
    rows = oracle.query_knn(X, Q, k)
    dev("sample_split", 4)
    for shape in SHAPES:
        _check(nb, dev, shape, rows, X, Q, k)


def test_split_ranges_share_thresholds(oracle, nb, dev):
    # 130 query blocks, every one split into two reference ranges: the ranges of a block tighten one another's thresholds
    # through the global words while they sweep, each leaves a list per query.  (A split SAMPLE needs fewer than 128 query
    # blocks: test_split_sample.)
    X, Q = synth_batches(36, [4096, 130 * 256], 50)
    rows = oracle.query_knn(X, Q, 20)
    dev("force_c", 2)
    for shape in SHAPES:
        _check(nb, dev, shape, rows, X, Q, 20)


def test_seeded_search(oracle, nat, dev):
    # findMutualNN as the merges run it: the second search only looks for the left cells some right cell lists, each within the
    # distance at which it was listed (a seed threshold per query, folded into the sampled one)
    X, Q = synth_batches(37, [4223, 300], 50)
    of, os_ = oracle.find_mutual_nn(X, Q, 20, 20)
    for shape in SHAPES:
        dev("mfma_shape", shape)
        before = _left_tier1()
        f, s = nat.find_mutual_nn(X, Q, 20, 20)
        assert np.array_equal(f, of) and np.array_equal(s, os_), shape
        f, s, _, _ = nat.mnn_average_correction(X, Q, 20)  # (the seeded form)
        assert np.array_equal(f, of) and np.array_equal(s, os_), shape
        assert _ran_shape() == shape
        assert _left_tier1() - before <= 0.05 * (2 * (4223 + 300)), shape
