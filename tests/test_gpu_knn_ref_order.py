"""Ordered references of the fp16 kNN tier (csrc/knn_order.hpp, knn_order.hip): the reference image is written in ascending
order of |r - c_Q|^2 (256 buckets, stable), the candidate pass lists image rows and the FP64 re-rank turns them back into
reference positions.  The testing hook "ref_order" forces the order off (0: the path as it was) and on (1: wherever the fp16
tier runs); the counters "knn_ordered_searches" / "knn_unordered_searches" say which path ran.  Under both settings the bar
is the usual one -- indices equal to the oracle's, distances bitwise -- and on the ordinary cases the fp16 tier must have
done the work: at most 5 % of a case's queries may leave it.  A lost or doubled image row, or a wrong translation, does not
survive the exact re-rank as a wrong distance but as a missing neighbour or a failed certificate, so both are asserted."""
import numpy as np
import pytest

from tests.conftest import synth_batches
from tests.find_knn_ref import find_knn_ref

pytestmark = pytest.mark.gpu
SETTINGS = (0, 1)


@pytest.fixture(scope="module")
def nb():
    from batchelor_amd import neighbors
    return neighbors


@pytest.fixture(scope="module")
def nat():
    from batchelor_amd import natives
    return natives


@pytest.fixture(scope="module")
def bx():
    import batchelor_amd
    return batchelor_amd


def _get(name):
    from batchelor_amd import _lib
    return _lib.dev_get(name)


def _left_tier1():
    return _get("knn_exact_fallbacks") + _get("knn_tier2_queries")


class _Ran:
    """The searches between enter and exit: how many ran ordered / unordered, how many queries left the fp16 tier."""

    def __enter__(self):
        self.o0, self.u0, self.l0 = _get("knn_ordered_searches"), _get("knn_unordered_searches"), _left_tier1()
        return self

    def __exit__(self, *exc):
        self.ordered = _get("knn_ordered_searches") - self.o0
        self.unordered = _get("knn_unordered_searches") - self.u0
        self.left = _left_tier1() - self.l0
        return False


def _forced_path_ran(setting, ran, what):
    if setting == 1:
        assert ran.ordered >= 1, (what, ran.ordered, ran.unordered)  # (a tier behind the fp16 one is never ordered)
    else:
        assert ran.ordered == 0 and ran.unordered >= 1, (what, ran.ordered, ran.unordered)


def _check_query(nb, dev, oracle_rows, X, Q, k, what, cap=True):
    oi, od = oracle_rows
    for setting in SETTINGS:
        dev("ref_order", setting)
        with _Ran() as ran:
            idx, dist = nb.query_knn(X, Q, k)
        _forced_path_ran(setting, ran, what)
        assert np.array_equal(idx, oi), (setting, what)
        assert np.array_equal(dist, od), (setting, what)
        print(f"ref_order={setting} {what}: {ran.left} of {Q.shape[0]} queries left the fp16 tier")
        if cap:
            assert ran.left <= 0.05 * Q.shape[0], (setting, what, ran.left)


@pytest.mark.parametrize("d", [3, 50, 61])
def test_shapes(oracle, nb, dev, d):
    # A: a reference with a sample, with several slots, with a padded tail; B: one query, query sets with tail blocks (hence
    # several reference ranges); C: the shortest rows, the bench's, the longest the 64-column image holds
    for nr in (4096, 4100, 8229):
        X, Qall = synth_batches(41, [nr, 700], d)
        rows_all = oracle.query_knn(X, Qall, 20)
        for nq in (1, 300, 700):
            rows = (rows_all[0][:nq], rows_all[1][:nq])
            _check_query(nb, dev, rows, X, Qall[:nq], 20, (d, nr, nq))


def test_offset_and_centred_queries(oracle, nb, dev):
    # E: queries three times the references' spread away (every key large, the near rows a thin slice), and queries centred on
    # the references (c_Q = the references' mean: the keys are the norms)
    (X,) = synth_batches(42, [8229], 50)
    rng = np.random.Generator(np.random.PCG64(4242))
    spread = X.std(axis=0)
    centred = X.mean(axis=0) + rng.standard_normal((300, 50)) * spread
    offset = centred + 3.0 * spread
    for name, Q in (("centred", centred), ("offset", offset)):
        _check_query(nb, dev, oracle.query_knn(X, Q, 20), X, Q, 20, name)


def test_identical_references(oracle, nb, dev):
    # F: all keys equal -- one bucket, the identity order; every distance ties, the lowest positions win
    X = np.tile(np.linspace(-1.0, 1.0, 50), (4100, 1))
    (Q,) = synth_batches(43, [300], 50)
    rows = oracle.query_knn(X, Q, 20)
    assert np.array_equal(rows[0], np.tile(np.arange(1, 21), (300, 1)))
    _check_query(nb, dev, rows, X, Q, 20, "identical", cap=False)


def test_lattice_ties_across_buckets(oracle, nb, dev):
    # G: integer-lattice coordinates in shuffled order: a query on a lattice point has many references at exactly the same
    # distance, and they lie at different distances from the queries' centre, i.e. in different buckets -- the image order of
    # equal candidates is not their position order, the result's must be
    g = np.arange(17.0)
    X = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)  # 4 913 points
    rng = np.random.Generator(np.random.PCG64(44))
    X = X[rng.permutation(X.shape[0])]
    Q = X[rng.choice(X.shape[0], 300, replace=False)]
    rows = oracle.query_knn(X, Q, 20)
    assert (np.diff(rows[1], axis=1) == 0).mean() > 0.5  # ties are the rule here
    _check_query(nb, dev, rows, X, Q, 20, "lattice", cap=False)


def test_every_row_is_its_own_neighbour(nb, dev):
    # H: a lost or a doubled image row shows as a row that does not come back as its own nearest neighbour
    (X,) = synth_batches(45, [4100], 50)
    want = np.arange(1, 4101, dtype=np.int32)[:, None]
    for setting in SETTINGS:
        dev("ref_order", setting)
        with _Ran() as ran:
            idx, dist = nb.query_knn(X, X, 1)
        _forced_path_ran(setting, ran, "self")
        assert np.array_equal(idx, want), setting
        assert not dist.any(), setting
        assert ran.left <= 0.05 * 4100, (setting, ran.left)


def test_find_knn_with_repeated_query_rows(oracle, nb, dev):
    # D (queries through a row list, a row named twice), and find_knn's own path
    (X,) = synth_batches(46, [4100], 50)
    rng = np.random.Generator(np.random.PCG64(46))
    sub = rng.permutation(4100)[:300] + 1
    sub[100:110] = sub[:10]
    oi, od = find_knn_ref(oracle, X, 20, sub)
    for setting in SETTINGS:
        dev("ref_order", setting)
        with _Ran() as ran:
            idx, dist = nb.find_knn(X, 20, subset=sub)
        _forced_path_ran(setting, ran, "find_knn")
        assert np.array_equal(idx, oi) and np.array_equal(dist, od), setting
        assert ran.left <= 0.05 * 300, (setting, ran.left)


def test_find_mutual_nn(oracle, nat, dev):
    # both searches of findMutualNN, the second one seeded
    X, Q = synth_batches(47, [4100, 700], 50)
    of, os_ = oracle.find_mutual_nn(X, Q, 20, 20)
    for setting in SETTINGS:
        dev("ref_order", setting)
        with _Ran() as ran:
            f, s = nat.find_mutual_nn(X, Q, 20, 20)
        _forced_path_ran(setting, ran, "find_mutual_nn")
        assert np.array_equal(f, of) and np.array_equal(s, os_), setting
        assert ran.left <= 0.05 * (4100 + 700), (setting, ran.left)


def test_two_batch_merge_with_restriction(oracle, bx, dev):
    # D (references AND queries through row lists, a row named twice) in one two-batch merge on an engine of its own: the
    # merge's three searches, the engine's node means as the centres.  The queries that leave the fp16 tier are the ENGINE's
    # (profile / profile_detail; the counters of _left_tier1 belong to the single primitives): a wrong gather through
    # ref_rows o img_src, or a wrong translation back, would send most queries to the FP64 paths and still give the right
    # pairs.  The merge asks at least 4 100 (first search) + 4 200 (tricube search) queries; the second search's are on top.
    B = synth_batches(48, [4300, 4200], 50)
    rng = np.random.Generator(np.random.PCG64(48))
    keep = [rng.permutation(4300)[:4100] + 1, rng.permutation(4200)[:4100] + 1]
    keep[0][7] = keep[0][3]
    keep[1][9] = keep[1][5]
    ref = oracle.reduced_mnn(*B, restrict=keep)
    outs = []
    for setting in SETTINGS:
        dev("ref_order", setting)
        eng = bx.MnnEngine()
        try:
            eng.upload(B, restrict=keep)
            with _Ran() as ran:
                eng.run(k=20)
            out = eng.download()
            left = eng.profile()["exact_fallbacks"] + eng.profile_detail()["tier2_queries"]
            retries = eng.profile_detail()["optimistic_retries"]
        finally:
            eng.close()
        _forced_path_ran(setting, ran, "two-batch merge")
        if setting == 1:
            assert ran.unordered == 0 and ran.ordered >= 3, (ran.ordered, ran.unordered)
        print(f"ref_order={setting} two-batch merge: {left} queries left the fp16 tier, {retries} optimistic retries")
        assert left <= 0.05 * (4100 + 4200), (setting, left)
        for (ol, orr), (rl, rr) in zip(out.merge_info.pairs, ref.merge_info.pairs):
            assert np.array_equal(ol, rl) and np.array_equal(orr, rr), setting
        np.testing.assert_allclose(out.corrected, ref.corrected, rtol=1e-5, atol=1e-12)
        outs.append(out.corrected)
    assert np.array_equal(outs[0], outs[1])  # the same neighbours, hence the same bits


def test_default_rule(oracle, nb, dev):
    # no hook set (-1): an fp16 search whose reference has a threshold sample (nr >= 4 096) runs ordered, a smaller one does
    # not (it is still the fp16 tier's: nr > 64), nor does any with the hook at 0; with the sample switched off nothing is
    # ordered either -- the order serves the sample first
    Xall, Q = synth_batches(49, [4096, 300], 50)
    for nr, knob, want in ((4096, None, True), (4095, None, False), (4096, ("sample", 0), False),
                           (4096, ("ref_order", 0), False)):
        X = Xall[:nr]
        rows = oracle.query_knn(X, Q, 20)
        dev("reset", 0)
        if knob:
            dev(*knob)
        with _Ran() as ran:
            idx, dist = nb.query_knn(X, Q, 20)
        assert np.array_equal(idx, rows[0]) and np.array_equal(dist, rows[1]), (nr, knob)
        assert (ran.ordered, ran.unordered) == ((1, 0) if want else (0, 1)), (nr, knob, ran.ordered, ran.unordered)
        if knob is None:
            assert ran.left <= 0.05 * 300, (nr, ran.left)
