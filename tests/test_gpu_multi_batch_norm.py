"""multiBatchNorm() on the device against the numpy restatement (tests/multi_batch_norm_ref.py), at the shapes where the
kernels can go wrong: one gene, odd and even gene counts (the 16-byte paths need an even one), gene counts on either side
of the 256-gene tile, batches of one cell, cells on either side of a wave's four columns and of the 256-cell chunk, more
than two chunks with a ragged last one.

Tolerances: the terms of every sum are non-negative, so a sum of n of them carries at most n * 2^-53 relative error
(1.3e-13 at n = 1200); size factors and averages are held to rtol 1e-12, the values to rtol 1e-12 / atol 1e-12."""
import functools

import numpy as np
import pytest

import batchelor_amd as bx
from batchelor_amd import multi_batch_norm as mbn
from tests import multi_batch_norm_ref as ref

pytestmark = pytest.mark.gpu

DEPTH = (1.0, 2.5, 0.6, 4.0, 1.7)
SHAPES = {                       # genes, cells per batch
    "g1": (1, (1, 3)),
    "g7": (7, (64, 65, 600)),
    "g255": (255, (3, 600)),
    "g257": (257, (65, 1, 64, 3, 600)),
    "g1000": (1000, (600, 65, 3)),
    # the chunk walk's edges, in the scalar form (odd gene counts) and the two-gene form (even ones): chunks of 1, 3, 4, 5,
    # 255, 256 and 257 cells and two chunks plus one; 257 and 258 genes put a single lane into a second tile
    "g1-chunks": (1, (4, 5, 255)),
    "g255-chunks": (255, (256, 257, 513)),
    "g2-chunks": (2, (1, 3, 4, 5)),
    "g256-chunks": (256, (255, 256, 257, 513)),
    "g258-chunks": (258, (4, 257)),
}


@functools.lru_cache(maxsize=None)
def batches(shape):
    """Negative-binomial counts with a depth factor per batch.  Every cell has a count (row 0); from 7 genes on, gene 1 is
    all zero in the second batch only (ratios 0 and inf) and gene 3 repeats gene 2 (tied ratios)."""
    G, cells = SHAPES[shape]
    rng = np.random.default_rng(7000 + G)
    mu = 2.0 ** rng.uniform(-1, 7, G)
    out = []
    for b, n in enumerate(cells):
        x = rng.negative_binomial(4, 4 / (4 + DEPTH[b] * mu[:, None]), (G, n)).astype(np.float64)
        x[0] += 1
        if G >= 7:
            x[3] = x[2]
            if b == 1:
                x[1] = 0
        x.setflags(write=False)
        out.append(x)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def given_factors(shape):
    rng = np.random.default_rng(11)
    return tuple(x.sum(axis=0) * rng.lognormal(0, 0.3, x.shape[1]) * 3.0 for x in batches(shape))


@functools.lru_cache(maxsize=None)
def expected(shape, given):
    return ref.multi_batch_norm(*batches(shape), size_factors=given_factors(shape) if given else None)


def run(shape, given=False, **kw):
    return bx.multiBatchNorm(*batches(shape), size_factors=list(given_factors(shape)) if given else None, **kw)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("given", [False, True], ids=["library", "given"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_against_the_restatement(shape, given):
    want = expected(shape, given)
    got = run(shape, given)
    B = len(batches(shape))
    assert got.ratios.shape == (B, B) and got.reference == want["reference"] + 1
    assert got.batch.tolist() == list(range(1, B + 1))
    for b in range(B):
        sf_err = np.abs(got.size_factors[b] / want["size_factors"][b] - 1).max()
        lc_err = np.abs(got.logcounts[b] - want["logcounts"][b]).max()
        print(f"{shape} given={given} batch {b}: size factors max rel {sf_err:.2e}, values max abs {lc_err:.2e}")
        np.testing.assert_allclose(got.size_factors[b], want["size_factors"][b], rtol=1e-12)
        np.testing.assert_allclose(got.logcounts[b], want["logcounts"][b], rtol=1e-12, atol=1e-12)
        assert got.logcounts[b].flags.f_contiguous
    np.testing.assert_allclose(got.averages, want["averages"], rtol=1e-12)
    np.testing.assert_allclose(got.ratios, want["ratios"], rtol=1e-12)
    assert set(got.stats["stage_ms"]) == set(mbn.STAGES)


def test_counts_without_the_log():
    want = ref.multi_batch_norm(*batches("g257"), log=False)
    got = run("g257", norm_args={"log": False})
    for b in range(5):
        np.testing.assert_allclose(got.logcounts[b], want["logcounts"][b], rtol=1e-12, atol=1e-12)
    want = ref.multi_batch_norm(*batches("g7"), pseudo_count=3.5)
    got = run("g7", norm_args={"pseudo_count": 3.5})
    for b in range(3):
        np.testing.assert_allclose(got.logcounts[b], want["logcounts"][b], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("shape", ["g7", "g257", "g1000"])
def test_the_ratio_stage_exactly(shape):
    """The restatement's step 3, fed the device's own averages, reproduces the device's ratios and reference bit for bit:
    the selection is exact.  Both parities of the number of kept genes occur over the thresholds."""
    parities = set()
    for mm in (0.5, 1.0, 3.0, 10.0):
        got = run(shape, min_mean=mm)
        aves = [np.ascontiguousarray(got.averages[:, b]) for b in range(got.averages.shape[1])]
        for f in range(len(aves)):
            for s in range(f + 1, len(aves)):
                grand = ref.grand_mean(aves[f], aves[s])
                # a precondition on the input: no gene so close to the threshold that the order of a sum decides it
                assert np.all(np.abs(grand - mm) > 1e-9 * mm), (shape, mm, f, s)
                parities.add(int((grand >= mm).sum()) % 2)
        ratios, smallest, _ = ref.rescale_size_factors(aves, mm)
        assert same_bits(got.ratios, ratios), (shape, mm)
        assert got.reference == smallest + 1
    assert parities == {0, 1}


def test_scaled_copies_on_the_device():
    """X, 2X, 3X with integer counts.  Scaling by 2 is exact in every step, so the first two batches agree bitwise.
    Scaling by 3 is not (mean(3 lib) is rounded on its own): the third batch agrees to 1e-12, not bitwise."""
    X = batches("g257")[4]
    got = bx.multiBatchNorm(X, X * 2, X * 3)
    assert got.reference == 1
    assert same_bits(got.logcounts[0], got.logcounts[1])
    np.testing.assert_allclose(got.logcounts[2], got.logcounts[0], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got.size_factors[1], 2 * got.size_factors[0], rtol=1e-12)
    np.testing.assert_allclose(got.size_factors[2], 3 * got.size_factors[0], rtol=1e-12)


def test_determinism(monkeypatch):
    first = run("g255")
    again = run("g255")
    for b in range(2):
        assert same_bits(first.logcounts[b], again.logcounts[b])
        assert same_bits(first.size_factors[b], again.size_factors[b])
    assert same_bits(first.averages, again.averages) and same_bits(first.ratios, again.ratios)
    # a permutation of the batches
    three = run("g1000")
    X = batches("g1000")
    perm = bx.multiBatchNorm(X[2], X[0], X[1])
    for i, j in enumerate([2, 0, 1]):
        assert same_bits(perm.logcounts[i], three.logcounts[j])
        assert same_bits(perm.size_factors[i], three.size_factors[j])
    assert perm.reference == [2, 0, 1].index(three.reference - 1) + 1
    # a blocked upload: 600 cells in blocks of 256, 256 and 88
    monkeypatch.setattr(mbn, "BLOCK_BYTES", 1)
    for shape, whole in (("g255", first), ("g1000", three)):
        blocked = run(shape)
        for b in range(len(whole.logcounts)):
            assert same_bits(blocked.logcounts[b], whole.logcounts[b])
            assert same_bits(blocked.size_factors[b], whole.size_factors[b])
        assert same_bits(blocked.averages, whole.averages) and same_bits(blocked.ratios, whole.ratios)
    given_whole = expected("g7", True)
    given_blocked = run("g7", True)
    for b in range(3):
        np.testing.assert_allclose(given_blocked.logcounts[b], given_whole["logcounts"][b], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("normalize_all", [False, True])
def test_subset_row(normalize_all):
    keep = np.arange(100, 0, -1)  # unsorted, as 100:1 in the reference's test
    want = ref.multi_batch_norm(*batches("g257"), subset_row=keep, normalize_all=normalize_all)
    got = run("g257", subset_row=keep, normalize_all=normalize_all)
    assert got.averages.shape == (100, 5)
    np.testing.assert_allclose(got.averages, want["averages"], rtol=1e-12)
    for b in range(5):
        assert got.logcounts[b].shape[0] == (257 if normalize_all else 100)
        np.testing.assert_allclose(got.size_factors[b], want["size_factors"][b], rtol=1e-12)
        np.testing.assert_allclose(got.logcounts[b], want["logcounts"][b], rtol=1e-12, atol=1e-12)
    # a row named twice counts twice
    twice = np.array([5, 2, 5, 7, 1])
    want = ref.multi_batch_norm(*batches("g7"), subset_row=twice, normalize_all=normalize_all, min_mean=0.1)
    got = run("g7", subset_row=twice, normalize_all=normalize_all, min_mean=0.1)
    np.testing.assert_allclose(got.averages, want["averages"], rtol=1e-12)
    for b in range(3):
        np.testing.assert_allclose(got.logcounts[b], want["logcounts"][b], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("preserve_single", [True, False])
def test_single_object(preserve_single):
    parts = batches("g257")
    combined = np.concatenate(parts, axis=1)
    labels = np.repeat(["a", "b", "c", "d", "e"], [p.shape[1] for p in parts])
    idx = np.random.default_rng(3).permutation(combined.shape[1])
    listed = bx.multiBatchNorm(*parts, names=["a", "b", "c", "d", "e"])
    assert listed.reference == "abcde"[expected("g257", False)["reference"]]
    got = bx.multiBatchNorm(combined[:, idx], batch=labels[idx], preserve_single=preserve_single)
    assert got.reference == listed.reference
    np.testing.assert_allclose(got.ratios, listed.ratios, rtol=1e-12)
    if preserve_single:
        assert got.logcounts.shape == combined.shape and got.logcounts.flags.f_contiguous
        np.testing.assert_allclose(got.logcounts, np.concatenate(listed.logcounts, axis=1)[:, idx], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(got.size_factors, np.concatenate(listed.size_factors)[idx], rtol=1e-12)
        assert np.array_equal(got.batch, labels[idx])
    else:
        assert got.batch.tolist() == ["a", "b", "c", "d", "e"]
        for lev, name in enumerate("abcde"):
            where = np.flatnonzero(labels[idx] == name)
            order = np.argsort(idx[where], kind="stable")  # the level's cells keep the caller's order
            np.testing.assert_allclose(got.logcounts[lev][:, order], listed.logcounts[lev], rtol=1e-12, atol=1e-12)
    # one level: the ratios are [[1]]
    one = bx.multiBatchNorm(parts[0], batch=np.ones(parts[0].shape[1]), preserve_single=preserve_single)
    assert one.ratios.tolist() == [[1.0]] and one.reference == 1
    lib = parts[0].sum(axis=0)
    lc = one.logcounts if preserve_single else one.logcounts[0]
    np.testing.assert_allclose(lc, np.log2(parts[0] / (lib / lib.mean()) + 1), rtol=1e-12, atol=1e-12)


def test_errors_raised_by_the_device():
    """What only the data can show comes back as an error after the kernels; the next call works."""
    A, B = (np.array(x) for x in batches("g255"))
    errors = (bx.BatchelorMI355XError, ValueError)

    def check_good():
        got = bx.multiBatchNorm(A, B)
        np.testing.assert_allclose(got.logcounts[1], expected("g255", False)["logcounts"][1], rtol=1e-12, atol=1e-12)

    bad = B.copy()
    bad[200, 450] = -1.0
    with pytest.raises(errors, match="counts should be finite and non-negative"):
        bx.multiBatchNorm(A, bad)
    check_good()
    bad = B.copy()
    bad[254, 599] = np.nan
    with pytest.raises(errors, match="counts should be finite and non-negative"):
        bx.multiBatchNorm(A, bad, size_factors=[None, np.ones(600)])
    check_good()
    bad = A.copy()
    bad[:, 2] = 0
    with pytest.raises(errors, match="size factors should be positive"):
        bx.multiBatchNorm(bad, B)
    check_good()
    with pytest.raises(errors, match="median ratio of averages between batches is not finite"):
        bx.multiBatchNorm(A, B, min_mean=1e9)
    check_good()
