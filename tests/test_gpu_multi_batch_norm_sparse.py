"""multiBatchNorm() on sparse counts against the dense path (bit for bit) and the numpy restatement
(tests/multi_batch_norm_ref.py), at the shapes where the sparse kernels can go wrong: one gene, gene counts around the
256-thread stride and one above the 4096-gene tile of the per-gene sums, batches of one cell, cells on either side of a
wave's four columns and of the 256-cell chunk, more than two chunks with a ragged last one.

The counts are negative-binomial integers with low means, so most entries are zero and library sizes are exact in any
order: the sparse path then divides by the dense path's size factors, and since leaving out a term +0 changes no bit of a
sum of non-negative terms taken in the same order, every comparison with the dense path is bitwise.

Tolerances against the restatement are the dense test's: the terms of every sum are non-negative, so a sum of n of them
carries at most n * 2^-53 relative error; size factors, averages and ratios are held to rtol 1e-12, the values to rtol
1e-12 / atol 1e-12."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import batchelor_amd as bx
from batchelor_amd import _lib
from batchelor_amd import multi_batch_norm as mbn
from tests import multi_batch_norm_ref as ref

pytestmark = pytest.mark.gpu

DEPTH = (1.0, 2.5, 0.6, 4.0, 1.7)
SHAPES = {                       # genes, cells per batch
    "g1": (1, (1, 3)),
    "g7": (7, (64, 65, 600)),
    "g257": (257, (255, 256, 257, 1, 600)),
    "g1000": (1000, (600, 65, 3)),
    "g4097": (4097, (3, 257)),   # one gene more than the tile of the per-gene sums
}
ERRORS = (bx.BatchelorMI355XError, ValueError)


@functools.lru_cache(maxsize=None)
def dense(shape):
    """Integer counts, mu = 2^U(-6, 3) times a depth per batch.  Every cell has a count (row 0); from 7 genes on, gene 1
    is all zero in the second batch only."""
    G, cells = SHAPES[shape]
    rng = np.random.default_rng(9000 + G)
    mu = 2.0 ** rng.uniform(-6, 3, G)
    out = []
    for b, n in enumerate(cells):
        x = rng.negative_binomial(2, 2 / (2 + DEPTH[b] * mu[:, None]), (G, n)).astype(np.float64)
        x[0] += 1
        if G >= 7 and b == 1:
            x[1] = 0
        x.setflags(write=False)
        out.append(x)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def sparse(shape):
    return tuple(sp.csc_matrix(x) for x in dense(shape))


@functools.lru_cache(maxsize=None)
def given_factors(shape):
    rng = np.random.default_rng(11)
    return tuple(x.sum(axis=0) * rng.lognormal(0, 0.3, x.shape[1]) * 3.0 for x in dense(shape))


@functools.lru_cache(maxsize=None)
def dense_result(shape, given=False):
    return bx.multiBatchNorm(*dense(shape), size_factors=list(given_factors(shape)) if given else None)


def run(shape, given=False, **kw):
    return bx.multiBatchNorm(*sparse(shape), size_factors=list(given_factors(shape)) if given else None, **kw)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def as_dense(m):
    return m.toarray() if sp.issparse(m) else m


def assert_same_result(got, want):
    """Every number of two results, bit for bit; either may hold sparse matrices where the other holds dense ones."""
    assert same_bits(got.averages, want.averages) and same_bits(got.ratios, want.ratios)
    assert got.reference == want.reference and np.array_equal(got.batch, want.batch)
    if isinstance(want.logcounts, list):
        assert len(got.logcounts) == len(want.logcounts)
        for b in range(len(want.logcounts)):
            assert same_bits(got.size_factors[b], want.size_factors[b]), b
            assert same_bits(as_dense(got.logcounts[b]), as_dense(want.logcounts[b])), b
    else:
        assert same_bits(got.size_factors, want.size_factors)
        assert same_bits(as_dense(got.logcounts), as_dense(want.logcounts))


@pytest.mark.parametrize("given", [False, True], ids=["library", "given"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_bitwise_against_the_dense_path(shape, given):
    got = run(shape, given)
    assert_same_result(got, dense_result(shape, given))
    for lc, x in zip(got.logcounts, sparse(shape)):
        assert sp.issparse(lc) and lc.format == "csc" and lc.shape == x.shape
        assert np.array_equal(lc.indptr, x.indptr) and np.array_equal(lc.indices, x.indices)
        assert lc.indices is not x.indices  # the caller's arrays are not lent out
    assert set(got.stats["stage_ms"]) == set(mbn.STAGES)


def assert_close_to_restatement(got, want):
    for b in range(len(got.logcounts)):
        np.testing.assert_allclose(got.size_factors[b], want["size_factors"][b], rtol=1e-12)
        np.testing.assert_allclose(as_dense(got.logcounts[b]), want["logcounts"][b], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got.averages, want["averages"], rtol=1e-12)
    np.testing.assert_allclose(got.ratios, want["ratios"], rtol=1e-12)
    assert got.reference == want["reference"] + 1


@pytest.mark.parametrize("given", [False, True], ids=["library", "given"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_against_the_restatement(shape, given):
    want = ref.multi_batch_norm(*dense(shape), size_factors=given_factors(shape) if given else None)
    assert_close_to_restatement(run(shape, given), want)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_non_integer_counts(shape):
    """Every stored count times a lognormal factor: the library sizes now depend on the order of their sums and need not
    have the dense path's bits; the restatement's tolerances hold."""
    rng = np.random.default_rng(13)
    mats = []
    for x in sparse(shape):
        y = x.copy()
        y.data = y.data * rng.lognormal(0, 0.5, y.nnz)
        mats.append(y)
    want = ref.multi_batch_norm(*[m.toarray() for m in mats])
    assert_close_to_restatement(bx.multiBatchNorm(*mats), want)


def test_other_value_modes():
    # without the log a zero stays a zero: sparse
    got = run("g257", norm_args={"log": False})
    assert all(sp.issparse(lc) for lc in got.logcounts)
    assert_same_result(got, bx.multiBatchNorm(*dense("g257"), norm_args={"log": False}))
    # log2(0 + 3.5) is not 0: dense, filled with the device's own image of a zero
    got = run("g257", norm_args={"pseudo_count": 3.5})
    assert all(isinstance(lc, np.ndarray) and lc.flags.f_contiguous for lc in got.logcounts)
    assert_same_result(got, bx.multiBatchNorm(*dense("g257"), norm_args={"pseudo_count": 3.5}))
    got = run("g7", norm_args={"pseudo_count": 1})
    assert all(sp.issparse(lc) for lc in got.logcounts)
    assert_same_result(got, dense_result("g7"))


@pytest.mark.parametrize("normalize_all", [False, True])
def test_subset_row(normalize_all):
    keep = np.arange(100, 0, -1)  # not ascending
    got = run("g257", subset_row=keep, normalize_all=normalize_all)
    assert got.averages.shape == (100, 5) and got.logcounts[0].shape[0] == (257 if normalize_all else 100)
    assert_same_result(got, bx.multiBatchNorm(*dense("g257"), subset_row=keep, normalize_all=normalize_all))
    twice = np.array([5, 2, 5, 7, 1])  # a row named twice counts twice
    got = run("g7", subset_row=twice, normalize_all=normalize_all, min_mean=0.1)
    assert_same_result(got, bx.multiBatchNorm(*dense("g7"), subset_row=twice, normalize_all=normalize_all, min_mean=0.1))
    # a subset that reaches over the tile edge of the per-gene sums
    over = np.array([4097, 1, 4096, 2, 4097])
    got = run("g4097", subset_row=over, normalize_all=normalize_all, min_mean=0.0)
    assert_same_result(got, bx.multiBatchNorm(*dense("g4097"), subset_row=over, normalize_all=normalize_all, min_mean=0.0))


@pytest.mark.parametrize("preserve_single", [True, False])
def test_single_object(preserve_single):
    parts = dense("g257")
    combined = np.concatenate(parts, axis=1)
    labels = np.repeat(["a", "b", "c", "d", "e"], [p.shape[1] for p in parts])
    idx = np.random.default_rng(3).permutation(combined.shape[1])
    want = bx.multiBatchNorm(combined[:, idx], batch=labels[idx], preserve_single=preserve_single)
    got = bx.multiBatchNorm(sp.csr_matrix(combined[:, idx]), batch=labels[idx], preserve_single=preserve_single)
    assert_same_result(got, want)
    if preserve_single:
        assert sp.issparse(got.logcounts) and got.logcounts.format == "csc" and got.logcounts.shape == combined.shape
    else:
        assert got.batch.tolist() == ["a", "b", "c", "d", "e"]
    sfs = np.concatenate(given_factors("g257"))[idx]
    want = bx.multiBatchNorm(combined[:, idx], batch=labels[idx], size_factors=sfs, preserve_single=preserve_single)
    got = bx.multiBatchNorm(sp.csc_matrix(combined[:, idx]), batch=labels[idx], size_factors=sfs,
                            preserve_single=preserve_single)
    assert_same_result(got, want)


def test_determinism(monkeypatch):
    first, again = run("g257"), run("g257")
    assert_same_result(again, first)
    for a, b in zip(first.logcounts, again.logcounts):
        assert same_bits(a.data, b.data)
    # a permutation of the batches
    three = run("g1000")
    X = sparse("g1000")
    perm = bx.multiBatchNorm(X[2], X[0], X[1])
    for i, j in enumerate([2, 0, 1]):
        assert same_bits(perm.logcounts[i].data, three.logcounts[j].data)
        assert same_bits(perm.size_factors[i], three.size_factors[j])
    assert perm.reference == [2, 0, 1].index(three.reference - 1) + 1
    # a blocked upload: 600 cells in blocks of 256, 256 and 88
    monkeypatch.setattr(mbn, "BLOCK_BYTES", 1)
    for shape, whole in (("g257", first), ("g1000", three)):
        assert_same_result(run(shape), whole)
    assert_same_result(run("g7", True), dense_result("g7", True))


def test_an_upload_block_without_entries_gives_the_bits_of_a_whole_upload(monkeypatch):
    """7 genes x 600 cells whose cells 256-511 hold no entry (size factors given): BLOCK_BYTES = 1 uploads the cells in
    blocks of 256, 256 and 88, the middle one without a stored entry; the default uploads them in one block."""
    A, B, C = (np.array(x) for x in dense("g7"))
    C[:, 256:512] = 0
    X = [sp.csc_matrix(x) for x in (A, B, C)]
    assert X[2].shape == (7, 600) and X[2].indptr[256] == X[2].indptr[512] and X[2].indptr[256] > 0 and X[2].nnz > X[2].indptr[512]
    sfs = list(given_factors("g7"))
    whole = bx.multiBatchNorm(*X, size_factors=sfs)
    monkeypatch.setattr(mbn, "BLOCK_BYTES", 1)
    blocked = bx.multiBatchNorm(*X, size_factors=sfs)
    assert_same_result(blocked, whole)
    for a, b in zip(blocked.logcounts, whole.logcounts):
        assert sp.issparse(a) and same_bits(a.data, b.data) and np.array_equal(a.indptr, b.indptr)
    assert_same_result(whole, bx.multiBatchNorm(A, B, C, size_factors=sfs))


def test_structure():
    A, B, C = (np.array(x) for x in dense("g7"))
    # cells without a stored entry in the middle of a batch and at its end (size factors given)
    C[:, 250:270] = 0
    C[:, 599] = 0
    sfs = list(given_factors("g7"))
    got = bx.multiBatchNorm(sp.csc_matrix(A), sp.csc_matrix(B), sp.csc_matrix(C), size_factors=sfs)
    assert got.logcounts[2].indptr[250] == got.logcounts[2].indptr[270] and got.logcounts[2][:, 599].nnz == 0
    assert_same_result(got, bx.multiBatchNorm(A, B, C, size_factors=sfs))
    # stored zeros are values like any other: they come back as stored entries with the image of a zero
    A, B, C = sparse("g7")
    Z = C.copy()
    hit = np.flatnonzero(Z.indices != 0)[::3]
    Z.data[hit] = 0.0
    want = bx.multiBatchNorm(A.toarray(), B.toarray(), Z.toarray())
    got = bx.multiBatchNorm(A, B, Z)
    assert np.array_equal(got.logcounts[2].indices, Z.indices) and np.array_equal(got.logcounts[2].indptr, Z.indptr)
    assert np.all(got.logcounts[2].data[hit] == 0.0) and got.logcounts[2].nnz == Z.nnz
    assert_same_result(got, want)
    got = bx.multiBatchNorm(A, B, Z, norm_args={"pseudo_count": 3.5})
    assert_same_result(got, bx.multiBatchNorm(A.toarray(), B.toarray(), Z.toarray(), norm_args={"pseudo_count": 3.5}))
    # COO with every entry stored as two halves
    halves = []
    for x in (A, B, C):
        h = x.tocoo()
        halves.append(sp.coo_matrix((np.concatenate([h.data / 2, h.data / 2]),
                                     (np.concatenate([h.row, h.row]), np.concatenate([h.col, h.col]))), shape=h.shape))
    assert_same_result(bx.multiBatchNorm(*halves), dense_result("g7"))


def test_errors_raised_by_the_device():
    """What only the data can show comes back as an error after the kernels, with the dense path's texts; the next call
    works."""
    A, B = sparse("g257")[:2]
    want = bx.multiBatchNorm(*dense("g257")[:2])

    def check_good():
        assert_same_result(bx.multiBatchNorm(A, B), want)

    bad = B.copy()
    bad.data[bad.nnz // 2] = -1.0
    with pytest.raises(ERRORS, match="counts should be finite and non-negative"):
        bx.multiBatchNorm(A, bad)
    check_good()
    bad = B.copy()
    bad.data[bad.nnz - 1] = np.nan
    with pytest.raises(ERRORS, match="counts should be finite and non-negative"):
        bx.multiBatchNorm(A, bad, size_factors=[None, np.ones(256)])
    check_good()
    bad = sp.csc_matrix(np.where(np.arange(255) == 2, 0.0, A.toarray()))
    with pytest.raises(ERRORS, match="size factors should be positive"):
        bx.multiBatchNorm(bad, B)
    check_good()
    with pytest.raises(ERRORS, match="median ratio of averages between batches is not finite"):
        bx.multiBatchNorm(A, B, min_mean=1e9)
    check_good()


@pytest.mark.parametrize("indices,message", [([0, 5, 1, 2], "row index is outside"),
                                             ([3, 1, 1, 2], "strictly ascending"),
                                             ([2, 2, 1, 2], "strictly ascending"),
                                             ([0, -1, 1, 2], "row index is outside")])
def test_patterns_only_the_device_sees(indices, message):
    """Through the C ABI, past the front end's canonical form: a block whose row indices are out of range or not strictly
    ascending is reported by the run -- the kernels leave such entries out, they never address memory with them --, the
    handle can be destroyed and the next ordinary call works."""
    L = _lib.lib()
    i32, i64, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    L.bmx_norm_sparse_destroy.argtypes = [ctypes.c_void_p]
    L.bmx_norm_sparse_destroy.restype = None
    h = ctypes.c_void_p()
    _lib.check(L.bmx_norm_sparse_create(i32(0), i32(5), None, i64(-1), ctypes.byref(h)))
    try:
        indptr = np.array([0, 2, 3, 4], dtype=np.int64)
        idx = np.array(indices, dtype=np.int32)
        data = np.ones(4)
        _lib.check(L.bmx_norm_sparse_begin_batch(h, i64(3), None, i64(4)))
        _lib.check(L.bmx_norm_sparse_add_block(h, i64(3), indptr.ctypes.data_as(_lib.c_i64p), _lib.i32p(idx),
                                               _lib.f64p(data), i64(4)))
        out = np.zeros(4)
        outs = (ctypes.c_void_p * 1)(out.ctypes.data)
        rc = L.bmx_norm_sparse_run(h, f64(1), i32(1), f64(1), outs, None, None, None, None, None)
        assert rc != 0 and message in L.bmx_last_error().decode()
    finally:
        L.bmx_norm_sparse_destroy(h)
    assert_same_result(run("g1"), dense_result("g1"))
