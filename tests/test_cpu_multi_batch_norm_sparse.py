"""multiBatchNorm() for sparse counts without a GPU: what the front end does to scipy.sparse inputs on the host (canonical
CSC, column blocks), the device-free check of a block (bmx_norm_check_sparse_block), the null-handle refusals of the
bmx_norm_sparse_* entries, and the argument errors, which are the dense path's and are raised before any device work."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import batchelor_amd as bx
from batchelor_amd import _lib
from batchelor_amd import multi_batch_norm as mbn


def dense_counts(seed, genes=40, cells=30):
    rng = np.random.default_rng(seed)
    mu = 2.0 ** rng.uniform(-6, 3, genes)
    return rng.negative_binomial(2, 2 / (2 + mu[:, None]), (genes, cells)).astype(np.float64)


def arrays(c):
    return c.indptr.tolist(), c.indices.tolist(), c.data.tolist()


def test_canonical_csc_from_every_form():
    d = dense_counts(1)
    d[3, 4] = d[7, 4] = 2.0
    want = sp.csc_matrix(d)
    want.sort_indices()
    # COO whose entries are split into two halves that sum to the matrix: every stored entry is a duplicate pair
    half = sp.coo_matrix(d / 2)
    rng = np.random.default_rng(2)
    order = rng.permutation(2 * half.nnz)
    coo = sp.coo_matrix((np.concatenate([half.data, half.data])[order],
                         (np.concatenate([half.row, half.row])[order], np.concatenate([half.col, half.col])[order])),
                        shape=d.shape)
    before = (coo.row.copy(), coo.col.copy(), coo.data.copy())
    got, owned = mbn.canonical_csc(coo)
    assert owned and arrays(got) == arrays(want)
    assert all(np.array_equal(a, b) for a, b in zip(before, (coo.row, coo.col, coo.data)))
    # CSR, integer values
    csr = sp.csr_matrix(d.astype(np.int64))
    got, owned = mbn.canonical_csc(csr)
    assert owned and arrays(got) == arrays(want)
    assert got.data.dtype == np.float64 and got.indices.dtype == np.int32
    # CSC with the rows of every column reversed: sorted on a copy
    rev_idx, rev_dat = want.indices.copy(), want.data.copy()
    for c in range(d.shape[1]):
        a, b = want.indptr[c], want.indptr[c + 1]
        rev_idx[a:b], rev_dat[a:b] = want.indices[a:b][::-1], want.data[a:b][::-1]
    unsorted = sp.csc_matrix((rev_dat, rev_idx, want.indptr.copy()), shape=d.shape)
    kept = unsorted.indices.copy()
    got, owned = mbn.canonical_csc(unsorted)
    assert owned and arrays(got) == arrays(want)
    assert np.array_equal(unsorted.indices, kept) and np.array_equal(unsorted.data, rev_dat)
    # canonical already: taken as it is, and said to be the caller's
    got, owned = mbn.canonical_csc(want)
    assert not owned and got.indices is want.indices
    # a sparse array (not a matrix), and stored zeros, which stay
    arr = sp.csr_array(d)
    assert arrays(mbn.canonical_csc(arr)[0]) == arrays(want)
    zeros = sp.csc_matrix((np.array([0.0, 3.0, 0.0]), np.array([1, 2, 0]), np.array([0, 2, 2, 3])), shape=(3, 3))
    got, _ = mbn.canonical_csc(zeros)
    assert got.nnz == 3 and got.data.tolist() == [0.0, 3.0, 0.0]


def test_column_blocks():
    d = dense_counts(3, genes=9, cells=23)
    d[:, 8:17] = 0  # cells 8..16 are empty: the block [8, 16) holds empty columns only
    d[:, 22] = 0    # and the last column
    c, _ = mbn.canonical_csc(sp.csc_matrix(d))
    blocks = list(mbn.csc_blocks(c, 8))
    assert [b[0] for b in blocks] == [8, 8, 7]
    for i, (m, indptr, indices, data) in enumerate(blocks):
        want = sp.csc_matrix(d[:, 8 * i:8 * i + m])
        want.sort_indices()
        assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == np.float64
        assert (indptr.tolist(), indices.tolist(), data.tolist()) == arrays(want)
    assert blocks[1][1].tolist() == [0] * 9 and blocks[1][2].size == 0
    whole, = mbn.csc_blocks(c, 256)
    assert whole[0] == 23 and (whole[1].tolist(), whole[2].tolist(), whole[3].tolist()) == arrays(c)


def test_check_sparse_block():
    L = _lib.lib()
    i64 = ctypes.c_int64

    def check(n, filled, m, indptr, indices, data, nnz):
        ip = None if indptr is None else np.asarray(indptr, dtype=np.int64)
        ix = None if indices is None else np.asarray(indices, dtype=np.int32)
        dv = None if data is None else np.asarray(data, dtype=np.float64)
        rc = L.bmx_norm_check_sparse_block(i64(n), i64(filled), i64(m), None if ip is None else ip.ctypes.data_as(_lib.c_i64p),
                                           None if ix is None else _lib.i32p(ix), None if dv is None else _lib.f64p(dv),
                                           i64(nnz))
        return "" if rc == 0 else L.bmx_last_error().decode()

    good = ([0, 2, 2, 3], [0, 4, 1], [1.0, 2.0, 3.0])
    assert check(10, 7, 3, *good, 3) == ""
    assert check(3, 0, 3, [0, 0, 0, 0], None, None, 0) == ""   # empty columns only
    assert "'indptr' is missing" in check(10, 0, 3, None, good[1], good[2], 3)
    assert "missing" in check(10, 0, 3, good[0], None, good[2], 3)
    assert "missing" in check(10, 0, 3, good[0], good[1], None, 3)
    assert "does not start at 0" in check(10, 0, 3, [1, 2, 2, 3], good[1], good[2], 3)
    assert "decreases" in check(10, 0, 3, [0, 2, 1, 3], good[1], good[2], 3)
    assert "does not end at" in check(10, 0, 3, *good, 4)
    assert "negative" in check(10, 0, 3, *good, -1)
    assert "does not fit" in check(10, 8, 3, *good, 3)
    assert "does not fit" in check(10, 0, 0, *good, 3)


def test_sparse_entries_refuse_a_null_handle():
    L = _lib.lib()
    i32, i64, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    h = ctypes.c_void_p()
    rows = np.array([1, 5], dtype=np.int32)
    assert L.bmx_norm_sparse_create(i32(0), i32(0), None, i64(-1), ctypes.byref(h)) != 0
    assert "gene" in L.bmx_last_error().decode()
    assert L.bmx_norm_sparse_create(i32(0), i32(4), _lib.i32p(rows), i64(2), ctypes.byref(h)) != 0
    assert "out of range" in L.bmx_last_error().decode()
    assert not h
    for call in (lambda: L.bmx_norm_sparse_begin_batch(None, i64(1), None, i64(0)),
                 lambda: L.bmx_norm_sparse_add_block(None, i64(1), None, None, None, i64(0)),
                 lambda: L.bmx_norm_sparse_run(None, f64(1), i32(1), f64(1), None, None, None, None, None, None),
                 lambda: L.bmx_norm_sparse_stage_ms(None, None)):
        assert call() != 0
        assert L.bmx_last_error()


def test_argument_errors_are_the_dense_path_s():
    f = bx.multiBatchNorm
    B1, B2 = sp.csc_matrix(dense_counts(4, 50, 20)), sp.csr_matrix(dense_counts(5, 50, 30))
    with pytest.raises(TypeError, match="all sparse or all dense"):
        f(B1, B2.toarray())
    with pytest.raises(TypeError, match="all sparse or all dense"):
        f(B1.toarray(), B2)
    with pytest.raises(ValueError, match="'batch' must be specified if '...' has only one object"):
        f(B1)
    with pytest.raises(ValueError, match="number of rows is not the same across batches"):
        f(B1[:10], B2)
    with pytest.raises(ValueError, match="'downsample'"):
        f(B1, B2, norm_args={"downsample": True})
    with pytest.raises(ValueError, match="pseudo_count"):
        f(B1, B2, norm_args={"pseudo_count": np.inf})
    with pytest.raises(ValueError, match="selects no genes"):
        f(B1, B2, subset_row=[])
    with pytest.raises(ValueError, match="subset indices out of range"):
        f(B1, B2, subset_row=[0, 1])
    with pytest.raises(ValueError, match="at least one cell"):
        f(B1, B2[:, :0])
    with pytest.raises(ValueError, match="one vector per batch"):
        f(B1, B2, size_factors=[np.ones(20)])
    with pytest.raises(ValueError, match="one value per cell"):
        f(B1, B2, size_factors=[np.ones(20), np.ones(3)])
    with pytest.raises(ValueError, match="one value per cell"):
        f(B1, batch=np.repeat([1, 2], 10), size_factors=np.ones(3))
    with pytest.raises(ValueError, match="should be equal to number of cells"):
        f(B1, batch=np.ones(5))
    with pytest.raises(ValueError, match="size factors should be positive"):
        f(B1, B2, size_factors=[np.zeros(20), None])
    # the other functions still take dense matrices only
    for g in (bx.rescaleBatches, bx.regressBatches):
        with pytest.raises(TypeError, match="sparse"):
            g(B1, B2)
