"""multiBatchNorm() without a GPU: the numpy restatement (tests/multi_batch_norm_ref.py) against the identities the
reference's own tests state (tests/testthat/test-multi-norm.R), and the argument errors of the product function and of
the bmx_norm_check_* entries, which are raised before any device work."""
import ctypes

import numpy as np
import pytest

from tests import multi_batch_norm_ref as ref


def counts(seed, genes=200, cells=100):
    """test-multi-norm.R:5-12: negative-binomial counts around gene means that span the min_mean thresholds."""
    rng = np.random.default_rng(seed)
    mu = 2.0 ** rng.uniform(-2, 8, genes)
    return rng.negative_binomial(5, 5 / (5 + mu[:, None]), (genes, cells)).astype(np.float64)


def test_scaled_copies_normalize_to_the_same_values():
    # test-multi-norm.R: X, 2X, 3X
    X = counts(1000)
    out = ref.multi_batch_norm(X, X * 2, X * 3)
    for lc in out["logcounts"][1:]:
        np.testing.assert_allclose(lc, out["logcounts"][0], rtol=1e-12, atol=1e-12)
    sf = out["size_factors"]
    np.testing.assert_allclose(sf[1], 2 * sf[0], rtol=1e-12)
    np.testing.assert_allclose(sf[2], 3 * sf[0], rtol=1e-12)
    assert out["reference"] == 0
    np.testing.assert_allclose(out["ratios"], [[1, 2, 3], [1 / 2, 1, 3 / 2], [1 / 3, 2 / 3, 1]], rtol=1e-12)
    # the result follows a permutation of the batches
    perm = ref.multi_batch_norm(X * 3, X, X * 2)
    assert perm["reference"] == 1
    for i, j in enumerate([2, 0, 1]):
        np.testing.assert_array_equal(perm["logcounts"][i], out["logcounts"][j])
        np.testing.assert_array_equal(perm["size_factors"][i], out["size_factors"][j])


def test_identical_batches_are_plainly_normalized():
    X3 = counts(1001) * 3
    out = ref.multi_batch_norm(X3, X3)
    lib = X3.sum(axis=0)
    want = np.log2(X3 / (lib / lib.mean()) + 1)
    for lc in out["logcounts"]:
        np.testing.assert_allclose(lc, want, rtol=1e-13, atol=1e-13)
    np.testing.assert_array_equal(out["ratios"], np.ones((2, 2)))


def test_library_size_fallback():
    A, B = counts(1002), counts(1003, cells=70) * 2
    want = ref.multi_batch_norm(A, B)
    got = ref.multi_batch_norm(A, B, size_factors=[A.sum(axis=0) * 7.0, B.sum(axis=0)])
    for a, b in zip(got["logcounts"], want["logcounts"]):
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12)
    # given size factors are used: doubling one cell's factor halves its normalized counts relative to the rest
    sf = A.sum(axis=0).copy()
    sf[0] *= 2
    other = ref.multi_batch_norm(A, B, size_factors=[sf, None], log=False)
    plain = ref.multi_batch_norm(A, B, log=False)
    assert not np.allclose(other["logcounts"][0][:, 0], plain["logcounts"][0][:, 0])


def test_min_mean_changes_the_ratio():
    rng = np.random.default_rng(1004)
    A = counts(1004)
    # the second batch is deeper for the high-abundance genes than for the low ones
    fold = np.where(A.mean(axis=1) > 30, 3.0, 1.5)
    B = rng.poisson(A * fold[:, None]).astype(np.float64)
    seen = []
    for mm in (1, 10, 100):
        out = ref.multi_batch_norm(A, B, min_mean=mm)
        ave = out["averages"]
        keep = ref.grand_mean(ave[:, 0], ave[:, 1]) >= mm
        assert 0 < keep.sum() < keep.size
        np.testing.assert_allclose(out["ratios"][0, 1], np.median(ave[keep, 1] / ave[keep, 0]), rtol=1e-14)
        seen.append(out["ratios"][0, 1])
    assert len(set(seen)) == 3, seen
    with pytest.raises(ValueError, match=ref.RATIO_ERROR):
        ref.multi_batch_norm(A, B, min_mean=1e9)


def test_subset_row_and_normalize_all():
    A, B = counts(1005), counts(1006, cells=60) * 2
    keep = np.arange(100, 0, -1)  # unsorted, as 100:1 in the reference's test
    sub = ref.multi_batch_norm(A, B, subset_row=keep)
    direct = ref.multi_batch_norm(A[keep - 1], B[keep - 1])
    full = ref.multi_batch_norm(A, B, subset_row=keep, normalize_all=True)
    for i in range(2):
        np.testing.assert_array_equal(sub["logcounts"][i], direct["logcounts"][i])
        np.testing.assert_array_equal(sub["size_factors"][i], full["size_factors"][i])
        assert full["logcounts"][i].shape[0] == 200
        np.testing.assert_array_equal(full["logcounts"][i][keep - 1], sub["logcounts"][i])
    np.testing.assert_array_equal(sub["averages"], full["averages"])
    assert not np.allclose(sub["size_factors"][0], ref.multi_batch_norm(A, B)["size_factors"][0])


@pytest.mark.parametrize("order", ["reversed", "shuffled"])
def test_single_object_against_the_list_form(order):
    parts = [counts(1007, cells=40), counts(1008, cells=70) * 2, counts(1009, cells=55) * 3]
    want = ref.multi_batch_norm(*parts)
    combined = np.concatenate(parts, axis=1)
    batch = np.repeat([1, 2, 3], [40, 70, 55])
    idx = np.arange(165)[::-1] if order == "reversed" else np.random.default_rng(5).permutation(165)
    got = ref.multi_batch_norm(combined[:, idx], batch=batch[idx])
    np.testing.assert_allclose(got["logcounts"], np.concatenate(want["logcounts"], axis=1)[:, idx], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got["size_factors"], np.concatenate(want["size_factors"])[idx], rtol=1e-12)
    split = ref.multi_batch_norm(combined[:, idx], batch=batch[idx], preserve_single=False)
    assert split["levels"] == [1, 2, 3]
    for lev in range(3):
        np.testing.assert_array_equal(split["logcounts"][lev], got["logcounts"][:, batch[idx] == lev + 1])


def test_list_inputs_are_flattened():
    A, B = counts(1010), counts(1011) * 2
    a, b = ref.multi_batch_norm([A, B]), ref.multi_batch_norm(A, B)
    for x, y in zip(a["logcounts"], b["logcounts"]):
        np.testing.assert_array_equal(x, y)


def test_zero_and_infinite_ratios_take_part_in_the_ordering():
    ave_f = np.array([0.0, 2.0, 4.0, 8.0, 16.0])
    ave_s = np.array([3.0, 2.0, 0.0, 8.0, 32.0])
    ratios, smallest, rescaling = ref.rescale_size_factors([ave_f, ave_s], 0.5)
    assert ratios[0, 1] == 1.0 and ratios[1, 0] == 1.0   # s/f: 0, 1, 1, 2, inf; f/s: 0, 0.5, 1, 1, inf
    with pytest.raises(ValueError, match=ref.RATIO_ERROR):   # 0 / 0 among the kept genes
        ref.rescale_size_factors([np.array([0.0, 1.0]), np.array([0.0, 1.0])], 0.0)
    with pytest.raises(ValueError, match=ref.SF_ERROR):
        ref.multi_batch_norm(np.array([[1.0, 0.0], [2.0, 0.0]]), np.ones((2, 2)))


# ---------------------------------------------------------------- the product function's argument errors (no device)

def test_argument_errors():
    import batchelor_amd as bx
    f = bx.multiBatchNorm
    B1, B2 = counts(1, 100, 50), counts(2, 100, 80)
    with pytest.raises(ValueError, match="at least one matrix of counts must be supplied"):
        f()
    with pytest.raises(ValueError, match="'batch' must be specified if '...' has only one object"):
        f(B1)
    with pytest.raises(ValueError, match="number of rows is not the same across batches"):
        f(B1[:10], B2)
    with pytest.raises(ValueError, match="names of batches should be unique"):
        f(B1, B2, names=["a", "a"])
    with pytest.raises(ValueError, match="subset indices out of range"):
        f(B1, B2, subset_row=[0, 1])
    with pytest.raises(ValueError, match="selects no genes"):
        f(B1, B2, subset_row=[])
    with pytest.raises(ValueError, match="should be equal to number of cells"):
        f(B1, batch=np.ones(5))
    with pytest.raises(ValueError, match="'downsample'"):
        f(B1, B2, norm_args={"downsample": True})
    with pytest.raises(ValueError, match="'size.factors'"):
        f(B1, B2, norm_args={"log": True, "size.factors": None})
    with pytest.raises(ValueError, match="pseudo_count"):
        f(B1, B2, norm_args={"pseudo_count": np.inf})
    with pytest.raises(ValueError, match="min_mean"):
        f(B1, B2, min_mean=np.nan)
    with pytest.raises(ValueError, match="one vector per batch"):
        f(B1, B2, size_factors=[np.ones(50)])
    with pytest.raises(ValueError, match="one value per cell"):
        f(B1, B2, size_factors=[np.ones(50), np.ones(3)])
    with pytest.raises(ValueError, match="one value per cell"):
        f(B1, batch=np.repeat([1, 2], 25), size_factors=np.ones(3))
    for bad in (0.0, -1.0, np.nan, np.inf):
        sf = np.ones(50)
        sf[7] = bad
        with pytest.raises(ValueError, match="size factors should be positive"):
            f(B1, B2, size_factors=[sf, None])
    with pytest.raises(ValueError, match="at least one cell"):
        f(B1, B2[:, :0])

    class Sparse:
        def tocsr(self):
            return self

    class Sce:
        assays = {}

    with pytest.raises(TypeError, match="sparse"):
        f(Sparse(), B2)
    with pytest.raises(TypeError, match="SingleCellExperiment"):
        f(Sce(), B2)


def test_abi_entry_points_check_their_arguments():
    """The bmx_norm_* calls refuse null handles and bad arguments with a status and a message, without a device."""
    from batchelor_amd import _lib
    L = _lib.lib()
    i32, i64, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_double

    def err(rc):
        assert rc != 0
        return L.bmx_last_error().decode()

    rows = np.array([1, 5, 0], dtype=np.int32)
    assert L.bmx_norm_check_create(i32(5), None, i64(-1)) == 0
    assert L.bmx_norm_check_create(i32(5), _lib.i32p(rows), i64(2)) == 0
    assert "gene" in err(L.bmx_norm_check_create(i32(0), None, i64(-1)))
    assert "out of range" in err(L.bmx_norm_check_create(i32(5), _lib.i32p(rows), i64(3)))
    assert "out of range" in err(L.bmx_norm_check_create(i32(4), _lib.i32p(rows), i64(2)))
    assert "no genes" in err(L.bmx_norm_check_create(i32(5), _lib.i32p(rows), i64(0)))
    sf = np.array([1.0, 2.0, 0.0, np.nan, np.inf, -1.0])
    assert L.bmx_norm_check_batch(i64(2), _lib.f64p(sf)) == 0
    assert L.bmx_norm_check_batch(i64(2), None) == 0
    assert "at least one cell" in err(L.bmx_norm_check_batch(i64(0), None))
    for n in (3, 4, 5, 6):
        probe = np.ascontiguousarray(np.concatenate([sf[:2], sf[n - 1:n]]))
        assert "size factors should be positive" in err(L.bmx_norm_check_batch(i64(3), _lib.f64p(probe)))
    assert L.bmx_norm_check_run(f64(1), i32(1), f64(1)) == 0
    assert L.bmx_norm_check_run(f64(-np.inf), i32(0), f64(0)) == 0
    assert "min_mean" in err(L.bmx_norm_check_run(f64(np.nan), i32(1), f64(1)))
    assert "pseudo_count" in err(L.bmx_norm_check_run(f64(1), i32(1), f64(np.inf)))
    assert "'log'" in err(L.bmx_norm_check_run(f64(1), i32(2), f64(1)))

    h = ctypes.c_void_p()
    assert "gene" in err(L.bmx_norm_create(i32(0), i32(0), None, i64(-1), ctypes.byref(h)))
    assert "out of range" in err(L.bmx_norm_create(i32(0), i32(4), _lib.i32p(rows), i64(2), ctypes.byref(h)))
    assert not h
    for call in (lambda: L.bmx_norm_begin_batch(None, i64(1), None),
                 lambda: L.bmx_norm_add_block(None, None, i64(1)),
                 lambda: L.bmx_norm_run(None, f64(1), i32(1), f64(1), None, None, None, None, None),
                 lambda: L.bmx_norm_stage_ms(None, None)):
        assert call() != 0
        assert L.bmx_last_error()
