"""rescaleBatches() / regressBatches() without a GPU: the numpy restatement (tests/linear_correct_ref.py) against the
identities the reference's own tests state (tests/testthat/test-rescale-batch.R, test-regress-batch.R), and the argument
errors of the product functions, which are raised before any device work."""
import ctypes

import numpy as np
import pytest

from tests import linear_correct_ref as ref


def counts(seed, ncol=(50, 100), genes=200):
    """test-rescale-batch.R:6-8: Poisson counts around gamma-distributed means, the second batch scaled gene by gene."""
    rng = np.random.default_rng(seed)
    means = 2.0 ** rng.gamma(2.0, 1.0, genes)
    out = [rng.poisson(means[:, None], (genes, ncol[0])).astype(np.float64)]
    for n in ncol[1:]:
        out.append(rng.poisson((means * rng.uniform(0, 2, genes))[:, None], (genes, n)).astype(np.float64))
    return out


def test_rescale_matches_the_closed_form():
    # test-rescale-batch.R:5-26
    A = counts(130000)
    ave = [a.mean(axis=1) for a in A]
    r = np.minimum(*ave)
    B = [np.log2(a + 1) for a in A]
    out, labels = ref.rescale(B)
    assert labels.tolist() == [1] * 50 + [2] * 100
    with np.errstate(divide="ignore", invalid="ignore"):
        s = [np.where(np.isfinite(r / a), r / a, 0.0) for a in ave]
    err = max(np.abs(out[:, :50] - np.log2(A[0] * s[0][:, None] + 1)).max(),
              np.abs(out[:, 50:] - np.log2(A[1] * s[1][:, None] + 1)).max())
    print("rescale against log2(A * ref/ave + 1): max abs", err)
    assert err < 1e-12


def test_rescale_rows_of_zeros_stay_zero():
    # test-rescale-batch.R:28-32
    B = [np.log2(a + 1) for a in counts(130000)]
    B[0][:10] = 0
    B[1][4:15] = 0
    out, _ = ref.rescale(B)
    assert np.array_equal(out[:15], np.zeros((15, 150)))


def test_rescale_log_base_and_pseudo_count():
    # test-rescale-batch.R:58-71
    A = counts(1300001)
    ave = [a.mean(axis=1) for a in A]
    r = np.minimum(*ave)
    B = [np.log2(a + 1) for a in A]
    base2, _ = ref.rescale(B)
    base10, _ = ref.rescale([b / np.log2(10) for b in B], log_base=10)
    np.testing.assert_allclose(base2 / np.log2(10), base10, rtol=1e-10, atol=1e-12)
    C = [np.log10(a + 3.2) for a in A]
    out, _ = ref.rescale(C, pseudo_count=3.2, log_base=10)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = [np.where(np.isfinite(r / a), r / a, 0.0) for a in ave]
    np.testing.assert_allclose(out[:, :50], np.log10(A[0] * s[0][:, None] + 3.2), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(out[:, 50:], np.log10(A[1] * s[1][:, None] + 3.2), rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("fn", ["rescale", "regress"])
def test_subset_row_and_correct_all(fn):
    # test-rescale-batch.R:48-56, test-regress-batch.R:36-43
    B = [np.log2(a + 1) for a in counts(1300002)]
    f = getattr(ref, fn)
    keep = np.random.default_rng(3).permutation(200)[:100] + 1
    np.testing.assert_array_equal(f(B, subset_row=keep)[0], f([b[keep - 1] for b in B])[0])
    np.testing.assert_array_equal(f(B, subset_row=keep, correct_all=True)[0], f(B)[0])


@pytest.mark.parametrize("fn", ["rescale", "regress"])
def test_within_object_batches(fn):
    # test-rescale-batch.R:150-171, test-regress-batch.R:131-152
    rng = np.random.default_rng(130002)
    B = [np.log2(rng.poisson(5, (100, n)) + 1.0) for n in (100, 200, 150)]
    f = getattr(ref, fn)
    combined = np.concatenate(B, axis=1)
    batches = np.repeat([1, 2, 3], [100, 200, 150])
    shuffle = rng.permutation(450)
    want = f(B)
    got = f([combined[:, shuffle]], batch=batches[shuffle])
    np.testing.assert_allclose(got[0], want[0][:, shuffle], rtol=1e-12, atol=1e-13)
    assert np.array_equal(got[1], want[1][shuffle])


@pytest.mark.parametrize("fn", ["rescale", "regress"])
def test_restricted_duplicates_get_the_values_of_their_originals(fn):
    # test-rescale-batch.R:178-193, test-regress-batch.R:160-175
    rng = np.random.default_rng(1300021)
    B = [np.log2(rng.poisson(5, (100, n)) + 1.0) for n in (100, 200)]
    f = getattr(ref, fn)
    want = f(B)[0]
    C = [np.concatenate([B[0], B[0][:, :10]], axis=1), np.concatenate([B[1], B[1][:, :20]], axis=1)]
    got = f(C, restrict=[np.arange(1, 101), np.arange(1, 201)])[0]
    np.testing.assert_allclose(got[:, :100], want[:, :100], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(got[:, 110:310], want[:, 100:], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(got[:, 100:110], want[:, :10], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(got[:, 310:], want[:, 100:120], rtol=1e-12, atol=1e-13)


def test_regress_default_is_centring_per_batch():
    # test-regress-batch.R:27-33
    B = [np.log2(a + 1) for a in counts(130000)]
    out, labels, coef = ref.regress(B)
    err = max(np.abs(out[:, :50] - (B[0] - B[0].mean(axis=1, keepdims=True))).max(),
              np.abs(out[:, 50:] - (B[1] - B[1].mean(axis=1, keepdims=True))).max())
    print("regress against B - rowMeans(B): max abs", err)
    assert err < 1e-12
    np.testing.assert_allclose(coef, np.stack([b.mean(axis=1) for b in B], axis=1), rtol=1e-12)


def test_regress_designs():
    # test-regress-batch.R:46-73
    B = [np.log2(a + 1) for a in counts(130000)]
    want = ref.regress(B)[0]
    b = np.repeat([1.0, 2.0], [50, 100])
    factor = np.stack([np.ones(150), (b == 2).astype(float)], axis=1)         # model.matrix(~factor(b))
    np.testing.assert_allclose(ref.regress(B, design=factor)[0], want, rtol=1e-10, atol=1e-12)
    cont = np.stack([np.ones(150), b], axis=1)                                # model.matrix(~b)
    combined = np.concatenate(B, axis=1)
    got = ref.regress(B, design=cont)[0]
    beta = np.linalg.solve(cont.T @ cont, cont.T @ combined.T)                # lm.fit's residuals by the normal equations
    np.testing.assert_allclose(got, combined - (cont @ beta).T, rtol=1e-9, atol=1e-10)
    single = ref.regress([combined], design=cont)
    np.testing.assert_allclose(single[0], got, rtol=1e-12, atol=1e-13)
    assert np.all(single[1] == 1)
    with pytest.raises(ValueError, match="total number"):
        ref.regress(B, design=np.ones((1, 1)))
    # keep: the intercept stays in
    kept = ref.regress(B, design=cont, keep=[1])[0]
    coef = ref.regress(B, design=cont)[2]
    np.testing.assert_allclose(kept, combined - np.outer(coef[:, 1], b), rtol=1e-12, atol=1e-12)


def test_lstsq_and_qr_agree():
    B = [np.log2(a + 1) for a in counts(130000)]
    rng = np.random.default_rng(5)
    cov = rng.normal(size=150)
    design = np.stack([np.ones(150), np.repeat([0.0, 1.0], [50, 100]), (cov - cov.mean()) / cov.std()], axis=1)
    a = ref.regress(B, design=design, solver="lstsq")[0]
    b = ref.regress(B, design=design, solver="qr")[0]
    spread = np.abs(a - b).max()
    print("lstsq against explicit QR: max abs", spread)
    assert spread < 1e-11


# ---------------------------------------------------------------- the product functions' argument errors (no device)

def _mats(seed=130003):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(100, 100)), rng.normal(size=(100, 200))


@pytest.mark.parametrize("fn", ["rescaleBatches", "regressBatches"])
def test_argument_errors(fn):
    import batchelor_amd as bx
    f = getattr(bx, fn)
    B1, B2 = _mats()
    with pytest.raises(ValueError, match="at least two batches must be specified"):
        f()
    with pytest.raises(ValueError, match="'batch' must be specified if '...' has only one object"):
        f(B1)
    with pytest.raises(ValueError, match="number of rows is not the same across batches"):
        f(B1[:10], B2)
    with pytest.raises(ValueError, match="no cells remaining in a batch after restriction"):
        f(B1, B2, restrict=[np.zeros(0, dtype=int), np.zeros(0, dtype=int)])
    with pytest.raises(ValueError, match="no cells remaining in a batch after restriction"):
        f(np.concatenate([B1, B2], axis=1), batch=np.repeat([1, 2], [100, 200]),
          restrict=[np.arange(1, 101)])
    with pytest.raises(ValueError, match="names of batches should be unique"):
        f(B1, B2, names=["a", "a"])
    with pytest.raises(ValueError, match="'restrict' indices out of range"):
        f(B1, B2, restrict=[[1, 101], None])
    with pytest.raises(ValueError, match="subset indices out of range"):
        f(B1, B2, subset_row=[0, 1])
    with pytest.raises(ValueError, match="should be equal to number of cells"):
        f(B1, batch=np.ones(5))

    class Sparse:
        def tocsr(self):
            return self

    class Sce:
        assays = {}

    with pytest.raises(TypeError, match="sparse"):
        f(Sparse(), B2)
    with pytest.raises(TypeError, match="SingleCellExperiment"):
        f(Sce(), B2)


def test_rescale_argument_errors():
    import batchelor_amd as bx
    B1, B2 = _mats()
    with pytest.raises(ValueError, match="at least two batches must be specified"):
        bx.rescaleBatches(B1, batch=np.ones(100))
    with pytest.raises(ValueError, match="log_base"):
        bx.rescaleBatches(B1, B2, log_base=1)
    with pytest.raises(ValueError, match="log_base"):
        bx.rescaleBatches(B1, B2, log_base=-2)
    with pytest.raises(ValueError, match="pseudo_count"):
        bx.rescaleBatches(B1, B2, pseudo_count=np.nan)


def test_regress_argument_errors():
    import batchelor_amd as bx
    B1, B2 = _mats()
    with pytest.raises(ValueError, match=r"'nrow\(design\)' should be equal to the total number of cells"):
        bx.regressBatches(B1, B2, design=np.ones((1, 1)))
    design = np.stack([np.ones(300), np.repeat([0.0, 1.0], [100, 200])], axis=1)
    with pytest.raises(ValueError, match="'keep' indices out of range"):
        bx.regressBatches(B1, B2, design=design, keep=[3])
    with pytest.raises(ValueError, match="'keep' indices out of range"):
        bx.regressBatches(B1, B2, keep=[0])
    with pytest.raises(ValueError, match="between 1 and 64 columns"):
        bx.regressBatches(B1, B2, design=np.random.default_rng(0).normal(size=(300, 65)))
    with pytest.raises(ValueError, match="not of full column rank"):
        bx.regressBatches(B1, B2, design=np.stack([np.ones(300), np.ones(300)], axis=1))
    # full rank over all cells, deficient over the restricted ones (only batch 1's cells of an indicator pair)
    with pytest.raises(ValueError, match="not of full column rank"):
        bx.regressBatches(np.concatenate([B1, B2], axis=1), design=design, restrict=[np.arange(1, 101)])
    with pytest.raises(ValueError, match="'d' must be positive"):
        bx.regressBatches(B1, B2, d=0)


def test_design_weights_reproduce_least_squares():
    from batchelor_amd.linear_correct import design_weights
    rng = np.random.default_rng(7)
    design = np.stack([np.ones(300), rng.normal(size=300), rng.normal(size=300)], axis=1)
    x = rng.normal(size=(20, 300))
    rows = np.sort(rng.choice(300, 120, replace=False))
    w = design_weights(design, rows)
    want = np.linalg.lstsq(design[rows], x[:, rows].T, rcond=None)[0].T
    np.testing.assert_allclose(x[:, rows] @ w, want, rtol=1e-10, atol=1e-12)


def test_abi_entry_points_check_their_arguments():
    """The bmx_linear_* calls refuse null handles and bad arguments with a status and a message, without a device."""
    from batchelor_amd import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    assert L.bmx_linear_create(ctypes.c_int32(0), ctypes.c_int32(0), ctypes.byref(h)) != 0
    assert b"gene" in L.bmx_last_error()
    for call in (lambda: L.bmx_linear_begin_batch(None, ctypes.c_int64(1), None, ctypes.c_int64(-1)),
                 lambda: L.bmx_linear_add_block(None, None, ctypes.c_int64(1)),
                 lambda: L.bmx_linear_expect(None, ctypes.c_int32(0), ctypes.c_double(2), ctypes.c_double(1), ctypes.c_int32(0)),
                 lambda: L.bmx_linear_rescale(None, ctypes.c_double(2), ctypes.c_double(1), None, None, None),
                 lambda: L.bmx_linear_regress(None, None, ctypes.c_int32(0), None, None, ctypes.c_int32(0), None, None),
                 lambda: L.bmx_linear_fetch(None, None),
                 lambda: L.bmx_linear_stage_ms(None, None)):
        assert call() != 0
        assert L.bmx_last_error()
