"""Every hand-written form of the correction kernels of a merge step (batchelor_amd/csrc/correct.hip) at its first and last
shape: the centring and variance passes (rows_pass, rows_pass_v2<32|64>), the tricube-weighted correction
(tricube_apply_half over one to four trips of its piece loop, tricube_apply_kernel) and the pair averaging
(average_correction_half, average_correction_kernel), each against the long-double restatement of tests/correct_ref.py
rounded to double and against the FP64 oracle, at the tolerances tests/test_gpu_primitives.py holds the same primitives to.
The cases, and which kernel each selects, are in tests/correct_forms_cases.py; tests/test_cpu_correct_ref.py shows that the
oracle alone meets these tolerances on them with a twentieth of the room."""
import numpy as np
import pytest

from tests import correct_forms_cases as cf
from tests import correct_ref as ref
from tests.test_gpu_engine import assert_same_result

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    from batchelor_amd import natives
    return natives


@pytest.fixture(scope="module")
def bx():
    import batchelor_amd
    return batchelor_amd


def _f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- centring ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cf.CENTRE_CASES, ids=cf.centre_id)
def test_centring_every_width_and_segment_length(oracle, nat, case):
    d, n, offset = case
    test, batch = cf.centre_inputs(d, n, offset)
    centered = nat.center_along_batch_vector(test, batch)
    np.testing.assert_allclose(centered, _f64(ref.center_along_batch_vector(test, batch)), **cf.CENTRE_TOL)
    np.testing.assert_allclose(centered, oracle.center_along_batch_vector(test, batch), **cf.CENTRE_TOL)
    if n > 1:  # (the sample standard deviation of one projection is undefined)
        assert np.std(centered @ batch, ddof=1) < 1e-8 * (1 + offset)


@pytest.mark.parametrize("d,kind", cf.RESTRICT_CASES)
def test_centring_restrict_lists(oracle, nat, d, kind):
    test, batch = cf.centre_inputs(d, cf.RESTRICT_N, 0.0)
    restrict = cf.restrict_list(d, kind)
    centered = nat.center_along_batch_vector(test, batch, restrict=restrict)
    np.testing.assert_allclose(centered, _f64(ref.center_along_batch_vector(test, batch, restrict)), **cf.CENTRE_TOL)
    np.testing.assert_allclose(centered, oracle.center_along_batch_vector(test, batch, restrict), **cf.CENTRE_TOL)


@pytest.mark.parametrize("d", cf.RESTRICT_D)
def test_centring_along_a_zero_vector_is_nan(oracle, nat, d):
    test, _ = cf.centre_inputs(d, 7, 0.0)
    zero = np.zeros(d)
    centered = nat.center_along_batch_vector(test, zero)
    assert np.isnan(centered).all()
    with np.errstate(invalid="ignore", divide="ignore"):
        want = oracle.center_along_batch_vector(test, zero)
    np.testing.assert_allclose(centered, want, equal_nan=True, **cf.CENTRE_TOL)
    np.testing.assert_allclose(centered, _f64(ref.center_along_batch_vector(test, zero)), equal_nan=True, **cf.CENTRE_TOL)


def test_centring_refuses_more_than_256_dimensions(nat):
    rng = np.random.default_rng(1200106)
    d = cf.CENTRE_REFUSED_D
    with pytest.raises(RuntimeError, match="more than 256 dimensions are not supported"):
        nat.center_along_batch_vector(rng.standard_normal((7, d)), rng.standard_normal(d))


# ---- total variance ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n", cf.VARIANCE_CASES)
def test_total_variance_far_from_the_origin(nat, d, n):
    x = cf.variance_input(d, n)
    got = nat.total_variance(x)
    assert abs(got / float(ref.total_variance(x)) - 1) < cf.VARIANCE_RTOL
    assert abs(got / np.var(x, axis=0, ddof=1).sum() - 1) < cf.VARIANCE_RTOL


@pytest.mark.parametrize("d", cf.VARIANCE_D)
def test_total_variance_of_one_row_is_nan(nat, d):
    assert np.isnan(nat.total_variance(cf.variance_input(d, 2)[:1]))


# ---- tricube ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cf.TRICUBE_CASES, ids=lambda c: c.id)
def test_tricube_every_form(oracle, nat, case):
    test, correction, involved = cf.tricube_inputs(case)
    idx, dist = cf.tricube_neighbours(case)
    out = nat.tricube_weighted_correction(test, correction, involved, k=case.k, ndist=case.ndist)
    want = _f64(ref.tricube_weighted_correction(test, correction, idx, dist, ndist=case.ndist))
    np.testing.assert_allclose(out, want, **cf.TRICUBE_TOL)
    np.testing.assert_allclose(out, oracle.tricube_weighted_correction(test, correction, involved, k=case.k, ndist=case.ndist),
                               **cf.TRICUBE_TOL)
    if case.k == 1 and case.ndist == 1:  # 0 / 0 on both sides, everywhere but at the MNN-involved cells
        assert np.array_equal(np.flatnonzero(~np.isnan(out).any(axis=1)) + 1, involved)
    else:
        assert np.isfinite(out).all()


def test_tricube_without_neighbours_returns_the_input(nat):
    test, correction, involved = cf.tricube_inputs(cf.TRICUBE_K0)
    out = nat.tricube_weighted_correction(test, correction, involved, k=0)
    assert np.array_equal(out, test)


# ---- pair averaging ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cf.AVERAGE_CASES, ids=lambda c: c.id)
def test_pair_averaging_every_form(oracle, nat, case):
    left, right = cf.average_inputs(case)
    of, os_ = cf.average_pairs(case)
    f, s, avg, su = nat.mnn_average_correction(left, right, case.k)
    assert np.array_equal(f, of) and np.array_equal(s, os_)
    assert su.tolist() == sorted(set(s.tolist()))
    if case.cluster:  # a right cell with exactly k partners -- the most a list holds -- from the pairs the device returned
        partners = np.bincount(s)
        assert partners.max() == case.k and (partners == case.k).sum() >= case.k - 4
    want, want_second = ref.average_correction(left, of, right, os_)
    assert np.array_equal(su, want_second)
    np.testing.assert_allclose(avg, _f64(want), **cf.AVERAGE_TOL)
    oavg, osu = oracle.average_correction(left, of, right, os_)
    assert np.array_equal(su, osu)
    np.testing.assert_allclose(avg, oavg, **cf.AVERAGE_TOL)


# ---- fused passes through the engine ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cf.ENGINE_CASES, ids=lambda c: c.id)
def test_fused_passes_through_the_engine(bx, case):
    """APPLY + STATS in one pass over several segments, the old means as pivots, the centre handed to the search: pairs bit
    for bit, lost_var to 1e-7, and the per-column error at the bar of test_config1_two_batches."""
    out = bx.reducedMNN(*cf.engine_batches(case))
    err = assert_same_result(out, cf.engine_reference(case))
    print("engine %s: per-column error %.3g" % (case.id, err))
    assert err < cf.ENGINE_ERR
