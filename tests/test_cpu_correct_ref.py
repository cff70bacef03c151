"""The inputs of tests/test_gpu_correct_forms.py are conditioned well enough for its tolerances: on every one of its cases
(tests/correct_forms_cases.py) the FP64 oracle agrees with the long-double restatement of tests/correct_ref.py within the
tolerance the device is held to, with room to spare -- so a device that misses the tolerance is wrong, not unlucky -- and
every case selects the kernel it is there for.  Oracle and numpy only: no device, no extension."""
import math

import numpy as np
import pytest

from oracle import fastmnn_oracle as orc
from tests import correct_forms_cases as cf
from tests import correct_ref as ref

# the share of a tolerance the oracle may use up against long double (it stays below 0.005 on the cases measured so far)
SHARE = 0.05


def _assert_within(actual, desired, share=SHARE, rtol=0.0, atol=0.0, equal_nan=False):
    np.testing.assert_allclose(actual, np.asarray(desired, dtype=np.float64), rtol=share * rtol, atol=share * atol,
                               equal_nan=equal_nan)


def test_long_double_is_wider_than_double():
    assert ref.has_extended_precision()


def test_case_tables_straddle_the_kernels_blocks():
    # the segment lengths and restrict lists were chosen around 512-row workgroups and 512-position reduction blocks
    assert cf.PASS_ROWS == 512 and cf.RED_ROWS == 512
    assert {cf.PASS_ROWS - 1, cf.PASS_ROWS, cf.PASS_ROWS + 1} <= set(cf.CENTRE_N) & set(cf.VARIANCE_N)
    assert max(cf.CENTRE_N) > 2 * cf.PASS_ROWS and max(cf.VARIANCE_N) > 2 * cf.PASS_ROWS


def test_every_form_is_selected():
    rows = {cf.rows_form(d) for d in cf.CENTRE_D}
    assert rows == {"rows_pass", "rows_pass_v2<32>", "rows_pass_v2<64>"}
    assert {cf.rows_form(d) for d in cf.VARIANCE_D} == rows
    assert [cf.rows_form(d) for d in cf.RESTRICT_D] == ["rows_pass_v2<32>", "rows_pass_v2<64>", "rows_pass"]
    assert [cf.rows_form(c.d) for c in cf.ENGINE_CASES] == ["rows_pass_v2<64>", "rows_pass_v2<64>", "rows_pass",
                                                            "rows_pass_v2<32>"]
    assert cf.rows_form(cf.CENTRE_REFUSED_D) == "refused"
    # four columns a lane in rows_pass, both parities
    assert {255, 256} <= set(cf.CENTRE_D) and cf.rows_form(255) == cf.rows_form(256) == "rows_pass"
    tri = {cf.tricube_form(c.k, c.d, c.U) for c in cf.TRICUBE_CASES}
    assert {("tricube_apply_half", t) for t in (1, 2, 3, 4)} | {("tricube_apply_kernel", 0)} == tri
    assert cf.tricube_form(32, 64, 300)[0] != cf.tricube_form(33, 64, 300)[0]
    assert {cf.tricube_form(c.k, c.d, c.U)[0] for c in cf.TRICUBE_CASES if c.clamp} == {"tricube_apply_half",
                                                                                         "tricube_apply_kernel"}
    avg = [cf.average_form(c.d, c.k) for c in cf.AVERAGE_CASES]
    assert avg[:2] == ["average_correction_half", "average_correction_kernel"]
    assert set(avg) == {"average_correction_half", "average_correction_kernel"}


# ---- centring ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cf.CENTRE_CASES, ids=cf.centre_id)
def test_centring_oracle_meets_the_tolerance(case):
    test, batch = cf.centre_inputs(*case)
    _assert_within(orc.center_along_batch_vector(test, batch), ref.center_along_batch_vector(test, batch), **cf.CENTRE_TOL)


@pytest.mark.parametrize("d,kind", cf.RESTRICT_CASES)
def test_restricted_centring_oracle_meets_the_tolerance(d, kind):
    test, batch = cf.centre_inputs(d, cf.RESTRICT_N, 0.0)
    restrict = cf.restrict_list(d, kind)
    assert restrict.min() >= 1 and restrict.max() <= cf.RESTRICT_N
    distinct = np.unique(restrict).size
    if kind == "twice":      # some rows twice, some not at all, more positions than two blocks
        assert distinct < restrict.size and distinct < cf.RESTRICT_N and restrict.size > 2 * cf.RED_ROWS
    else:                    # a true subset, not in row order
        assert distinct == restrict.size < cf.RESTRICT_N and np.any(np.diff(restrict) < 0)
        assert abs(restrict.size - cf.RED_ROWS) <= 1
    want = ref.center_along_batch_vector(test, batch, restrict)
    _assert_within(orc.center_along_batch_vector(test, batch, restrict), want, **cf.CENTRE_TOL)
    # the restriction matters: the unrestricted result is far outside the tolerance
    plain = orc.center_along_batch_vector(test, batch)
    assert np.abs(plain - np.asarray(want, dtype=np.float64)).max() > 1e-6


def test_zero_batch_vector_is_nan_on_both_sides():
    for d in cf.RESTRICT_D:
        test, _ = cf.centre_inputs(d, 7, 0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            got = orc.center_along_batch_vector(test, np.zeros(d))
        assert np.isnan(got).all() and np.isnan(ref.center_along_batch_vector(test, np.zeros(d))).all()


# ---- total variance ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n", cf.VARIANCE_CASES)
def test_variance_numpy_meets_the_tolerance_and_needs_the_pivot(d, n):
    x = cf.variance_input(d, n)
    want = float(ref.total_variance(x))
    assert abs(np.var(x, axis=0, ddof=1).sum() / want - 1) < SHARE * cf.VARIANCE_RTOL
    # the device's one-pass form with its first-row pivot has the accuracy; without the shift it misses the tolerance on
    # every case (by 1e3 .. 1e6 times on most: the rounding of x^2 = 1e10 is random and partly cancels over the columns)
    assert abs(ref.one_pass_variance(x, pivot=x[0]) / want - 1) < SHARE * cf.VARIANCE_RTOL
    assert abs(ref.one_pass_variance(x) / want - 1) > 10 * cf.VARIANCE_RTOL


def test_variance_of_one_row_is_nan():
    assert np.isnan(ref.total_variance(cf.variance_input(64, 2)[:1]))


# ---- tricube ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cf.TRICUBE_CASES, ids=lambda c: c.id)
def test_tricube_oracle_meets_the_tolerance(case):
    test, correction, involved = cf.tricube_inputs(case)
    assert test.shape == (case.n, case.d) and correction.shape == (case.U, case.d) and involved.size == case.U
    assert np.unique(involved).size == case.U
    idx, dist = cf.tricube_neighbours(case)
    k = min(case.k, case.U)
    assert idx.shape == (case.n, k) and np.all(np.diff(dist, axis=1) >= 0)
    want = ref.tricube_weighted_correction(test, correction, idx, dist, ndist=case.ndist)
    got = test + orc.compute_tricube_average(correction, idx, dist, ndist=case.ndist)
    _assert_within(got, want, **cf.TRICUBE_TOL)
    # ... and the oracle's own kNN inside gives the very same thing
    assert np.array_equal(got, orc.tricube_weighted_correction(test, correction, involved, k=case.k, ndist=case.ndist),
                          equal_nan=True)
    nan_rows = np.isnan(got).any(axis=1)
    if case.k == 1 and case.ndist == 1:
        # rel = 1 for the only neighbour: 0 / 0, but for the MNN-involved cells themselves (distance 0, the floor)
        assert np.array_equal(np.flatnonzero(~nan_rows) + 1, involved) and np.isnan(got[nan_rows]).all()
    else:
        assert not nan_rows.any()
    middle = dist[:, math.ceil(k / 2) - 1]
    if case.clamp:
        floored = middle * case.ndist < 1e-8
        copies = math.ceil(case.k / 2)
        assert floored.sum() == cf.CLAMP_GROUPS * (1 + copies + cf.CLAMP_NEAR)
        rel = dist[floored] / 1e-8
        # the cell and its copies: the middle distance is exactly 0; the near-copies: 3 j 1e-9, still under the floor
        assert ((rel == 0).sum(axis=1) >= copies).sum() == cf.CLAMP_GROUPS * (1 + copies)
        assert np.all(((rel > 0.05) & (rel < 0.5)).sum(axis=1) >= cf.CLAMP_NEAR - 1)   # weights strictly inside (0, 1)
        assert np.all((rel > 1).sum(axis=1) >= 1)                              # weights exactly 0
    elif case.ndist != 1 and case.n > case.U:
        assert np.all(middle[np.setdiff1d(np.arange(case.n), involved - 1)] * case.ndist > 1e-8)


def test_tricube_without_neighbours_is_the_input():
    case = cf.TRICUBE_K0
    test, correction, involved = cf.tricube_inputs(case)
    # (the oracle follows R to the letter there -- zeros shaped like the CORRECTION, R/utils_tricube.R:22-23, which do not
    # add to the cells -- so only the reference speaks: no neighbours, no correction)
    assert involved.size == case.U and correction.shape[0] != test.shape[0]
    empty = np.zeros((case.n, 0))
    assert np.array_equal(np.asarray(ref.tricube_weighted_correction(test, correction, empty, empty), dtype=np.float64), test)


# ---- pair averaging ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cf.AVERAGE_CASES, ids=lambda c: c.id)
def test_averaging_oracle_meets_the_tolerance(case):
    left, right = cf.average_inputs(case)
    first, second = cf.average_pairs(case)
    assert first.size > 0
    partners = np.bincount(second)
    if case.cluster:
        # the k right cells nearest the cluster are paired with every left cell: k1 = n1 = k partners, the most there can be
        assert case.n1 == case.k
        # (the cluster's own spread moves the last places of that list for a few left cells: most, not all, are complete)
        assert partners.max() == case.k and (partners == case.k).sum() >= case.k - 4
    else:
        assert np.unique(second).size > 8 and partners.max() > 1
    want, want_second = ref.average_correction(left, first, right, second)
    got, got_second = orc.average_correction(left, first, right, second)
    assert np.array_equal(got_second, want_second)
    _assert_within(got, want, **cf.AVERAGE_TOL)


# ---- fused passes through the engine ----------------------------------------------------------------------------------
def _same_pairs(a, b):
    assert len(a) == len(b)
    for (al, ar), (bl, br) in zip(a, b):
        assert np.array_equal(al, bl) and np.array_equal(ar, br)


@pytest.mark.parametrize("case", cf.ENGINE_CASES, ids=lambda c: c.id)
def test_engine_cases_are_no_near_ties(case):
    """The oracle's pairs do not move when every coordinate moves by a few units in its last place, and neither merge is
    skipped: a pair mismatch of the device on these inputs is a finding."""
    info = cf.engine_reference(case).merge_info
    assert len(info.pairs) == 2 and all(p[0].size > 0 for p in info.pairs) and not np.any(info.skipped)
    assert [len(x) for x in info.left] == [1, 2]     # the second merge has two segments on its left
    got = orc.reduced_mnn(*cf.nudge(cf.engine_batches(case)))
    _same_pairs(got.merge_info.pairs, info.pairs)
    assert cf.engine_reference(case).corrected.shape == (sum(cf.ENGINE_SIZES), case.d)
