"""regressBatches(d=, deferred=True) on the device: the PCA of residuals that are never formed, against the longdouble
operator of tests/residual_pca_ref.py built from the device's OWN coefficients (so only the PCA is under test), and
against today's route (residuals through the host, then multiBatchPCA).

The allowances are derived in the docstring of tests/residual_pca_ref.py; tests/test_cpu_residual_pca.py shows that a
float64 restatement meets them on these inputs and that a planted fault misses them a hundredfold.  Every test prints the
ratio it asserts on."""
import numpy as np
import pytest

import batchelor_amd as bx
from batchelor_amd import linear_correct as lc
from tests import pca_ref
from tests import residual_pca_ref as ref

pytestmark = pytest.mark.gpu

D = ref.D_WANTED
_today, _refs = {}, {}


def call(name, **kw):
    k = ref.case(name)
    return bx.regressBatches(*k["batches"], design=k["design"], keep=k["keep"], restrict=k["restrict"],
                             subset_row=k["subset_row"], correct_all=k["subset_row"] is not None, d=D, **kw)


def today(name):
    """regressBatches(..., d=5) without `deferred`, once per case."""
    if name not in _today:
        _today[name] = call(name)
    return _today[name]


def reference(name, coefficients):
    """(exact, allowances) from the device's coefficients, once per case (they are the same bits in every call)."""
    if name not in _refs:
        _refs[name] = (coefficients.copy(), *ref.reference(name, coefficients))
    coef, ex, al = _refs[name]
    assert np.array_equal(coef, coefficients)
    return ex, al


def as_fit(name, got):
    sizes = np.cumsum([x.shape[1] for x in ref.case(name)["batches"]])[:-1]
    return dict(got.pca, pcs=np.split(got.pcs, sizes, axis=0))


@pytest.mark.parametrize("iters", [1, 2])
@pytest.mark.parametrize("name", list(ref.CASES))
def test_fixed_count_fit_is_the_operator_of_the_residuals(name, iters):
    got = call(name, deferred=True, residuals=False, pca_iters=iters)
    assert got.corrected is None and got.pca["path"] == "device-deferred" and got.pca["iters_used"] == iters
    assert got.pcs.shape == (sum(x.shape[1] for x in ref.case(name)["batches"]), D)
    ex, al = reference(name, got.coefficients)
    fit = as_fit(name, got)
    r = pca_ref.fit_ratios(ex, al, fit)
    r["projection"] = pca_ref.projection_ratio(ex, al, fit)
    print(f"{name}, {iters} step(s): error / allowance: " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r


@pytest.mark.parametrize("name", ref.CONVERGED)
def test_converged_fit_and_todays_route_agree(name):
    got = call(name, deferred=True, pca_tol=ref.TOL)
    ex, al = reference(name, got.coefficients)
    fit = as_fit(name, got)
    r = pca_ref.fit_ratios(ex, al, fit)
    r["projection"] = pca_ref.projection_ratio(ex, al, fit)
    res = pca_ref.residual_ratios(ex, al, fit, ref.TOL)
    want = today(name).pcs
    diff = float(np.abs(np.abs(got.pcs) - np.abs(want)).max() / np.abs(want).max())
    print(f"{name}: converged in {got.pca['iters_used']} applications: " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()) +
          f"; residual reported {res['reported']:.3g}, recomputed {res['true']:.3g} (allowance {res['allow']:.3g}): over tol "
          f"{res['over_tol']:.3g}, own figure off {res['reported_off']:.3g}; pcs against today's route, up to sign: {diff:.3g}")
    assert all(v <= 1.0 for v in r.values()), r
    assert res["reported"] <= ref.TOL
    assert res["over_tol"] <= 1.0 and res["reported_off"] <= 1.0, res
    assert got.pcs.shape == want.shape and diff < 1e-6


@pytest.mark.parametrize("name", list(ref.CASES))
def test_coefficients_and_residuals_are_bitwise_todays(name):
    got, want = call(name, deferred=True, pca_iters=1), today(name)
    same = {"coefficients": np.array_equal(got.coefficients, want.coefficients),
            "corrected": np.array_equal(got.corrected, want.corrected), "batch": np.array_equal(got.batch, want.batch)}
    print(f"{name}: deferred against today's call, bitwise equal: {same}")
    assert all(same.values()) and got.corrected.shape == want.corrected.shape
    assert got.corrected.flags.f_contiguous and want.pca is None


@pytest.mark.parametrize("name", ["r130-three-none-restrict", "r65-small-fc", "r65-three-p64-restrict", "r64-split-fc",
                                  "sub70-small-p16-restrict"])
def test_without_residuals_repeats_and_blocked_uploads_are_bitwise_equal(name, monkeypatch):
    G = ref.CASES[name].G
    full = call(name, deferred=True, pca_iters=2)
    bare = call(name, deferred=True, residuals=False, pca_iters=2)
    again = call(name, deferred=True, residuals=False, pca_iters=2)
    monkeypatch.setattr(lc, "BLOCK_BYTES", 8 * G * 50)   # blocks of 50 cells
    blocked = call(name, deferred=True, residuals=False, pca_iters=2)
    same = {}
    for what, other in (("residuals=True", full), ("second run", again), ("blocked upload", blocked)):
        same[what] = all(np.array_equal(getattr(bare, f), getattr(other, f)) for f in ("pcs", "coefficients")) and all(
            np.array_equal(bare.pca[k], other.pca[k]) for k in ("rotation", "centers", "d"))
    print(f"{name}: pcs, coefficients, rotation, centers, d of residuals=False bitwise equal to: {same}")
    assert bare.corrected is None and again.corrected is None and full.corrected is not None
    assert all(same.values())


def test_batch_correct_passes_the_arguments_through():
    name = "r130-three-none-restrict"
    k = ref.case(name)
    direct = call(name, deferred=True, residuals=False)
    via = bx.batchCorrect(*k["batches"], restrict=k["restrict"], PARAM=bx.RegressParam(d=D, deferred=True, residuals=False))
    same = np.array_equal(via.pcs, direct.pcs)
    print(f"batchCorrect(PARAM=RegressParam(d={D}, deferred=True, residuals=False)): pcs bitwise equal to the direct call: {same}")
    assert via.corrected is None and via.pca["path"] == "device-deferred" and same


def test_one_object_forms():
    """One object divided by `batch` (interleaved labels) has the batches of the several-object call resident; one object
    with a design and no `batch` is one batch."""
    name = "r130-three-p16"
    k = ref.case(name)
    sizes = [x.shape[1] for x in k["batches"]]
    whole = np.concatenate(k["batches"], axis=1)
    labels = np.repeat(np.arange(1, len(sizes) + 1), sizes)
    perm = np.random.default_rng(5).permutation(whole.shape[1])
    several = bx.regressBatches(*k["batches"], d=D, deferred=True, residuals=False)
    divided = bx.regressBatches(whole[:, perm], batch=labels[perm], d=D, deferred=True)
    # (the divided parts hold a batch's cells in another order: the sums over cells agree to rounding, not to the bit, so
    # the bound is the one of the converged comparison above)
    diff = float(np.abs(np.abs(divided.pcs) - np.abs(several.pcs[perm])).max() / np.abs(several.pcs).max())
    print(f"one object divided by batch against several objects, converged, up to sign: pcs max rel {diff:.3g}")
    assert diff < 1e-6 and np.array_equal(divided.batch, labels[perm]) and divided.corrected.shape == whole.shape

    got = bx.regressBatches(whole, design=k["design"], d=D, deferred=True, residuals=False, pca_iters=1)
    ex = ref.exact([whole], got.coefficients, [k["design"]], np.arange(k["design"].shape[1]))
    al = ref.allowances(ex)
    fit = dict(got.pca, pcs=[got.pcs])
    r = pca_ref.fit_ratios(ex, al, fit)
    r["projection"] = pca_ref.projection_ratio(ex, al, fit)
    print("one object with a design and no batch (one batch), 1 step: error / allowance: " +
          ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r
    with pytest.raises(ValueError, match="both 'design'"):
        bx.regressBatches(whole, batch=labels, design=k["design"], d=D, deferred=True)


def test_a_shape_the_device_pca_refuses_takes_todays_route():
    rng = np.random.default_rng(60)
    B = [rng.standard_normal((60, 40)) + 1.0, rng.standard_normal((60, 50))]
    want = bx.regressBatches(*B, d=D)
    got = bx.regressBatches(*B, d=D, deferred=True, residuals=False)
    kept = bx.regressBatches(*B, d=D, deferred=True)
    print(f"60 genes: path {got.pca['path']!r}; pcs bitwise today's: {np.array_equal(got.pcs, want.pcs)}")
    assert got.pca["path"].startswith("residuals through the host") and got.pca["path"] != "device-deferred"
    assert got.corrected is None and got.pcs.shape == (90, D) and np.array_equal(got.pcs, want.pcs)
    assert np.array_equal(kept.corrected, want.corrected) and np.array_equal(kept.pcs, want.pcs)
    assert got.pca["rotation"].shape == (60, D)
