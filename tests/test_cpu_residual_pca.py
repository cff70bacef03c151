"""regressBatches(d=, deferred=True) without a GPU: the float64 restatement of the deferred operator
(tests/residual_pca_ref.py) is held to every allowance on every input that tests/test_gpu_residual_pca.py uses, the same
checks reject the restatement with one planted fault by a factor of 100 at the least, and the new arguments and entry
points answer before any device work.

The allowances are derived in the docstring of tests/residual_pca_ref.py; nothing here is fitted to a result.  Every test
prints the ratios it asserts on."""
import ctypes
import os
import re

import numpy as np
import pytest

import batchelor_amd as bx
from batchelor_amd import _lib
from tests import pca_ref
from tests import residual_pca_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("bmx_residual_pca_create", "bmx_residual_pca_fit", "bmx_residual_pca_project", "bmx_linear_check_pca")


def f64_fit(name, iters, fault=None):
    batches, coefs, designs, drop, restrict = ref.operands(name, ref.coefficients_f64(name))
    return ref.deferred_f64(batches, coefs, designs, drop, ref.D_WANTED, iters, restrict=restrict, fault=fault)


def ratios(name, fit):
    ex, al = ref.reference(name, ref.coefficients_f64(name))
    r = pca_ref.fit_ratios(ex, al, fit)
    r["projection"] = pca_ref.projection_ratio(ex, al, fit)
    return ex, al, r


@pytest.mark.parametrize("iters", [1, 2])
@pytest.mark.parametrize("name", list(ref.CASES))
def test_float64_restatement_stays_inside_the_allowances(name, iters):
    """Completing at all is a condition on the inputs: every block has a positive definite Gram matrix, so the device is
    expected to take the case."""
    _, _, r = ratios(name, f64_fit(name, iters))
    print(f"{name}, {iters} step(s): float64 restatement error / allowance: " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r


@pytest.mark.parametrize("name", ref.CONVERGED)
def test_float64_restatement_converges_inside_the_allowances(name):
    fit = f64_fit(name, ref.F64_ITERS_CONVERGED)
    ex, al, r = ratios(name, fit)
    res = pca_ref.residual_ratios(ex, al, fit, ref.TOL)
    print(f"{name}: converged float64 restatement: " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()) +
          f"; residual {res['true']:.3g} (own figure {res['reported']:.3g}, allowance {res['allow']:.3g})")
    assert all(v <= 1.0 for v in r.values()), r
    assert res["over_tol"] <= 1.0 and res["reported_off"] <= 1.0, res


def _applies(fault, c):
    if fault in ("no_ET", "no_FS"):   # no fault without a design and without a restriction (residual_pca_ref.py, at FAULTS)
        return c.design is not None or c.restrict
    if fault == "mu_restricted":
        return c.restrict
    return True


@pytest.mark.parametrize("fault", ref.FAULTS)
def test_planted_fault_is_rejected_a_hundredfold(fault):
    seen = []
    for name, c in ref.CASES.items():
        if not _applies(fault, c):
            continue
        ex, al = ref.reference(name, ref.coefficients_f64(name))
        fit = f64_fit(name, 1, fault)
        ritz = pca_ref.worst(ex.ritz_defect(fit["rotation"], fit["d"]), al.ritz(fit["rotation"], fit["d"]))
        cen = pca_ref.worst(np.asarray(fit["centers"], dtype=ref.LD) - ex.centers(), al.centers())
        print(f"{fault} in {name}: Ritz defect / allowance {ritz:.3g}, centres / allowance {cen:.3g}")
        assert max(ritz, cen) >= 100.0, (fault, name, ritz, cen)
        seen.append(name)
    assert len(seen) >= 6


def test_the_low_rank_terms_cancel_without_design_and_restriction():
    """There E_b T and F S_b left out are no faults (residual_pca_ref.py, at FAULTS): the check must not cry wolf."""
    for name in ("r64-small-none", "r130-three-none", "r65-split-none"):
        for fault in ("no_ET", "no_FS"):
            ex, al = ref.reference(name, ref.coefficients_f64(name))
            fit = f64_fit(name, 1, fault)
            ratio = pca_ref.worst(ex.ritz_defect(fit["rotation"], fit["d"]), al.ritz(fit["rotation"], fit["d"]))
            print(f"{name}: {fault} in every batch: Ritz defect / allowance {ratio:.3g}")
            assert ratio <= 1.0


def test_case_table_covers_what_it_claims():
    cases = list(ref.CASES.values())
    assert {c.rows for c in cases} >= {64, 65, 130} and {c.sizes for c in cases} == {ref.SMALL, ref.THREE, ref.SPLIT}
    for design in (None, "factor+covariate"):
        assert {c.rows for c in cases if c.design == design} >= {64, 65}
    assert {c.restrict for c in cases if c.design is None} == {False, True}
    for pd in (15, 16, 64):
        assert {c.restrict for c in cases if c.design == pd} == {False, True}
    assert {c.rows for c in cases if c.design == 64} >= {64, 65, 130}
    assert any(c.G > c.rows for c in cases) and all(c.G == 130 and c.rows == 70 for c in cases if c.G > c.rows)
    for name in ref.CASES:
        k = ref.case(name)
        if k["subset_row"] is not None:
            assert not np.array_equal(k["subset_row"], np.sort(k["subset_row"]))


# ---------------------------------------------------------------------------------------------- arguments, ABI
def _two():
    rng = np.random.default_rng(3)
    return [rng.standard_normal((70, 40)), rng.standard_normal((70, 50))]


def test_new_keywords_are_checked_before_a_device_is_asked_for(monkeypatch):
    def no_gpu():
        raise AssertionError("require_gpu was reached")
    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    B = _two()
    with pytest.raises(ValueError, match="residuals=False"):
        bx.regressBatches(*B, d=5, residuals=False)
    with pytest.raises(ValueError, match="deferred=True"):
        bx.regressBatches(*B, deferred=True)
    with pytest.raises(ValueError, match="deferred=True"):
        bx.regressBatches(*B, deferred=True, residuals=False)
    one = np.concatenate(B, axis=1)
    design = np.column_stack([np.ones(90), np.arange(90.0)])
    batch = np.repeat([1, 2], [40, 50])
    with pytest.raises(ValueError, match="both 'design'"):
        bx.regressBatches(one, batch=batch, design=design, d=5, deferred=True)
    with pytest.raises(ValueError, match="both 'design'"):
        bx.regressBatches(one, batch=batch, keep=[1], d=5, deferred=True)
    for bad in (0.0, -1e-9, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="pca_tol"):
            bx.regressBatches(*B, d=5, deferred=True, pca_tol=bad)
    with pytest.raises(ValueError, match="pca_maxit"):
        bx.regressBatches(*B, d=5, deferred=True, pca_maxit=0)
    with pytest.raises(ValueError, match="pca_iters"):
        bx.regressBatches(*B, d=5, deferred=True, pca_iters=0)
    with pytest.raises(AssertionError, match="require_gpu"):   # a good call gets as far as the device
        bx.regressBatches(*B, d=5, deferred=True, residuals=False)


def test_check_pca_and_null_handles_answer_without_a_device():
    L = _lib.lib()
    i32, f64 = ctypes.c_int32, ctypes.c_double

    def err(rc):
        assert rc != 0
        return L.bmx_last_error().decode()

    w = np.array([1.0, 2.0])
    assert L.bmx_linear_check_pca(i32(130), i32(70), i32(5), f64(1e-9), i32(500), None, i32(2)) == 0
    assert L.bmx_linear_check_pca(i32(130), i32(130), i32(120), f64(0.0), i32(1), _lib.f64p(w), i32(2)) == 0
    assert "n_pca_rows" in err(L.bmx_linear_check_pca(i32(130), i32(131), i32(5), f64(1e-9), i32(500), None, i32(2)))
    assert "n_pca_rows" in err(L.bmx_linear_check_pca(i32(130), i32(0), i32(5), f64(1e-9), i32(500), None, i32(2)))
    assert "d <= 120" in err(L.bmx_linear_check_pca(i32(130), i32(130), i32(121), f64(1e-9), i32(500), None, i32(2)))
    assert "d <= 120" in err(L.bmx_linear_check_pca(i32(130), i32(130), i32(0), f64(1e-9), i32(500), None, i32(2)))
    assert "exceeds" in err(L.bmx_linear_check_pca(i32(130), i32(4), i32(5), f64(1e-9), i32(500), None, i32(2)))
    assert "tolerance" in err(L.bmx_linear_check_pca(i32(130), i32(70), i32(5), f64(float("nan")), i32(500), None, i32(2)))
    assert "iteration" in err(L.bmx_linear_check_pca(i32(130), i32(70), i32(5), f64(1e-9), i32(0), None, i32(2)))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        wb = np.array([1.0, bad])
        assert "weights" in err(L.bmx_linear_check_pca(i32(130), i32(70), i32(5), f64(1e-9), i32(500), _lib.f64p(wb), i32(2)))
    out = np.zeros(8)
    handle = ctypes.c_void_p()
    assert "null handle" in err(L.bmx_residual_pca_create(i32(70), None, ctypes.byref(handle))) and not handle
    assert "null handle" in err(L.bmx_residual_pca_fit(None, None, i32(0), None, None, i32(0), None, i32(5), f64(1e-9),
                                                       i32(500), None, None, None, None, None, None))
    assert "null handle" in err(L.bmx_residual_pca_project(None, i32(0), _lib.f64p(out)))
    L.bmx_residual_pca_destroy.argtypes, L.bmx_residual_pca_destroy.restype = [ctypes.c_void_p], None
    L.bmx_residual_pca_destroy(None)


def test_entry_points_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "batchelor_mi355x.h")) as f:
        header = f.read()
    L = _lib.lib()
    for name in ENTRIES:
        assert re.search(r"\bint32_t\s+" + name + r"\s*\(", header), name
        assert hasattr(L, name), name
