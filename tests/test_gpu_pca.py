"""The device multiBatchPCA (csrc/pca.hip) and the stand-alone projection (csrc/prepca.hip) at their tile edges, against
the longdouble restatement of tests/pca_ref.py.

Two identities carry the tests; both hold for whatever `fit` returns, after one application of the operator or after
convergence, so they need no sign alignment and no spectral gap:
    Ritz identity        R^T M R = diag(s^2) and R^T R = I, with M rebuilt from the inputs
    projection identity  pcs[b] = (x_b diag(scale_b) - centers 1^T)^T R, from the device's own centers and R
The inputs and the allowances come from tests/pca_ref.py, which derives the allowances; tests/test_cpu_pca.py holds the
float64 restatement to them on every input used here and shows that they reject planted faults.  Every test prints the
device's error / allowance and asserts that it is at most 1."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import batchelor_amd as bx
from batchelor_amd import _lib
from batchelor_amd.inputs import canonical_csc
from tests import pca_ref as ref

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def device_fit(name):
    """One device run per case, shared by the tests: through multiBatchPCA, which must take the device path."""
    c, B = ref.case(name)
    out = bx.multiBatchPCA(*B, iters=c.iters, **c.kwargs())
    assert out["path"] == "device", out["path"]
    assert out["iters_used"] == c.iters if c.iters is not None else 1 <= out["iters_used"] <= 500
    np.testing.assert_array_equal(out["weights"], ref.weight_vector(c.sizes, c.weights))
    assert np.all(np.diff(out["d"]) <= 0) and np.all(out["d"] >= 0)
    return out


@pytest.mark.parametrize("name", ref.FIXED + ref.CONVERGED)
def test_ritz_identity(name):
    ex, al = ref.reference(name)
    r = ref.fit_ratios(ex, al, device_fit(name))
    print(f"{name}: device error / allowance: Ritz defect {r['ritz']:.3g}, R^T R - I {r['orth']:.3g}, centres {r['centers']:.3g}")
    assert all(v <= 1.0 for v in r.values()), r


@pytest.mark.parametrize("name", ref.FIXED + ref.CONVERGED)
def test_projection_identity(name):
    ex, al = ref.reference(name)
    ratio = ref.projection_ratio(ex, al, device_fit(name))
    print(f"{name}: device projection error / allowance, every cell and component: {ratio:.3g}")
    assert ratio <= 1.0


@pytest.mark.parametrize("name", ref.CONVERGED)
def test_reported_residual_is_the_residual(name):
    ex, al = ref.reference(name)
    fit = device_fit(name)
    res = ref.residual_ratios(ex, al, fit, ref.TOL)
    print(f"{name}: {fit['iters_used']} applications; residual recomputed {res['true']:.4g}, reported {res['reported']:.4g}, "
          f"allowance {res['allow']:.3g}: over tol by {res['over_tol']:.3g} allowances, reported off by "
          f"{res['reported_off']:.3g} allowances")
    assert fit["residual"] <= ref.TOL
    assert res["over_tol"] <= 1.0 and res["reported_off"] <= 1.0


def _run_handle(B, w, c, blocked):
    pca = bx.DevicePCA(c.G)
    try:
        for m, wi in zip(B, w):
            if blocked:
                pca.begin_batch(m.shape[1], weight=wi, cos_norm=c.cos_norm)
                for a in range(0, m.shape[1], 37):
                    pca.add_block(m[:, a:a + 37])
            else:
                pca.add_batch(m, weight=wi, cos_norm=c.cos_norm)
        out = pca.fit(d=c.d, iters=c.iters)
        out["pcs"] = [pca.project(b) for b in range(len(B))]
    finally:
        pca.close()
    return out


def test_blocked_upload_and_repeat_are_bitwise_equal():
    """add_batch, add_batch again, and begin_batch + add_block in blocks of 37 cells: the per-cell norms and every sum
    order are the same, so the results are.  The only check of where add_block writes a block's norms."""
    name = "g130-three-cos-wn-i2"
    c, B = ref.case(name)
    w = ref.weight_vector(c.sizes, c.weights)
    first, again, blocked = _run_handle(B, w, c, False), _run_handle(B, w, c, False), _run_handle(B, w, c, True)
    for label, other in (("a second run", again), ("blocks of 37 cells", blocked)):
        same = {k: bool(np.array_equal(first[k], other[k])) for k in ("centers", "rotation", "d")}
        same["pcs"] = all(np.array_equal(p, q) for p, q in zip(first["pcs"], other["pcs"]))
        print(f"{name}, {label}: bitwise equal to the first run: {same}")
        assert all(same.values()), (label, same)
    ex, al = ref.reference(name)       # and the handle driven directly meets the identities too
    r = ref.fit_ratios(ex, al, blocked)
    r["projection"] = ref.projection_ratio(ex, al, blocked)
    print(f"{name}, blocked upload: device error / allowance {r}")
    assert all(v <= 1.0 for v in r.values())


@pytest.mark.parametrize("G,n,d,cos_norm", ref.PROJECT_SHAPES)
def test_standalone_project(G, n, d, cos_norm):
    x, rot, cen = ref.project_case(G, n, d, cos_norm)
    got = bx.project(x, rot, cen, cos_norm=cos_norm)
    ratio = ref.project_ratio(x, rot, cen, cos_norm, got)
    print(f"project G={G} n={n} d={d} cos_norm={cos_norm}: device error / allowance {ratio:.3g}")
    assert ratio <= 1.0


def test_standalone_project_refuses_more_than_256_dimensions():
    rng = np.random.default_rng(5)
    with pytest.raises(_lib.BatchelorMI355XError, match="more than 256 dimensions"):
        bx.project(rng.standard_normal((65, 17)), rng.standard_normal((65, 257)), np.zeros(65))


def test_error_paths_that_need_the_device():
    _, B = ref.case("g130-chunks-w-i1")
    pca = bx.DevicePCA(130)
    try:
        pca.add_batch(B[0])
        with pytest.raises(_lib.BatchelorMI355XError, match="has not been run"):
            pca.project(0)
        few = bx.DevicePCA(64)
        try:
            few.add_batch(np.ascontiguousarray(B[0][:64]))
            with pytest.raises(_lib.BatchelorMI355XError, match="d exceeds the number of genes"):
                few.fit(d=65, iters=1)
        finally:
            few.close()
        pca.begin_batch(B[1].shape[1])
        pca.add_block(B[1][:, :100])
        with pytest.raises(_lib.BatchelorMI355XError, match="has not received all its cells"):
            pca.fit(d=10, iters=1)
        pca.add_block(B[1][:, 100:])
        out = pca.fit(d=10, iters=1)           # and the handle is still good once the batch is complete
        assert out["rotation"].shape == (130, 10) and pca.project(1).shape == (513, 10)
    finally:
        pca.close()


def _contract_handle(kind):
    """ref.contract_case() resident in a DevicePCA, or as CSC of the same matrices in a DeviceSparsePCA."""
    B = ref.contract_case()
    pca = bx.DevicePCA(B[0].shape[0]) if kind == "dense" else bx.DeviceSparsePCA(B[0].shape[0])
    for m in B:
        pca.add_batch(m if kind == "dense" else canonical_csc(sp.csc_matrix(m))[0])
    return pca


@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_fit_contract_of_both_handles(kind):
    """What DevicePCA and DeviceSparsePCA share since they run one iteration: the refusals and their messages; a
    refused fit leaves the handle unfitted whatever an earlier fit had left, and a repeat of the earlier fit gives its
    bits again; a fit that misses its tolerance has written its results, the wrapper knows its d, and project() works."""
    B = ref.contract_case()
    pca = _contract_handle(kind)
    try:
        for kwargs, text in (({"d": 0}, "the device PCA takes 1 <= d <= 120"),
                             ({"d": 121}, "the device PCA takes 1 <= d <= 120"),
                             ({"d": 131}, "the device PCA takes 1 <= d <= 120"),   # (checked before d > 130 genes,
                             # which test_error_paths_that_need_the_device reaches at 64 genes)
                             ({"d": 5, "max_iters": 0}, "the PCA needs at least one iteration"),
                             ({"d": 5, "tol": 0.0}, "the PCA tolerance must be positive")):
            with pytest.raises(_lib.BatchelorMI355XError) as info:
                pca.fit(**kwargs)
            print(f"{kind}: fit({kwargs}) refused with: {info.value}")
            assert text in str(info.value), (kwargs, str(info.value))
        first = pca.fit(d=5, iters=2)
        first["pcs"] = [pca.project(b) for b in range(len(B))]
        with pytest.raises(_lib.BatchelorMI355XError, match="the device PCA takes 1 <= d <= 120"):
            pca.fit(d=121, iters=2)
        with pytest.raises(_lib.BatchelorMI355XError, match="has not been run"):
            pca.project(0)
        again = pca.fit(d=5, iters=2)
        again["pcs"] = [pca.project(b) for b in range(len(B))]
        same = {k: bool(np.array_equal(first[k], again[k])) for k in ("centers", "rotation", "d")}
        same["pcs"] = all(np.array_equal(p, q) for p, q in zip(first["pcs"], again["pcs"]))
        print(f"{kind}: the good fit repeated after a refused one, bitwise equal to the first: {same}")
        assert all(same.values()), same
        # one application cannot reach 1e-9 on this input (tests/test_cpu_pca.py::test_contract_case_needs_more_than_one_step)
        with pytest.raises(_lib.BatchelorMI355XError, match="did not reach the tolerance"):
            pca.fit(d=5, tol=ref.TOL, max_iters=1)
        print(f"{kind}: after max_iters=1: iters_used {pca.iters_used}, residual {pca.residual:.3g}, wrapper d {pca.d}")
        assert pca.iters_used == 1 and np.isfinite(pca.residual) and pca.residual > ref.TOL and pca.d == 5
        pcs = pca.project(0)
        assert pcs.shape == (257, 5) and np.all(np.isfinite(pcs))
    finally:
        pca.close()
