"""The device PCA's checks without a GPU: the float64 restatement (tests/pca_ref.py) is held to every allowance on every
input that tests/test_gpu_pca.py uses, and the same checks reject the restatement with one planted fault.

The allowances are derived in the docstring of tests/pca_ref.py from the lengths of the sums involved; nothing here or in
the GPU tests is fitted to a result.  Every test prints the error / allowance ratios it asserts on."""
import numpy as np
import pytest

from tests import pca_ref as ref


def f64_fit(name, fault=None, iters=None):
    c, B = ref.case(name)
    iters = iters or (c.iters if c.iters is not None else ref.F64_ITERS_CONVERGED)
    return ref.fixed_count_f64(B, c.weights, c.cos_norm, c.d, iters, fault=fault)


@pytest.mark.parametrize("name", ref.FIXED + ref.CONVERGED)
def test_float64_restatement_stays_inside_the_allowances(name):
    """Completing at all is the condition on the inputs: every block the restatement orthonormalises has a positive
    definite Gram matrix, so the device path is expected to take the case."""
    c, _ = ref.case(name)
    ex, al = ref.reference(name)
    fit = f64_fit(name)
    r = ref.fit_ratios(ex, al, fit)
    r["projection"] = ref.projection_ratio(ex, al, fit)
    line = ", ".join(f"{k} {v:.3g}" for k, v in r.items())
    if c.iters is None:
        res = ref.residual_ratios(ex, al, fit, ref.TOL)
        line += (f"; residual {res['true']:.3g} (own figure {res['reported']:.3g}, allowance {res['allow']:.3g}): "
                 f"over tol {res['over_tol']:.3g}, own figure off {res['reported_off']:.3g}")
        r.update(over_tol=res["over_tol"], reported_off=res["reported_off"])
    print(f"{name}: float64 restatement error / allowance: {line}")
    assert all(v <= 1.0 for v in r.values()), r


# which check must reject which fault, and the cases it is planted in: every fixed-count case where the fault changes
# the identity it is checked by
def _applies(fault, c):
    if fault == "scale_once":
        return c.cos_norm
    if fault == "no_centring_term":        # one batch: mu is its mean and the term is mu (1^T Z) = 0
        return len(c.sizes) > 1
    if fault == "n_minus_one":
        return min(c.sizes) > 1
    if fault == "drop_last_gene":
        # G = L: the block is the whole space, the Ritz vectors are exact eigenvectors of the operator without the gene, they
        # are zero in that gene, and on such vectors the two operators agree.  The identity holds; nothing to reject.
        # Two steps: the first leaves the whole block zero in that gene, with the same end.  One step from the random start
        # shows the fault at full size; in a converged run it is the recomputed residual that does not fall for it.
        return c.G > ref.width(c.d) and c.iters == 1
    return True


OPERATOR_FAULTS = [f for f in ref.FAULTS if not f.startswith("projection")]


@pytest.mark.parametrize("fault", ref.FAULTS)
def test_planted_fault_is_rejected(fault):
    seen = []
    for name in ref.FIXED:
        c, _ = ref.case(name)
        if not _applies(fault, c):
            continue
        ex, al = ref.reference(name)
        fit = f64_fit(name, fault)
        if fault in OPERATOR_FAULTS:
            ratio = ref.worst(ex.ritz_defect(fit["rotation"], fit["d"]), al.ritz(fit["rotation"], fit["d"]))
        else:
            ratio = ref.projection_ratio(ex, al, fit)
        print(f"{fault} in {name}: error / allowance {ratio:.3g}")
        assert ratio > 1.0, (fault, name, ratio)
        seen.append(name)
    assert len(seen) >= 5
    if fault == "drop_last_gene":      # also where the products over genes are split, the last gene in the last split
        assert "g2100-gsplit4-d57-i1" in seen and "g1100-gsplit2-cos-w-i1" in seen


def test_the_rank_one_term_cancels_over_the_batches():
    """Left out of EVERY batch the centring term is no fault (tests/pca_ref.py, at FAULTS): the check must not cry wolf."""
    for name in ("g130-three-w-i2", "g65-clamp-cos-w-i1"):
        ex, al = ref.reference(name)
        fit = f64_fit(name, ref.HARMLESS)
        ratio = ref.worst(ex.ritz_defect(fit["rotation"], fit["d"]), al.ritz(fit["rotation"], fit["d"]))
        print(f"{name}: the rank-one term left out of every batch: Ritz defect / allowance {ratio:.3g}")
        assert ratio <= 1.0


def test_a_fault_in_the_residual_is_rejected():
    """A restatement that reports the residual of d - 1 of its d pairs, or of all genes but one.  Three steps in, where the
    residual is of the size a converged device run reports (far above rounding), not at the restatement's own 1e-15."""
    for name in ref.CONVERGED:
        c, _ = ref.case(name)
        ex, al = ref.reference(name)
        fit = f64_fit(name, iters=3)
        honest = ref.residual_ratios(ex, al, fit, ref.TOL)
        print(f"{name}, three steps: residual {honest['true']:.3g}, own figure off by {honest['reported_off']:.3g} allowances")
        assert honest["reported_off"] <= 1.0
        R, s = fit["rotation"], fit["d"]
        D = np.asarray(ex.apply(R) - R * (np.asarray(s, dtype=ref.LD) ** 2)[None, :], dtype=np.float64)
        norms = np.sqrt((D * D).sum(axis=0))
        worst_col = int(np.argmax(norms))
        without_col = np.delete(norms, worst_col).max() if c.d > 1 else 0.0
        worst_gene = int(np.argmax(np.abs(D[:, worst_col])))
        without_gene = np.sqrt((np.delete(D, worst_gene, axis=0) ** 2).sum(axis=0)).max()
        for what, value in (("worst pair left out", without_col), ("one gene left out", without_gene)):
            bad = dict(fit, residual=value / float(s[0]) ** 2)
            res = ref.residual_ratios(ex, al, bad, ref.TOL)
            print(f"{name}, {what}: reported {res['reported']:.3g} against {res['true']:.3g}: "
                  f"off by {res['reported_off']:.3g} allowances")
            assert res["reported_off"] > 1.0


@pytest.mark.parametrize("G,n,d,cos_norm", ref.PROJECT_SHAPES)
def test_float64_projection_stays_inside_the_allowance(G, n, d, cos_norm):
    x, rot, cen = ref.project_case(G, n, d, cos_norm)
    good = ref.project_ratio(x, rot, cen, cos_norm, ref.project_f64(x, rot, cen, cos_norm))
    no_off = ref.project_ratio(x, rot, cen, cos_norm, ref.project_f64(x, rot, 0.0 * cen, cos_norm))
    print(f"project G={G} n={n} d={d} cos_norm={cos_norm}: float64 error / allowance {good:.3g}; without the centres {no_off:.3g}")
    assert good <= 1.0 < no_off


def test_case_table_covers_what_it_claims():
    cases = [ref.CASES[k] for k in ref.CASES]
    assert {c.G for c in cases} >= {64, 65, 95, 96, 130, 333, 128, 129, 191, 1100, 1600, 2100}
    assert {c.G // 512 for c in cases} >= {0, 2, 3, 4} and 1100 - 576 == 16 * 32 + 12     # the gene splits (pca_ref.py)
    assert {c.d for c in cases} == {1, 10, 56, 57, 80, 120}
    assert {c.sizes for c in cases} >= {(1, 2, 63, 70), (31, 33, 64, 65), (257, 513), (4100, 300), (6149,)}
    assert {sum(c.sizes) - ref.width(c.d) for c in cases} >= {1}
    for cos in (False, True):
        kinds = {("sizes" if c.weights is False else "equal" if c.weights is None else "vector") for c in cases
                 if c.cos_norm == cos and len(c.sizes) > 1}
        assert kinds == {"sizes", "equal", "vector"}, (cos, kinds)
    assert any(c.cos_norm and len(c.sizes) == 3 and c.weights is not None for c in cases)
    assert any(len(c.sizes) == 3 and isinstance(c.weights, tuple) for c in cases)
    assert {c.iters for c in cases} == {1, 2, None}
    assert sum(c.zero is not None for c in cases) >= 4 and all(c.cos_norm for c in cases if c.zero is not None)
    for c in cases:   # where the zero cell is: the middle of its batch
        if c.zero is not None:
            assert 0 < c.zero[1] < c.sizes[c.zero[0]] - 1
    assert 20 <= len(cases) <= 30


def test_contract_case_needs_more_than_one_step():
    """The input of test_gpu_pca.py::test_fit_contract_of_both_handles cannot be fitted to TOL by one application of the
    operator: the host PCA shows a flat spectrum (no gap for a single step to exploit), and one power step of the float64
    restatement leaves a residual many orders above TOL from any of several start blocks."""
    from batchelor_amd import multiBatchPCA_host
    B = ref.contract_case()
    s = multiBatchPCA_host(*B, d=64)["d"]
    resid = [ref.fixed_count_f64(B, None, False, 5, 1, seed=seed)["residual"] for seed in range(4)]
    print(f"contract case: (s_6 / s_1)^2 = {(s[5] / s[0]) ** 2:.3g}, (s_64 / s_1)^2 = {(s[63] / s[0]) ** 2:.3g}; residual "
          f"after one application from 4 start blocks: {min(resid):.3g} .. {max(resid):.3g}")
    assert (s[63] / s[0]) ** 2 > 0.05
    assert min(resid) > 1e6 * ref.TOL
