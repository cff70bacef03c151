"""subset_row / get_all_genes / get_variance without a device: the float64 restatement of the streaming pass
(tests/pca_genes_ref.py) meets every allowance on every input the device tests use and each planted fault is far
outside; multiBatchPCA_host with the three arguments against the reference's own words; the argument handling; the
bmx_pca_genes_* entry points' null-handle contract.

Smallest factor by which a planted fault missed its allowance, over all cases and faults (printed by
test_planted_faults_are_far_outside): 9.2e5 ("inv_offset" on case f, where the second block of 37 cells reads the first
block's norms); the next smallest is 1.4e9 ("n_minus_one" on case d, 4100 cells in a batch)."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import pca_genes_ref as ref
from tests import pca_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from batchelor_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def fit_on_subset(name):
    """pca_ref's float64 fit on the subset rows: what the streaming pass borrows."""
    c, B, subset1 = ref.case(name)
    sub = subset1 - 1
    return pca_ref.fixed_count_f64([b[sub] for b in B], c.weights, c.cos_norm, c.d, c.iters)


def _d_ok(c):
    return c.d <= pca_ref.width(c.d) - 8 and c.nS >= pca_ref.width(c.d)


RESTATED = [k for k in ref.DEVICE if _d_ok(ref.CASES[k])]


def test_every_device_case_is_restated():
    assert RESTATED == ref.DEVICE


@pytest.mark.parametrize("name,block", [(k, None) for k in RESTATED] + [("a", 37), ("a", 1), ("f", 37)])
def test_restatement_meets_the_allowances(name, block):
    c, B, subset1 = ref.case(name)
    got = ref.stream_f64(B, subset1, fit_on_subset(name), c.weights, c.cos_norm, block=block)
    r = ref.ratios(ref.reference(name), got)
    print(f"case {name}, block {block}: float64 error / allowance {r}")
    assert all(v <= 1.0 for v in r.values()), r
    assert ref.assembly_ok(subset1, got, fit_on_subset(name))
    assert np.array_equal(got["var_explained"], got["d"] ** 2 / len(B))


def test_planted_faults_are_far_outside():
    smallest = np.inf
    for name in RESTATED:
        c, B, subset1 = ref.case(name)
        ex, fit = ref.reference(name), fit_on_subset(name)
        for fault in ref.FAULTS:
            if fault in ref.NEEDS_COS and not c.cos_norm:
                continue
            got = ref.stream_f64(B, subset1, fit, c.weights, c.cos_norm, block=37, fault=fault)
            if fault == "sorted_subset":
                assert not ref.assembly_ok(subset1, got, fit), name
                continue
            r = ref.ratios(ex, got)
            factor = max(r["rotation_left"], r["centers_left"], r["var_total"])
            print(f"case {name}, {fault}: error / allowance {factor:.3g}")
            assert factor > 1e3, (name, fault, r)
            smallest = min(smallest, factor)
    print(f"smallest factor by which a planted fault missed its allowance: {smallest:.3g}")


@pytest.mark.parametrize("name", RESTATED)
def test_centring_term_left_out_everywhere_is_harmless(name):
    c, B, subset1 = ref.case(name)
    got = ref.stream_f64(B, subset1, fit_on_subset(name), c.weights, c.cos_norm, fault=ref.HARMLESS)
    r = ref.ratios(ref.reference(name), got)
    print(f"case {name}: mu_L t^T left out of every batch: error / allowance {r}")
    assert all(v <= 1.0 for v in r.values()), r


# ------------------------------------------------------------------------------------- the host path
def _host_record(B, subset1, c_kwargs, **more):
    import batchelor_amd as bx
    l2 = None
    if c_kwargs.get("cos_norm"):
        l2 = [np.sqrt((b[subset1 - 1] ** 2).sum(axis=0)) for b in B]
    return bx.multiBatchPCA_host(*B, d=c_kwargs["d"], weights=c_kwargs["weights"], l2=l2, subset_row=subset1, **more)


@pytest.mark.parametrize("name", ["a", "e", "f"])
def test_host_path_meets_the_identities(built, name):
    """The host fallback's own arithmetic (case e is the one the device front end sends there); its pcs are
    numpy's here."""
    c, B, subset1 = ref.case(name)
    rec = _host_record(B, subset1, c.kwargs(), get_all_genes=True, get_variance=True)
    sub = subset1 - 1
    assert rec["rotation"].shape == (c.G_all, c.d) and rec["centers"].shape == (c.G_all,)
    rec["pcs"] = [pca_ref.project_f64(b[sub], rec["rotation"][sub], rec["centers"][sub], c.cos_norm) for b in B]
    r = ref.ratios(ref.reference(name), rec)
    print(f"case {name}: multiBatchPCA_host error / allowance {r}")
    assert all(v <= 1.0 for v in r.values()), r
    assert np.array_equal(rec["var_explained"], rec["d"] ** 2 / len(B))


@pytest.mark.parametrize("cos_norm,weights", [(False, None), (True, (1.0, 2.0, 0.5))])
def test_host_path_against_the_reference_word_for_word(built, cos_norm, weights):
    B, subset1, d = ref.planted_case()
    rec = _host_record(B, subset1, {"d": d, "weights": weights, "cos_norm": cos_norm}, get_all_genes=True, get_variance=True)
    lit = ref.literal(B, subset1, weights, cos_norm, d)
    bounds = ref.literal_bounds(lit, d)
    sub, left = ref.split_rows(B[0].shape[0], subset1)
    sign = np.sign((rec["rotation"][sub] * lit["rotation"][sub]).sum(axis=0))
    assert np.all(sign != 0)
    diff = np.linalg.norm(rec["rotation"][left] * sign[None, :] - lit["rotation"][left], axis=0)
    ratio = {"columns": float((diff / bounds["columns"]).max()),
             "var_explained": float((np.abs(rec["var_explained"] - lit["var_explained"]) / bounds["var_explained"]).max()),
             "var_total": abs(rec["var_total"] - lit["var_total"]) / bounds["var_total"]}
    print(f"cos_norm={cos_norm}: host vs literal, difference / bound {ratio}; leftover columns have norm "
          f"{np.linalg.norm(lit['rotation'][left], axis=0)}")
    assert all(v <= 1.0 for v in ratio.values()), ratio
    cen = ref.exact(B, subset1, weights, cos_norm)
    assert pca_ref.worst(rec["centers"][left] - lit["centers"][left], 2 * cen.centers_left_allow()) <= 1.0
    assert np.linalg.norm(lit["rotation"][left], axis=0).min() > 0.05   # (the comparison is not of zeros)


def test_subset_forms_and_rules(built):
    import batchelor_amd as bx
    c, B, subset1 = ref.case("b")
    kw = {"d": 5, "weights": None, "cos_norm": False}
    by_index = _host_record(B, subset1, kw, get_all_genes=True, get_variance=True)
    # a logical mask names the rows in ascending order: the same call as the sorted indices
    mask = np.zeros(c.G_all, dtype=bool)
    mask[subset1 - 1] = True
    by_mask = bx.multiBatchPCA_host(*B, d=5, subset_row=mask, get_all_genes=True, get_variance=True)
    by_sorted = bx.multiBatchPCA_host(*B, d=5, subset_row=np.sort(subset1), get_all_genes=True, get_variance=True)
    for k in ("rotation", "centers", "d", "var_total", "var_explained"):
        assert np.array_equal(by_mask[k], by_sorted[k]), k
    assert by_index["rotation"].shape == (c.G_all, 5)
    # without get_all_genes the record covers the subset rows, in the subset's order: the call on x[subset]
    plain = bx.multiBatchPCA_host(*[b[subset1 - 1] for b in B], d=5)
    only = bx.multiBatchPCA_host(*B, d=5, subset_row=subset1)
    assert np.array_equal(only["rotation"], plain["rotation"]) and np.array_equal(only["centers"], plain["centers"])
    assert "var_total" not in only
    assert np.array_equal(by_index["rotation"][subset1 - 1], plain["rotation"])
    # get_all_genes without a subset, or with a subset that leaves nothing out, changes nothing
    every = np.random.default_rng(0).permutation(c.G_all) + 1
    for sr in (None, every):
        a = bx.multiBatchPCA_host(*B, d=5, subset_row=sr)
        b = bx.multiBatchPCA_host(*B, d=5, subset_row=sr, get_all_genes=True)
        assert np.array_equal(a["rotation"], b["rotation"]) and np.array_equal(a["centers"], b["centers"])
    # a row named twice: both copies go into the PCA, the later one's rotation row is the one kept
    twice = np.concatenate([subset1[:20], subset1[3:4], subset1[20:]])
    rec = bx.multiBatchPCA_host(*B, d=5, subset_row=twice, get_all_genes=True)
    sub_fit = bx.multiBatchPCA_host(*[b[twice - 1] for b in B], d=5)
    assert rec["rotation"].shape == (c.G_all, 5)
    assert np.array_equal(rec["rotation"][twice[20] - 1], sub_fit["rotation"][20])
    assert ref.assembly_ok(twice, rec, sub_fit)
    # out of range, for every front end that takes the argument, before any device is asked for
    for bad in ([0, 1, 2], [1, c.G_all + 1], np.ones(c.G_all + 1, dtype=bool)):
        for call in (lambda: bx.multiBatchPCA_host(*B, d=5, subset_row=bad),
                     lambda: bx.multiBatchPCA(*B, d=5, subset_row=bad),
                     lambda: bx.cosineNorm(B[0], subset_row=bad)):
            with pytest.raises(ValueError, match="subset indices out of range"):
                call()


def test_reconstructed_selects_rows_and_cells(built):
    from batchelor_amd.fast_mnn import FastMnnResult
    rng = np.random.default_rng(3)
    rot, cor = rng.standard_normal((30, 4)), rng.standard_normal((50, 4))
    res = FastMnnResult(corrected=cor, batch=np.zeros(50), rotation=rot, centers=np.zeros(30), merge_info=None)
    assert res.var_explained is None and res.var_total is None
    assert np.array_equal(res.reconstructed(), rot @ cor.T)
    rows, cells = np.array([7, 0, 29]), np.arange(50) % 3 == 0
    assert np.array_equal(res.reconstructed(rows, cells), rot[rows] @ cor[cells].T)
    assert np.array_equal(res.reconstructed(rows=slice(2, 9)), rot[2:9] @ cor.T)
    assert res.reconstructed(rows=5, cells=[1, 2]).shape == (1, 2)


# ------------------------------------------------------------------------------------- the C entry points
GENES_ENTRIES = {   # name: argument types after the handle
    "bmx_pca_genes_begin_batch": [ctypes.c_int32],
    "bmx_pca_genes_add_block": [ctypes.c_void_p, ctypes.c_int64],
    "bmx_pca_genes_finish": [ctypes.c_void_p, ctypes.c_void_p],
    "bmx_pca_genes_total_variance": [ctypes.c_void_p],
}


def test_genes_entry_points_refuse_a_null_handle(built):
    lib = built.lib()
    header = open(os.path.join(ROOT, "include", "batchelor_mi355x.h")).read()
    for name in list(GENES_ENTRIES) + ["bmx_pca_genes_create", "bmx_pca_genes_destroy"]:
        assert hasattr(lib, name) and name + "(" in header, name
    lib.bmx_pca_genes_destroy.argtypes, lib.bmx_pca_genes_destroy.restype = [ctypes.c_void_p], None
    lib.bmx_pca_genes_destroy(None)   # a no-op
    for name, types in GENES_ENTRIES.items():
        fn = getattr(lib, name)
        saved = fn.argtypes, fn.restype
        fn.argtypes, fn.restype = [ctypes.c_void_p] + types, ctypes.c_int32
        try:
            rc = fn(None, *[None if t is ctypes.c_void_p else t(1) for t in types])
        finally:
            fn.argtypes, fn.restype = saved
        assert rc == -6, (name, rc)
        assert lib.bmx_last_error().decode() == "null handle", (name, lib.bmx_last_error().decode())
    # create: a null PCA is a null handle too, and the output pointer is looked at first
    out = ctypes.c_void_p()
    lib.bmx_pca_genes_create.argtypes = [ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    try:
        assert lib.bmx_pca_genes_create(3, None, ctypes.byref(out)) == -6
        assert lib.bmx_last_error().decode() == "null handle" and not out.value
        assert lib.bmx_pca_genes_create(3, None, None) == -6
        assert lib.bmx_last_error().decode() == "null output pointer"
    finally:
        lib.bmx_pca_genes_create.argtypes = None
