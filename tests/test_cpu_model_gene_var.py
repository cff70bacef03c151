"""modelGeneVar / combineVar / getTopHVGs, batchCorrect and its Param classes, noCorrect, intersectRows and quickCorrect:
everything that needs no device -- the host-side functions against tests/model_gene_var_ref.py, the dispatch, and the
argument checks of the bmx_genevar_* entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from tests import model_gene_var_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BMX_ERR_ARG = -6


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from batchelor_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def bx(built):
    import batchelor_amd
    return batchelor_amd


def table(bx, total, bio=None, n_cells=10, gene_index=None, mean=None):
    total = np.asarray(total, dtype=np.float64)
    return bx.GeneVarTable(mean=np.zeros(total.size) if mean is None else np.asarray(mean, dtype=np.float64), total=total,
                           tech=None if bio is None else total - np.asarray(bio, dtype=np.float64),
                           bio=None if bio is None else np.asarray(bio, dtype=np.float64), n_cells=n_cells,
                           gene_index=gene_index)


# ------------------------------------------------------------------------------------------------------- getTopHVGs
def test_top_hvgs_order_ties_nan_and_threshold(bx):
    v = [0.5, 2.0, np.nan, 2.0, -1.0, 0.0, 3.0]
    t = table(bx, v)
    assert bx.getTopHVGs(t).tolist() == [7, 2, 4, 1]                      # > 0, ties by ascending index, NaN never
    assert bx.getTopHVGs(t, var_threshold=None).tolist() == [7, 2, 4, 1, 6, 5]
    assert bx.getTopHVGs(t, var_threshold=0.5).tolist() == [7, 2, 4]
    for kw in ({}, {"var_threshold": None}, {"var_threshold": 1.0}, {"n": 3}, {"prop": 0.5}, {"n": 2, "prop": 0.5},
               {"n": 5, "prop": 0.1}, {"n": 0}):
        assert bx.getTopHVGs(t, **kw).tolist() == ref.top_hvgs(v, **{"var_threshold": 0, **kw}).tolist(), kw


def test_top_hvgs_n_against_prop(bx):
    t = table(bx, np.arange(10, 0, -1.0))
    assert bx.getTopHVGs(t, n=3).tolist() == [1, 2, 3]
    assert bx.getTopHVGs(t, prop=0.5).tolist() == [1, 2, 3, 4, 5]
    assert bx.getTopHVGs(t, n=3, prop=0.5).tolist() == [1, 2, 3, 4, 5]     # the larger of the two
    assert bx.getTopHVGs(t, n=7, prop=0.5).tolist() == [1, 2, 3, 4, 5, 6, 7]
    assert bx.getTopHVGs(t, n=100).tolist() == list(range(1, 11))


def test_top_hvgs_field_and_gene_index(bx):
    t = table(bx, [1.0, 2.0, 3.0], bio=[0.3, -0.2, 0.1], gene_index=np.array([11, 5, 8]))
    assert bx.getTopHVGs(t).tolist() == [11, 8]                           # `bio` by default when the table has it
    assert bx.getTopHVGs(t, var_field="total").tolist() == [8, 5, 11]
    with pytest.raises(ValueError, match="no field"):
        bx.getTopHVGs(table(bx, [1.0]), var_field="bio")


# ------------------------------------------------------------------------------------------------------- combineVar
def test_combine_var_weights(bx):
    rng = np.random.default_rng(5)
    tabs = [table(bx, rng.random(6), bio=rng.random(6), n_cells=c, mean=rng.random(6)) for c in (5, 50, 20)]
    for equi in (True, False):
        got = bx.combineVar(*tabs, equiweight=equi)
        for f in ("mean", "total", "tech", "bio"):
            want = ref.combine_var([getattr(t, f) for t in tabs], [t.n_cells for t in tabs], equi).astype(np.float64)
            np.testing.assert_allclose(getattr(got, f), want, rtol=8 * ref.U, atol=0)
        assert got.per_block == tabs and got.n_cells == 75
    assert not np.array_equal(bx.combineVar(*tabs).total, bx.combineVar(*tabs, equiweight=False).total)


def test_combine_var_leaves_out_small_blocks(bx):
    a, b, one = table(bx, [1.0, 2.0], n_cells=4), table(bx, [3.0, 6.0], n_cells=2), table(bx, [np.nan, np.nan], n_cells=1)
    got = bx.combineVar(a, one, b)
    assert got.total.tolist() == [2.0, 4.0] and got.n_cells == 6 and len(got.per_block) == 3
    assert got.tech is None and got.bio is None
    assert np.array_equal(bx.combineVar(a, one).total, a.total)           # one table that counts: that table's bits
    assert np.isnan(bx.combineVar(one, one).total).all()
    with pytest.raises(ValueError, match="same number of genes"):
        bx.combineVar(a, table(bx, [1.0, 2.0, 3.0]))


def test_model_gene_var_argument_errors_need_no_device(bx):
    x = np.ones((3, 4))
    with pytest.raises(ValueError, match="at least two cells"):
        bx.modelGeneVar(x[:, :1])
    with pytest.raises(ValueError, match="no block has at least two cells"):
        bx.modelGeneVar(x, block=[1, 2, 3, 4])
    with pytest.raises(ValueError, match="selects no genes"):
        bx.modelGeneVar(x, subset_row=[])
    with pytest.raises(ValueError, match="out of range"):
        bx.modelGeneVar(x, subset_row=[4])
    with pytest.raises(ValueError, match="callable"):
        bx.modelGeneVar(x, trend_fit=3)
    with pytest.raises(ValueError):
        bx.modelGeneVar(x, block=[1, 2])


def test_restatement_shows_the_one_pass_form_outside_the_allowance():
    """Values far from zero with a small spread: the two-pass restatement in float64 keeps within the allowance of the
    long-double one, the one-pass form does not."""
    for offset, scale in ((10.0, 1e-3), (1e6, 1.0)):
        x = ref.gaussian(65, 513, 3, offset, scale)
        _, total = ref.mean_var(x)
        _, allow = ref.allowances(x)
        two_pass = np.var(x, axis=1, ddof=1)
        assert (np.abs(two_pass - total.astype(np.float64)) <= allow).all()
        worst = np.abs(ref.one_pass_total(x) - total.astype(np.float64)) / allow
        print(f"offset {offset:g}: the one-pass form misses by up to {worst.max():.3g} allowances")
        assert worst.max() > 1.0


# ------------------------------------------------------------------------------------------------------- intersectRows
def test_intersect_rows_order_and_subsets(bx):
    a, b = np.arange(12.0).reshape(4, 3), 100 + np.arange(10.0).reshape(5, 2)
    names = (["g1", "g2", "g3", "g4"], ["g4", "x", "g2", "g1", "y"])
    (ia, ib), uni = bx.intersectRows(a, b, row_names=names)
    assert uni == ["g1", "g2", "g4"]                                       # the first batch's order
    assert np.array_equal(ia, a[[0, 1, 3]]) and np.array_equal(ib, b[[3, 2, 0]])
    (sa, sb), rows = bx.intersectRows(a, b, row_names=names, subset_row=["g4", "g1"])
    assert rows == ["g4", "g1"] and np.array_equal(sa, a[[3, 0]]) and np.array_equal(sb, b[[0, 3]])
    (ka, kb), rows = bx.intersectRows(a, b, row_names=names, subset_row=["g4"], keep_all=True)
    assert rows == uni and np.array_equal(ka, ia) and np.array_equal(kb, ib)
    same = (["p", "q", "r", "s"],) * 2
    (na, _), rows = bx.intersectRows(a, a + 1, row_names=same, subset_row=[3, 1])   # same names: indices are allowed
    assert rows == ["r", "p"] and np.array_equal(na, a[[2, 0]])
    (csc, _), _ = bx.intersectRows(sp.csc_matrix(a), sp.csc_matrix(b), row_names=names)
    assert sp.issparse(csc) and np.array_equal(csc.toarray(), ia)


def test_intersect_rows_errors(bx):
    a, b = np.zeros((2, 3)), np.zeros((2, 2))
    with pytest.raises(ValueError, match="no genes remaining in the intersection"):
        bx.intersectRows(a, b, row_names=(["a", "b"], ["c", "d"]))
    with pytest.raises(ValueError, match="only character 'subset.row' is allowed when '...' have different rownames"):
        bx.intersectRows(a, b, row_names=(["a", "b"], ["b", "a"]), subset_row=[1])
    with pytest.raises(ValueError, match="one sequence of names per batch"):
        bx.intersectRows(a, b, row_names=(["a", "b"],))
    with pytest.raises(ValueError, match="name every row"):
        bx.intersectRows(a, b, row_names=(["a"], ["a", "b"]))
    with pytest.raises(ValueError, match="not in the intersection"):
        bx.intersectRows(a, b, row_names=(["a", "b"], ["a", "b"]), subset_row=["z"])


# ------------------------------------------------------------------------------------------------------- noCorrect
def test_no_correct_dense_and_csc(bx):
    rng = np.random.default_rng(2)
    a, b = rng.random((5, 3)), rng.random((5, 4))
    out = bx.noCorrect(a, b)
    assert out.corrected.flags.f_contiguous and np.array_equal(out.corrected, np.hstack([a, b]))
    assert out.batch.tolist() == [1, 1, 1, 2, 2, 2, 2]
    assert bx.noCorrect(a, b, names=["x", "y"]).batch.tolist() == ["x"] * 3 + ["y"] * 4
    sub = bx.noCorrect(a, b, subset_row=[4, 2])
    assert np.array_equal(sub.corrected, np.hstack([a, b])[[3, 1]])
    assert bx.noCorrect(a, b, subset_row=[4, 2], correct_all=True).corrected.shape == (5, 7)
    sa, sb = sp.csr_matrix(a * (a > 0.5)), sp.csc_matrix(b * (b > 0.5))
    s = bx.noCorrect(sa, sb, subset_row=[1, 5])
    assert sp.issparse(s.corrected) and s.corrected.format == "csc"
    assert np.array_equal(s.corrected.toarray(), np.hstack([sa.toarray(), sb.toarray()])[[0, 4]])
    one = bx.noCorrect(a, batch=["u", "v", "u"])
    assert np.array_equal(one.corrected, a) and one.batch.tolist() == ["u", "v", "u"]


def test_no_correct_errors(bx):
    a, b = np.zeros((5, 3)), np.zeros((5, 4))
    with pytest.raises(ValueError, match="names of batches should be unique"):
        bx.noCorrect(a, b, names=["x", "x"])
    with pytest.raises(ValueError, match="number of rows is not the same across batches"):
        bx.noCorrect(a, np.zeros((4, 2)))
    with pytest.raises(ValueError, match="'batch' must be specified"):
        bx.noCorrect(a)
    with pytest.raises(ValueError, match="length"):
        bx.noCorrect(a, batch=[1, 2])
    with pytest.raises(TypeError, match="all sparse or all dense"):
        bx.noCorrect(a, sp.csc_matrix(b))


# ------------------------------------------------------------------------------------------------------- dispatch
def test_params_refuse_unknown_arguments(bx):
    for cls in (bx.FastMnnParam, bx.ClassicMnnParam, bx.RescaleParam, bx.RegressParam, bx.NoCorrectParam):
        with pytest.raises(ValueError, match="takes no argument 'bogus'"):
            cls(bogus=1)
        with pytest.raises(ValueError, match="an argument of batchCorrect"):
            cls(subset_row=[1])
        assert cls().args == {}
    assert bx.FastMnnParam(k=10, d=5).args == {"k": 10, "d": 5}
    assert bx.ClassicMnnParam(sigma=0.5).args == {"sigma": 0.5}
    with pytest.raises(ValueError):
        bx.RescaleParam(sigma=0.5)             # mnnCorrect's, not rescaleBatches'
    with pytest.raises(ValueError):
        bx.NoCorrectParam(k=3)


def test_batch_correct_reaches_the_function_the_param_names(bx):
    """Each target is recognised by an error of its own that it raises before it asks for a device, from an argument
    that came through the PARAM, next to arguments that came through batchCorrect."""
    a, b = np.ones((6, 5)), np.ones((6, 4))
    with pytest.raises(ValueError, match="'pca' should be one of 'device', 'host'"):
        bx.batchCorrect(a, b, PARAM=bx.FastMnnParam(pca="abacus"))
    with pytest.raises(ValueError, match="svd"):
        bx.batchCorrect(a, b, PARAM=bx.ClassicMnnParam(svd_dim=2))
    with pytest.raises(ValueError, match="'log_base' must be positive, finite and not 1"):
        bx.batchCorrect(a, b, PARAM=bx.RescaleParam(log_base=1))
    with pytest.raises(ValueError, match=r"'nrow\(design\)' should be equal to the total number of cells"):
        bx.batchCorrect(a, b, PARAM=bx.RegressParam(design=np.ones((3, 1))))
    # batchCorrect's own arguments arrive as well
    with pytest.raises(ValueError, match="'restrictions' must of length equal to the number of batches"):
        bx.batchCorrect(a, b, restrict=[None], PARAM=bx.RescaleParam())
    with pytest.raises(ValueError, match="subset indices out of range"):
        bx.batchCorrect(a, b, subset_row=[7], PARAM=bx.RescaleParam(log_base=3))
    with pytest.raises(ValueError, match="names of batches should be unique"):
        bx.batchCorrect(a, b, names=["x", "x"], PARAM=bx.RegressParam())
    with pytest.raises(TypeError, match="'PARAM' must be"):
        bx.batchCorrect(a, b, PARAM={"k": 3})
    with pytest.raises(TypeError):
        bx.batchCorrect(a, b)                  # PARAM is required


def test_no_correct_param_end_to_end(bx):
    rng = np.random.default_rng(3)
    a, b = rng.random((6, 5)), rng.random((6, 4))
    out = bx.batchCorrect(a, b, subset_row=[2, 3], restrict=["dropped", "as in the reference"], names=["p", "q"],
                          PARAM=bx.NoCorrectParam())
    assert isinstance(out, bx.NoCorrectResult)
    assert np.array_equal(out.corrected, np.hstack([a, b])[[1, 2]]) and out.batch.tolist() == ["p"] * 5 + ["q"] * 4
    full = bx.batchCorrect([a, b], subset_row=[2, 3], correct_all=True, PARAM=bx.NoCorrectParam())
    assert full.corrected.shape == (6, 9)


def test_quick_correct_checks_before_the_device(bx):
    a, b = np.ones((6, 5)), np.ones((6, 4))
    t = table(bx, np.ones(6))
    msg = r"'length\(precomputed\)' is not the same as the number of objects in '...'"
    with pytest.raises(ValueError, match=msg):
        bx.quickCorrect(a, b, precomputed=[t])
    with pytest.raises(ValueError, match=msg):
        bx.quickCorrect(a, batch=[1, 1, 2, 2, 2], precomputed=[t, t])
    with pytest.raises(ValueError, match="one row per gene"):
        bx.quickCorrect(a, b, precomputed=[t, table(bx, np.ones(5))])
    with pytest.raises(ValueError, match="'model_var_args' takes"):
        bx.quickCorrect(a, b, model_var_args={"block": [1]})
    with pytest.raises(ValueError, match="no genes remaining in the intersection"):
        bx.quickCorrect(a, b, row_names=(list("abcdef"), list("uvwxyz")))


def test_quick_counts_leave_a_gap_at_the_cut():
    """The seed of the quickCorrect tests: between the 150th and the 151st gene's variance lies far more than the
    allowance of the device's variances, so the chosen set cannot depend on their rounding."""
    from tests import multi_batch_norm_ref as norm_ref
    counts = ref.quick_counts()
    assert [c.shape for c in counts] == [(ref.QUICK_GENES, n) for n in ref.QUICK_SIZES]
    logcounts = norm_ref.multi_batch_norm(*counts)["logcounts"]
    hvgs, comb, gap, allow = ref.quick_choice(logcounts)
    print(f"gap at the cut {gap:.3g}, allowance {allow:.3g}")
    assert hvgs.size == ref.QUICK_N and gap > 1e6 * allow
    single = np.hstack(logcounts)
    assert np.abs(single).max() > 0


# ------------------------------------------------------------------------------------------------------- the C ABI
def test_genevar_checks_without_a_device(built):
    lib = built.lib()
    i64, i32 = ctypes.c_int64, ctypes.c_int32

    def refused(rc, text):
        assert rc == BMX_ERR_ARG and text in lib.bmx_last_error().decode(), (rc, lib.bmx_last_error().decode())

    assert lib.bmx_genevar_check_create(i32(1)) == 0
    refused(lib.bmx_genevar_check_create(i32(0)), "at least one gene")
    refused(lib.bmx_genevar_check_create(i32(65535 * 256 + 1)), "at most")
    chunk = built.dev_get("genevar_chunk")
    assert chunk == 256 and built.dev_get("genevar_gene_tile") >= 256
    assert lib.bmx_genevar_check_block(i64(1000), i64(0), i64(1000)) == 0
    assert lib.bmx_genevar_check_block(i64(1000), i64(0), i64(2 * chunk)) == 0
    assert lib.bmx_genevar_check_block(i64(1000), i64(3 * chunk), i64(1000 - 3 * chunk)) == 0
    refused(lib.bmx_genevar_check_block(i64(1000), i64(0), i64(chunk + 1)), "whole chunks of 256 cells")
    refused(lib.bmx_genevar_check_block(i64(1000), i64(3 * chunk), i64(1000 - 3 * chunk + 1)), "does not fit")
    refused(lib.bmx_genevar_check_block(i64(1000), i64(0), i64(0)), "does not fit")
    refused(lib.bmx_genevar_check_block(i64(0), i64(0), i64(1)), "at least one cell")
    refused(lib.bmx_genevar_check_block(i64(1 << 31), i64(0), i64(256)), "2^31 - 1")

    indptr = np.array([0, 2, 2, 3], dtype=np.int64)
    idx, val = np.array([0, 4, 1], dtype=np.int32), np.array([1.0, 2.0, 3.0])
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    fn = lib.bmx_genevar_check_sparse_block
    assert fn(i64(3), i64(0), i64(3), p(indptr), p(idx), p(val), i64(3)) == 0
    empty = np.zeros(3, dtype=np.int64)
    assert fn(i64(2), i64(0), i64(2), p(empty), None, None, i64(0)) == 0
    refused(fn(i64(3), i64(0), i64(3), None, p(idx), p(val), i64(3)), "'indptr' is missing")
    refused(fn(i64(3), i64(0), i64(3), p(indptr), None, p(val), i64(3)), "'indices' or 'data' is missing")
    refused(fn(i64(3), i64(0), i64(3), p(indptr), p(idx), p(val), i64(2)), "does not end at")
    down = np.array([0, 2, 1, 3], dtype=np.int64)
    refused(fn(i64(3), i64(0), i64(3), p(down), p(idx), p(val), i64(3)), "decreases")
    refused(fn(i64(1000), i64(0), i64(3), p(indptr), p(idx), p(val), i64(3)), "whole chunks")


def _genevar_entry_points():
    header = open(os.path.join(ROOT, "include", "batchelor_mi355x.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    out = []
    for ret, name, params in re.findall(r"\b(int32_t|void)\s+(bmx_genevar_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", header):
        types = [" ".join(p.split()).rsplit(" ", 1)[0].replace(" *", "*") for p in params.split(",")]
        out.append((ret, name, types))
    return out


def test_every_genevar_entry_point_refuses_a_null_handle(built):
    lib = built.lib()
    scalars = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
    entries = _genevar_entry_points()
    assert len(entries) == 15   # 9 of the dense handle (3 of them checks), 6 of the sparse one
    taking = [e for e in entries if re.match(r"^(const )?bmx_genevar(_sparse)?_t\*$", e[2][0])]
    assert sorted(n for r, n, _ in taking if r == "void") == ["bmx_genevar_destroy", "bmx_genevar_sparse_destroy"]
    assert len(taking) == 10 and sum(n.endswith("_stage_ms") for _, n, _ in taking) == 2
    for ret, name, types in taking:
        fn = getattr(lib, name)
        saved = fn.argtypes, fn.restype
        fn.argtypes = [ctypes.c_void_p if t.endswith("*") else scalars[t] for t in types]
        fn.restype = None if ret == "void" else ctypes.c_int32
        try:
            rc = fn(*[None if t.endswith("*") else scalars[t](1) for t in types])
        finally:
            fn.argtypes, fn.restype = saved
        if ret == "void":
            continue
        assert rc == BMX_ERR_ARG, (name, rc)
        want = "null argument" if name.endswith("_stage_ms") else "null handle"
        assert lib.bmx_last_error().decode() == want, (name, lib.bmx_last_error().decode())
    for create in ("bmx_genevar_create", "bmx_genevar_sparse_create"):   # the checks come before the device
        assert getattr(lib, create)(ctypes.c_int32(0), ctypes.c_int32(5), None) == BMX_ERR_ARG
        assert lib.bmx_last_error().decode() == "null output pointer"
        h = ctypes.c_void_p()
        assert getattr(lib, create)(ctypes.c_int32(0), ctypes.c_int32(0), ctypes.byref(h)) == BMX_ERR_ARG
        assert not h


def test_new_symbols_are_exported(built, bx):
    lib = built.lib()
    for _, name, _ in _genevar_entry_points():
        assert hasattr(lib, name), name
    for name in ("modelGeneVar", "combineVar", "getTopHVGs", "GeneVarTable", "batchCorrect", "quickCorrect", "noCorrect",
                 "intersectRows", "FastMnnParam", "ClassicMnnParam", "RescaleParam", "RegressParam", "NoCorrectParam",
                 "QuickCorrectResult", "NoCorrectResult"):
        assert hasattr(bx, name), name
    from batchelor_amd import model_gene_var as mgv
    assert mgv.STAGES == ("upload", "kernels", "run_wall") and mgv.chunk() == mgv.CHUNK
