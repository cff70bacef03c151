"""mnnCorrect() on scipy.sparse batches, on the device: the bits of the dense call over toarray() for every form of the
prepare stage and every edge of the expansion kernel, the CPU restatement as a second anchor, the patterns only the device
sees, and the quickCorrect workflow over sparse counts."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import batchelor_amd as bx
from batchelor_amd import _lib
from batchelor_amd.mnn_correct import BmxMnnParams
from tests import mnn_correct_ref as ref
from tests import model_gene_var_ref as gv_ref
from tests.test_gpu_mnn_correct import CASES, _batches, _compare

pytestmark = pytest.mark.gpu
DENSITY = 0.2
SPARSE_CASES = CASES[:12]   # rows 1-12 of the dense file: all at G = 10


def masked(seed, cells, G, density=DENSITY):
    """_batches of the dense file with every value kept with probability `density`, as CSC."""
    rng = np.random.default_rng(10_000 + seed)
    return [sp.csc_matrix(b * (rng.random(b.shape) < density)) for b in _batches(seed, cells, G)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_same_result(got, want, what=""):
    """Everything mnnCorrect returns, bit for bit."""
    assert got.corrected.shape == want.corrected.shape, what
    assert got.corrected.flags.f_contiguous and got.corrected.dtype == np.float64
    differ = int((bits(got.corrected) != bits(want.corrected)).sum())
    assert differ == 0, (what, differ)
    assert len(got.merge_info.pairs) == len(want.merge_info.pairs)
    for (gl, gr), (wl, wr) in zip(got.merge_info.pairs, want.merge_info.pairs):
        assert np.array_equal(np.asarray(gl), np.asarray(wl)) and np.array_equal(np.asarray(gr), np.asarray(wr)), what
    assert got.merge_info.left == want.merge_info.left and got.merge_info.right == want.merge_info.right, what
    assert np.array_equal(np.asarray(got.batch), np.asarray(want.batch)), what


def both(B, **kw):
    """The sparse call and the dense call over toarray(); asserts that they agree and returns the sparse result."""
    got = bx.mnnCorrect(*B, **kw)
    want = bx.mnnCorrect(*[m.toarray() for m in B], **kw)
    assert_same_result(got, want, str(kw))
    return got


def case_batches(i):
    cells, G, _ = SPARSE_CASES[i]
    return masked(len(cells) * 7 + G, cells, G)


@functools.lru_cache(maxsize=None)
def dense_case(i):
    return bx.mnnCorrect(*[m.toarray() for m in case_batches(i)], **SPARSE_CASES[i][2])


# ------------------------------------------------------------------------------------------ 1. the dense call's bits
def test_the_g10_data_has_empty_and_repeated_cells():
    """What makes the G = 10 cases worth running: columns without an entry (the clamp at l2 = 0) and cells that coincide
    (ties in the search)."""
    first = case_batches(0)[0]
    empty = int((np.diff(first.indptr) == 0).sum())
    cols = first.toarray().T
    repeated = cols.shape[0] - np.unique(cols, axis=0).shape[0]
    print(f"first batch: {empty} of {cols.shape[0]} cells empty, {repeated} repeated")
    assert empty >= 3 and repeated >= 2


@pytest.mark.parametrize("i", range(len(SPARSE_CASES)), ids=[str(c[2]) for c in SPARSE_CASES])
def test_bitwise_against_the_dense_call(i):
    got = bx.mnnCorrect(*case_batches(i), **SPARSE_CASES[i][2])
    assert_same_result(got, dense_case(i), str(SPARSE_CASES[i][2]))


@pytest.mark.parametrize("form", [sp.csr_matrix, sp.coo_array, sp.csc_array], ids=["csr_matrix", "coo_array", "csc_array"])
def test_any_scipy_format(form):
    B = [form(m) for m in case_batches(0)]
    kept = [m.copy() for m in B]
    assert_same_result(bx.mnnCorrect(*B), dense_case(0))
    assert_same_result(bx.mnnCorrect(B), dense_case(0))   # a list of batches
    for m, k in zip(B, kept):
        assert m.format == k.format and (m != k).nnz == 0


@pytest.mark.parametrize("G", [63, 64, 65, 257])
@pytest.mark.parametrize("kw", [dict(), dict(subset_row="unordered", correct_all=True)], ids=["all_genes", "subset_correct_all"])
def test_gene_counts_around_the_wave_and_cells_that_do_not_fill_a_workgroup(G, kw):
    kw = dict(kw)
    if "subset_row" in kw:   # more than 64 positions, unordered, with repeats: the search form's second round of lanes
        rng = np.random.default_rng(G)
        kw["subset_row"] = rng.integers(1, G + 1, size=min(G, 70) + 3)
    both(masked(G, [101, 203], G), **kw)


def edited(G=257, cells=(101, 203)):
    """Density 0.2 with, in the first batch, a cell that holds all G rows, one with exactly 64 entries, one with exactly
    65, a stored 0.0 and a stored -0.0, and the second batch's last three cells empty."""
    rng = np.random.default_rng(99)
    B = _batches(31, list(cells), G)
    keep = [rng.random(b.shape) < DENSITY for b in B]
    keep[0][:, 0] = True
    for cell, count in ((1, 64), (2, 65)):
        keep[0][:, cell] = False
        keep[0][rng.choice(G, count, replace=False), cell] = True
    keep[1][:, -3:] = False
    vals = [b.copy() for b in B]
    keep[0][[4, 9], 5] = True
    vals[0][4, 5], vals[0][9, 5] = 0.0, -0.0
    out = []
    for v, k in zip(vals, keep):
        r, c = np.nonzero(k)
        out.append(sp.coo_matrix((v[r, c], (r, c)), shape=v.shape).tocsc())   # (keeps the stored zeros)
    counts = np.diff(out[0].indptr)
    assert counts[0] == G and counts[1] == 64 and counts[2] == 65 and (np.diff(out[1].indptr)[-3:] == 0).all()
    col = out[0][:, 5]
    stored = dict(zip(col.indices.tolist(), col.data.tolist()))
    assert stored[4] == 0.0 and not np.signbit(stored[4]) and stored[9] == 0.0 and np.signbit(stored[9])
    return out


@pytest.mark.parametrize("kw", [dict(), dict(cos_norm_in=False, cos_norm_out=False, var_adj=False),
                                dict(subset_row=[6, 201, 5, 10, 5, 257, 1], correct_all=True),
                                dict(subset_row=[6, 201, 5, 10, 5, 257, 1], correct_all=True, cos_norm_out=False, var_adj=False)],
                         ids=["default", "raw", "subset_correct_all", "subset_correct_all_raw_out"])
def test_full_cells_64_and_65_entries_empty_tail_and_stored_zeros(kw):
    got = both(edited(), **kw)
    if not kw.get("cos_norm_out", True) and "subset_row" not in kw:
        # the first batch is never corrected: the stored zeros of either sign come back as toarray()'s +0.0
        assert bits(got.corrected[[4, 9], 5]).tolist() == [0, 0]


@pytest.mark.parametrize("correct_all", [False, True])
def test_subset_with_repeats_in_any_order(correct_all):
    B = case_batches(0)
    kw = dict(subset_row=[5, 2, 2, 9], correct_all=correct_all)
    try:
        want = bx.mnnCorrect(*[m.toarray() for m in B], **kw)
    except (ValueError, bx.BatchelorMI355XError) as err:
        print(f"the dense call refuses {kw}: {err}")
        pytest.skip(f"the dense call refuses {kw}")
    got = bx.mnnCorrect(*B, **kw)
    assert_same_result(got, want, str(kw))
    assert got.corrected.shape[0] == (10 if correct_all else 4)


def test_restrict_with_a_cell_named_twice():
    both(case_batches(0), restrict=[np.arange(1, 61), None, np.concatenate([np.arange(1, 301), np.arange(1, 51)])])


def test_merge_tree_on_four_batches():
    i = [c[2] for c in SPARSE_CASES].index(dict(merge_order=[[1, 3], [4, 2]]))
    got = bx.mnnCorrect(*case_batches(i), merge_order=[[1, 3], [4, 2]], names=["a", "b", "c", "d"])
    want = dense_case(i)
    assert np.array_equal(bits(got.corrected), bits(want.corrected))
    assert got.merge_info.left[-1] == ["a", "c"] and got.merge_info.right[-1] == ["d", "b"]


def test_one_object_with_batch_and_shuffled_columns():
    B = case_batches(0)
    x = sp.hstack(B).tocsc()
    lab = np.repeat(np.array(["b", "c", "a"]), [m.shape[1] for m in B])
    perm = np.random.default_rng(3).permutation(x.shape[1])
    x, lab = x[:, perm], lab[perm]
    mask = np.ones(x.shape[1], dtype=bool)
    mask[::7] = False
    for form in (sp.csc_matrix, sp.csr_array):
        for kw in (dict(), dict(restrict=[mask])):
            got = bx.mnnCorrect(form(x), batch=lab, **kw)
            want = bx.mnnCorrect(x.toarray(), batch=lab, **kw)
            assert_same_result(got, want, str(kw))
            assert list(got.batch) == list(lab)


def test_batch_correct_passes_sparse_batches_to_the_classic_param():
    got = bx.batchCorrect(*case_batches(1), PARAM=bx.ClassicMnnParam(cos_norm_in=False))
    assert_same_result(got, dense_case(1))


# --------------------------------------------------------------------------------------------- 2. the restatement
@pytest.mark.parametrize("G,cells,seed", [(65, [101, 203], 87), (500, [1000, 2000, 3000], 521)])
def test_against_the_restatement(G, cells, seed):
    """Anchored to something other than the dense path.  Every cell of these has at least 6 stored entries and no two
    cells coincide (asserted; the seeds are the first that give it), so ties cannot separate the restatement from the
    device."""
    B = masked(seed, cells, G)
    dense = [m.toarray() for m in B]
    assert min(int(np.diff(m.indptr).min()) for m in B) >= 6
    allc = np.hstack(dense).T
    assert np.unique(allc, axis=0).shape[0] == allc.shape[0]
    dev = bx.mnnCorrect(*B)
    cpu = ref.mnn_correct(*dense)
    rel = _compare(dev, cpu, f"G={G}")
    print(f"cells={cells} G={G} density {DENSITY}: max rel {rel:.2e}")


# ------------------------------------------------------------------------------- 3. patterns only the device sees
@pytest.mark.parametrize("indices,message", [
    ([0, 5, 1, 2], "a row index is outside [0, number of genes)"),
    ([0, -1, 1, 2], "a row index is outside [0, number of genes)"),
    ([3, 1, 1, 2], "the row indices of a column should be strictly ascending"),
])
@pytest.mark.parametrize("kw", [dict(), dict(subset=[4, 1], correct_all=1)], ids=["scatter", "search_and_scatter"])
def test_patterns_only_the_device_sees(indices, message, kw):
    """Through the C entry point, past the front end's canonical form: a row equal to G, a row of -1 and rows that descend
    end the call with the pattern error -- such an entry is left out, never an address --, and the next ordinary call
    gives the bits it should."""
    L = _lib.lib()
    G = 5
    indptr = [np.array([0, 2, 3, 4], dtype=np.int64), np.array([0, 1, 3], dtype=np.int64)]
    idx = [np.array(indices, dtype=np.int32), np.array([2, 0, 4], dtype=np.int32)]
    data = [np.ones(4), np.ones(3)]
    ncells = np.array([3, 2], dtype=np.int32)
    tree = np.array([1, 2, 0], dtype=np.int32)
    sub = np.array(kw.get("subset", []), dtype=np.int32)
    p = BmxMnnParams(ctypes.sizeof(BmxMnnParams), 1, float("nan"), 0.1, 1, 1, 1, kw.get("correct_all", 0), 0, 0,
                     sub.ctypes.data if sub.size else None, int(sub.size), tree.ctypes.data, 3)
    ptrs = [(ctypes.c_void_p * 2)(*[a.ctypes.data for a in arrs]) for arrs in (indptr, idx, data)]
    h = ctypes.c_void_p()
    _lib.check(L.bmx_set_device(0))
    rc = L.bmx_mnn_correct_sparse(ctypes.c_int32(2), ctypes.c_int32(G), ptrs[0], ptrs[1], ptrs[2], _lib.i32p(ncells), None,
                                  None, ctypes.byref(p), ctypes.byref(h))
    assert rc == -6 and message in L.bmx_last_error().decode() and not h
    assert_same_result(bx.mnnCorrect(*case_batches(0)), dense_case(0))


# ------------------------------------------------------------------------------------------------ 4. the workflow
def test_quick_correct_sparse_counts_with_the_classic_param():
    counts = gv_ref.quick_counts()
    assert [c.shape[1] for c in counts] == list(gv_ref.QUICK_SIZES)
    hvg = {"n": gv_ref.QUICK_N}
    dense = bx.quickCorrect(*counts, hvg_args=hvg, PARAM=bx.ClassicMnnParam())
    got = bx.quickCorrect(*[sp.csc_matrix(c) for c in counts], hvg_args=hvg, PARAM=bx.ClassicMnnParam())
    assert np.array_equal(got.hvgs, dense.hvgs)
    assert got.corrected.corrected.shape == (gv_ref.QUICK_GENES, sum(gv_ref.QUICK_SIZES))   # correct_all=True by default
    assert_same_result(got.corrected, dense.corrected)
    # multiBatchNorm's sparse log-values straight into mnnCorrect
    normed = bx.multiBatchNorm(*[sp.csr_matrix(c) for c in counts])
    assert all(sp.issparse(m) for m in normed.logcounts)
    both(list(normed.logcounts), subset_row=dense.hvgs)
