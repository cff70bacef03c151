"""mnnDeltaVariance() on scipy.sparse batches, without a GPU: the float64 restatement of the device's sparse algorithm
(tests/delta_variance_sparse_ref.py: chunked pair order, one implicit-zero term per chunk) held to the bounds of
tests/test_cpu_delta_variance.py on every input tests/test_gpu_delta_variance_sparse.py uses; planted faults that leave
those bounds; the front end (formats, the mixture, the dense path's refusals, subset_row on the host); and what the
library answers without a device.

Inputs: the dense tests' batches (values on the 2^-12 grid) with every entry kept with probability `dens` from a seeded
generator, else not stored.  The bounds are the dense ones -- 8 P u total for the variance, 4 P u mean(|x_l| + |x_r|) / 2
for the mean, against the longdouble restatement of tests/delta_variance_ref.py on the densified batches: leaving a term
of zero out of a sum, or adding (n m) m for n terms of m m, adds no rounding beyond what those bounds allow a sum of P
terms.  Shapes are relative to the sparse gene tile Ts and the pair chunk C the kernels use, asked of the library."""
import functools
import zlib

import numpy as np
import pytest
import scipy.sparse as sp

from tests import delta_variance_sparse_ref as sref
from tests.test_cpu_delta_variance import (A, B2, OK, REFUSED, SIZES, Bounds, built, case, cross_pairs,  # noqa: F401
                                           make_batches, one_pass_total)

G_LABELS = ["1", "7", "Ts-1", "Ts", "Ts+1", "2Ts+1"]
P_LABELS = ["0", "1", "2", "3", "C-1", "C", "C+1", "3C+5"]
SHAPE_DENSITY = 0.1
DENSITIES = (0.02, 0.5, 1.0)          # at G = 2Ts+1, P = 3C+5
CPU_DENSITIES = (0.02, 0.1, 0.5)      # the grid of shapes the restatement is held to the bounds on
SPARSIFIED = ["left-run", "same-pair-twice", "only-one-pair-twice", "offset", "three-steps", "three-steps-one-pair"]
COS_CASES = ["subset", "subset-all", "subset-cos", "subset-all-cos", "subset-all-cos:63", "subset-all-cos:64",
             "subset-all-cos:65", "cos-zero-cell-paired", "cos-zero-cell-unpaired"]


@functools.lru_cache(maxsize=None)
def tile_and_chunk():
    """The sparse gene-tile width and the pair-chunk length, asked of the library (no device needed)."""
    from batchelor_amd import delta_variance as dv
    return dv.sparse_gene_tile(), dv.pair_chunk()


def resolve(label):
    Ts, C = tile_and_chunk()
    return int(eval(label.replace("2Ts", "2*Ts").replace("3C", "3*C"), {"Ts": Ts, "C": C}))


# ---------------------------------------------------------------------------------------------- inputs
def from_pattern(x, stored):
    """CSC with exactly the entries `stored` marks (a marked zero is a stored zero)."""
    rows, cols = np.nonzero(stored)
    return sp.csc_matrix((x[rows, cols], (rows, cols)), shape=x.shape)


def sparsify(batches, dens, seed):
    """Every non-zero entry kept with probability dens, else not stored; dens = 1: the full matrix as CSC (a zero is
    never stored here: the cell of the cos-zero-cell cases stores nothing; stored zeros are in the patterns case)."""
    rng = np.random.default_rng(seed)
    return [from_pattern(b, (rng.random(b.shape) < dens) & (b != 0.0)) for b in batches]


class SparseCase:
    def __init__(self, batches, pairs, **kwargs):
        self.batches, self.pairs, self.kwargs = batches, pairs, kwargs     # batches: CSC; pairs: a list of (left, right)
        self.dense = [b.toarray() for b in batches]


def _seed(name, dens):
    return zlib.crc32(f"{name}@{dens}".encode())


def pattern_pairs(left, right):
    """The pairs the patterns sit at: the pair whose left cell is emptied, the one whose right cell is, and two more that
    share no cell with those two."""
    e_l = 0
    e_r = next(i for i in range(len(left)) if left[i] != left[e_l])
    empty = (left[e_l], right[e_r])
    free = [i for i in range(len(left)) if left[i] not in empty and right[i] not in empty]
    return e_l, e_r, free[0], free[1]


def patterns_case():
    """Test 4's patterns, in one input of Ts + 5 genes and C + 1 pairs at density 0.1."""
    Ts, C = tile_and_chunk()
    G = Ts + 5
    full = [b + 1.0 for b in make_batches(G, SIZES, 91)]                   # (no value is 0)
    left, right = cross_pairs(C + 1, SIZES, 92)
    rng = np.random.default_rng(93)
    x = np.concatenate(full, axis=1)
    stored = rng.random(x.shape) < 0.1
    e_l, e_r, edge, zeros = pattern_pairs(left, right)
    stored[:, left[e_l] - 1] = False                                       # an empty column paired on the left ...
    stored[:, right[e_r] - 1] = False                                      # ... and one paired on the right
    stored[3, :] = False                                                   # a gene no cell stores
    stored[5, :] = True                                                    # a gene every cell stores
    stored[5, left[e_l] - 1] = stored[5, right[e_r] - 1] = False           # (but for the two empty columns)
    for c in (left[edge] - 1, right[edge] - 1):                            # rows Ts - 1 and Ts of one column: a tile edge
        stored[Ts - 1:Ts + 1, c] = True
    lz, rz = left[zeros] - 1, right[zeros] - 1                             # stored zeros in both cells of a pair
    x[9, lz] = x[9, rz] = 0.0
    stored[9, lz] = stored[9, rz] = True
    off = np.concatenate([[0], np.cumsum(SIZES)])
    B = [from_pattern(x[:, off[i]:off[i + 1]], stored[:, off[i]:off[i + 1]]) for i in range(len(SIZES))]
    return SparseCase(B, [(left, right)])


@functools.lru_cache(maxsize=None)
def sparse_case(name, dens):
    """The inputs of the GPU tests by name and density, built once."""
    if name == "patterns":
        return patterns_case()
    if name.startswith("shape:"):
        _, g, p = name.split(":")
        G, P = resolve(g), resolve(p)
        return SparseCase(sparsify(make_batches(G, SIZES, 1000 + G), dens, _seed(name, dens)), [cross_pairs(P, SIZES, 2000 + P)])
    c = case(name)                                                         # the dense tests' case, sparsified
    return SparseCase(sparsify(c.batches, dens, _seed(name, dens)), c.pairs, **c.kwargs)


@functools.lru_cache(maxsize=None)
def sparse_bounds(name, dens):
    c = sparse_case(name, dens)
    return Bounds(c.dense, c.pairs, **c.kwargs)


SHAPE_CASES = [(f"shape:{g}:{p}", SHAPE_DENSITY) for g in G_LABELS for p in P_LABELS]
DENSITY_CASES = [("shape:2Ts+1:3C+5", d) for d in DENSITIES]
PATTERN_CASES = [("patterns", 0.1)] + [(n, 1.0 if n == "offset" else 0.1) for n in SPARSIFIED]
COS_NORM_CASES = [(n, 0.1) for n in COS_CASES]
GPU_CASES = SHAPE_CASES + DENSITY_CASES + PATTERN_CASES + COS_NORM_CASES
# the grid the issue names for the restatement: three densities, cos_norm only from C pairs on, as the dense tests do
CPU_GRID = [(f"shape:{g}:{p}", d, cos) for d in CPU_DENSITIES for g in G_LABELS for p in P_LABELS[2:]
            for cos in ((False, True) if p in ("C", "C+1", "3C+5") else (False,))]


def restatement(c, fault=None, **more):
    _, C = tile_and_chunk()
    return sref.sparse_delta_variance(c.batches, c.pairs, C, fault=fault, **{**c.kwargs, **more})


def case_id(v):
    return v if isinstance(v, str) else str(v)


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name,dens", GPU_CASES, ids=case_id)
def test_float64_sparse_restatement_stays_inside_the_bounds_on_the_gpu_inputs(built, name, dens):
    c, b = sparse_case(name, dens), sparse_bounds(name, dens)
    for i, t in enumerate(restatement(c)):
        em, et = b.worst(i, t["mean"], t["total"])
        print(f"{name} dens {dens} step {i} P={b.steps[i]['P']}: sparse restatement error / allowance: mean {em:.3g}, total {et:.3g}")
        assert em <= 1.0 and et <= 1.0
    for s in b.steps:
        assert s["P"] <= 10_000


@pytest.mark.parametrize("name,dens,cos", CPU_GRID, ids=case_id)
def test_float64_sparse_restatement_stays_inside_the_bounds_on_the_grid(built, name, dens, cos):
    c = sparse_case(name, dens)
    b = Bounds(c.dense, c.pairs, cos_norm=cos)
    t = restatement(c, cos_norm=cos)[0]
    em, et = b.worst(0, t["mean"], t["total"])
    print(f"{name} dens {dens} cos_norm {cos}: sparse restatement error / allowance: mean {em:.3g}, total {et:.3g}")
    assert em <= 1.0 and et <= 1.0


def test_restatement_matches_the_dense_one_where_everything_is_stored(built):
    """At density 1 nothing is implicit: the sparse order of operations is the dense restatement's up to the summation
    order, which the bounds cover; the mean of one chunk is the dense float64 mean bit for bit."""
    from tests import delta_variance_ref as ref
    _, C = tile_and_chunk()
    B = make_batches(9, SIZES, 5)
    pairs = [cross_pairs(C - 3, SIZES, 6)]
    got = sref.sparse_delta_variance([sp.csc_matrix(b) for b in B], pairs, C)[0]
    x = np.concatenate(B, axis=1)
    l, r = pairs[0]
    sl, sr = np.zeros(9), np.zeros(9)
    for p in range(len(l)):
        sl += x[:, l[p] - 1]
        sr += x[:, r[p] - 1]
    assert np.array_equal(got["mean"], (sl / len(l) + sr / len(l)) / 2)
    want = ref.mnn_delta_variance(B, pairs)["per_step"][0]
    np.testing.assert_allclose(got["total"], want["total"], rtol=8 * len(l) * 2.0 ** -53 * 2)


@pytest.mark.parametrize("fault", ["no-zero-term", "squared-separately"])
def test_a_planted_fault_leaves_the_bounds(built, fault):
    name, dens = "shape:2Ts+1:3C+5", 0.1
    c, b = sparse_case(name, dens), sparse_bounds(name, dens)
    t = restatement(c, fault=fault)[0]
    em, et = b.worst(0, t["mean"], t["total"])
    print(f"{fault}: error / allowance: mean {em:.3g}, total {et:.3g}")
    assert em <= 1.0 and et > 1.0


def test_the_sparsified_offset_case_catches_a_one_pass_variance(built):
    c, b = sparse_case("offset", 1.0), sparse_bounds("offset", 1.0)
    assert all(m.nnz == np.count_nonzero(d) >= 0.99 * d.size for m, d in zip(c.batches, c.dense))   # dense-valued, as CSC
    x = np.concatenate(c.dense, axis=1)
    left, right = c.pairs[0]
    em, et = b.worst(0, b.steps[0]["mean"].astype(np.float64), one_pass_total(x, left, right))
    print(f"offset case as CSC: one-pass variance error / allowance {et:.3g}")
    assert et > 1.0
    t = restatement(c)[0]
    assert max(b.worst(0, t["mean"], t["total"])) <= 1.0


def test_the_patterns_are_what_test_4_names(built):
    Ts, C = tile_and_chunk()
    c = sparse_case("patterns", 0.1)
    x = sp.hstack(c.batches).tocsc()
    left, right = c.pairs[0]
    e_l, e_r, edge, zeros = pattern_pairs(left, right)
    nnz = np.diff(x.indptr)
    assert nnz[left[e_l] - 1] == 0 and nnz[right[e_r] - 1] == 0
    rows = x.tocsr()
    assert rows[3].nnz == 0 and rows[5].nnz == x.shape[1] - 2
    for col in (left[edge] - 1, right[edge] - 1):
        assert {Ts - 1, Ts} <= set(x[:, col].indices.tolist())
    for col in (left[zeros] - 1, right[zeros] - 1):
        k = x.indptr[col] + np.flatnonzero(x.indices[x.indptr[col]:x.indptr[col + 1]] == 9)
        assert k.size == 1 and x.data[k[0]] == 0.0                         # a stored zero
    t = restatement(c)[0]
    assert t["mean"][3] == 0.0 and t["total"][3] == 0.0                    # exactly


# ---------------------------------------------------------------------------------------------- the front end
def test_every_format_reaches_the_same_canonical_csc(built):
    from batchelor_amd import delta_variance as dv
    c = sparse_case("shape:7:3", SHAPE_DENSITY)
    want = dv.csc_batches(c.batches)
    forms = [[sp.csr_matrix(m) for m in c.batches], [sp.coo_matrix(m) for m in c.batches], [sp.csc_array(m) for m in c.batches],
             [sp.csr_array(m) for m in c.batches]]
    coo = sp.coo_matrix(c.batches[0])                                      # unsorted, with a duplicate that must be summed
    order = np.random.default_rng(1).permutation(coo.nnz)
    dup = sp.coo_matrix((np.concatenate([coo.data[order], coo.data[:1]]),
                         (np.concatenate([coo.row[order], coo.row[:1]]), np.concatenate([coo.col[order], coo.col[:1]]))),
                        shape=coo.shape)
    for mats in forms:
        got = dv.csc_batches(mats)
        for g, w in zip(got, want):
            assert g.format == "csc" and g.has_canonical_format and g.data.dtype == np.float64 and g.indices.dtype == np.int32
            assert np.array_equal(g.indptr, w.indptr) and np.array_equal(g.indices, w.indices) and np.array_equal(g.data, w.data)
    g = dv.csc_batches([dup])[0]
    twice = want[0].toarray()
    twice[coo.row[0], coo.col[0]] *= 2
    assert g.has_canonical_format and np.array_equal(g.indices, want[0].indices) and np.array_equal(g.toarray(), twice)
    zero = sp.csc_matrix((np.array([0.0, 2.0]), np.array([1, 3]), np.array([0, 2])), shape=(5, 1))
    assert dv.csc_batches([zero])[0].nnz == 2                              # stored zeros stay


def test_a_shuffled_subset_row_takes_the_rows_the_dense_path_takes(built):
    from batchelor_amd import delta_variance as dv
    from batchelor_amd.linear_correct import _rows
    c = sparse_case("shape:Ts+1:3", SHAPE_DENSITY)
    G = c.dense[0].shape[0]
    sub = np.random.default_rng(7).permutation(G)[:G // 2] + 1
    plan = dv.plan_genes(sub, False, G)
    got = dv.csc_batches(c.batches, plan.rows)
    want = _rows(c.dense, plan.rows)
    for g, w in zip(got, want):
        assert g.has_canonical_format and g.shape == w.shape and np.array_equal(g.toarray(), w)
    assert dv.csc_batches(c.batches, dv.plan_genes(sub, True, G).rows)[0].shape[0] == G    # compute_all: every gene


def test_a_mixture_is_refused(built):
    import batchelor_amd as bx
    for mix in ((sp.csc_matrix(A), B2), (A, sp.csr_matrix(B2))):
        with pytest.raises(TypeError, match="all sparse or all dense, not a mixture"):
            bx.mnnDeltaVariance(*mix, pairs=OK)


@pytest.mark.parametrize("args,kwargs,msg", REFUSED, ids=[str(i) for i in range(len(REFUSED))])
@pytest.mark.parametrize("form", [sp.csc_matrix, sp.csr_array])
def test_sparse_batches_are_refused_as_dense_ones_before_a_device_is_asked_for(built, form, args, kwargs, msg):
    from tests.test_cpu_inputs import _refused
    _refused("mnnDeltaVariance", tuple(form(a) for a in args), kwargs, msg)


def test_the_linear_corrections_still_refuse_sparse_batches(built):
    import batchelor_amd as bx
    for fn in (bx.rescaleBatches, bx.regressBatches):
        with pytest.raises(TypeError, match="sparse"):
            fn(sp.csc_matrix(A), sp.csc_matrix(B2))


# ---------------------------------------------------------------------------------------------- the library
def test_the_library_answers_without_a_device(built):
    import ctypes
    import os
    L = built.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "batchelor_mi355x.h")).read()
    for name in ("create", "destroy", "begin_batch", "add_block", "run", "stage_ms"):
        assert hasattr(L, f"bmx_delta_sparse_{name}"), name
        assert f"bmx_delta_sparse_{name}(" in header, name
    Ts, C = tile_and_chunk()
    assert Ts >= 64 and C >= 4
    h = ctypes.c_void_p()
    assert L.bmx_delta_sparse_create(ctypes.c_int32(0), ctypes.c_int32(0), ctypes.byref(h)) != 0
    assert b"at least one gene" in L.bmx_last_error()
    i64, f64 = ctypes.c_int64, ctypes.c_double
    ip = (i64 * 2)(0, 0)
    out = (f64 * 5)()
    calls = {"begin_batch": (None, i64(3), i64(0)),
             "add_block": (None, i64(1), ip, None, None, i64(0)),
             "run": (None, ctypes.c_int32(0), None, ctypes.c_int32(0), ctypes.c_int32(0), None, None, None, None, None)}
    for name, args in calls.items():
        assert getattr(L, f"bmx_delta_sparse_{name}")(*args) != 0 and b"null handle" in L.bmx_last_error(), name
    assert L.bmx_delta_sparse_stage_ms(None, out) != 0 and b"null" in L.bmx_last_error()
    L.bmx_delta_sparse_destroy.argtypes = [ctypes.c_void_p]
    L.bmx_delta_sparse_destroy.restype = None
    L.bmx_delta_sparse_destroy(None)                                       # (delete of a null handle: nothing happens)
