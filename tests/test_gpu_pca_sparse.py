"""multiBatchPCA and fastMNN on scipy.sparse batches kept sparse on the device (csrc/pca_sparse.hip, DeviceSparsePCA),
against the longdouble machinery of tests/pca_ref.py and tests/pca_genes_ref.py on the dense equivalents
(tests/pca_sparse_ref.py builds the cases; tests/test_cpu_pca_sparse.py holds a float64 restatement of the sparse
algorithm to the same allowances and shows that they reject planted faults).  Every test prints the device's error /
allowance and asserts that it is at most 1."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

import batchelor_amd as bx
from batchelor_amd import _lib
from batchelor_amd.inputs import canonical_csc, csc_blocks
from tests import pca_sparse_ref as ref

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def device_record(name):
    c, B, subset1 = ref.case(name)
    return bx.multiBatchPCA(*B, iters=c.iters, subset_row=subset1, get_all_genes=True, get_variance=True, **c.kwargs())


def test_cases_reach_what_they_are_for():
    seg = bx.sparse_row_segment()
    assert seg == ref.SEG              # (tests/test_cpu_pca_sparse.py asserts the edge cases' patterns with that figure)
    for name in ref.CASES:
        c, B, subset1 = ref.case(name)
        src = np.arange(c.G_all) if subset1 is None else subset1 - 1
        if name not in ref.EDGE:
            assert max(c.sizes) > 2 * seg, (name, seg)             # the full row has at least three segments
        for i, m in enumerate(B):
            if i == c.empty_prefix:                                # nothing in the PCA rows: no segment there at all
                assert m[src].nnz == 0 and m.nnz > 0
                continue
            full = m[int(src[ref.FULL_ROW])].nnz
            assert full == m.shape[1] - (1 if i == ref.EMPTY_CELL[0] else 0)
            assert m[int(src[ref.ZERO_ROW])].nnz == 0
        b, cell = ref.EMPTY_CELL
        assert B[b][:, cell].nnz == 0
    # rows whose length sits on a segment boundary: (rowlen + seg - 1) / seg with rowlen = seg, 2 seg and 2 seg + 1
    for name, want in (("g1025-d60-cos-w-i1", (seg, 2 * seg)), ("g4300-i1", (seg, 2 * seg, 2 * seg + 1)),
                       ("g4300-i2", (seg, 2 * seg, 2 * seg + 1))):
        c, B, subset1 = ref.case(name)
        assert tuple(m[ref.FULL_ROW].nnz for m in B) == want, (name, seg)


@pytest.mark.parametrize("name", ref.FIXED)
def test_fixed_count_identities(name):
    c, B, subset1 = ref.case(name)
    out = device_record(name)
    assert out["path"] == "device-sparse", out["path"]
    assert out["iters_used"] == c.iters
    r = ref.all_ratios(name, out)
    print(f"case {name}: device error / allowance {r}")
    assert all(v <= 1.0 for v in r.values()), r
    assert np.array_equal(out["var_explained"], out["d"] ** 2 / len(B))


@pytest.mark.parametrize("name", ref.CONVERGED)
def test_converged_identities_and_residual(name):
    c, B, subset1 = ref.case(name)
    out = device_record(name)
    assert out["path"] == "device-sparse", out["path"]
    assert out["residual"] <= ref.TOL
    r = ref.all_ratios(name, out, tol=ref.TOL)
    print(f"case {name}: {out['iters_used']} applications, residual {out['residual']:.3g}; error / allowance {r}")
    assert all(v <= 1.0 for v in r.values()), r


@pytest.mark.parametrize("name", ref.SUBSETS)
def test_subset_rows_sit_where_they_belong(name):
    c, B, subset1 = ref.case(name)
    full = device_record(name)
    only = bx.multiBatchPCA(*B, iters=c.iters, subset_row=subset1, **c.kwargs())      # no get_all_genes: the subset's rows
    assert only["path"] == "device-sparse" and only["rotation"].shape == (subset1.size, c.d) and "var_total" not in only
    assert ref.pca_genes_ref.assembly_ok(subset1, full, only)
    same = {"d": np.array_equal(full["d"], only["d"]),
            "pcs": all(np.array_equal(p, q) for p, q in zip(full["pcs"], only["pcs"]))}
    print(f"case {name}: with and without the leftover rows resident, bitwise equal: {same}")
    assert all(same.values()), same


def _direct(name, block_cells=None):
    """The handle driven directly on case `name`, the batches uploaded in blocks of block_cells (None: whole)."""
    c, B, subset1 = ref.case(name)
    w = bx.multi_batch_pca._weight_vector(c.sizes, c.weights)
    mats = [ref.rows_first(m, subset1) for m in B]
    pca = bx.DeviceSparsePCA(mats[0][0].shape[0], mats[0][1])
    try:
        for (m, _), wi in zip(mats, w):
            pca.add_batch(canonical_csc(m)[0], weight=wi, cos_norm=c.cos_norm, block_cells=block_cells)
        out = pca.fit(d=c.d, iters=c.iters)
        out["pcs"] = [pca.project(b) for b in range(len(B))]
    finally:
        pca.close()
    return out


def test_bitwise_repeat_blocks_and_formats():
    name = "g130-d60-cos-w-i2"
    c, B, subset1 = ref.case(name)
    runs = {"whole": _direct(name), "again": _direct(name), "blocks of 37": _direct(name, block_cells=37)}
    front = {"csc": device_record(name),
             "csr": bx.multiBatchPCA(*[m.tocsr() for m in B], iters=c.iters, **c.kwargs()),
             "coo": bx.multiBatchPCA(*[m.tocoo() for m in B], iters=c.iters, **c.kwargs())}
    base = runs["whole"]
    for label, out in list(runs.items()) + list(front.items()):
        same = {k: bool(np.array_equal(base[k], out[k])) for k in ("centers", "rotation", "d")}
        same["pcs"] = all(np.array_equal(p, q) for p, q in zip(base["pcs"], out["pcs"]))
        print(f"case {name}, {label}: bitwise equal to one whole upload {same}")
        assert all(same.values()), (label, same)


def test_bitwise_repeat_and_blocks_across_tiles():
    """Two tiles of the counting sort, columns of two strides, rows of exactly one, two and two-and-a-bit segments: the
    companion is built after the last block, so neither the tile walk nor a result may depend on the blocks."""
    name = "g4300-i2"
    runs = {"whole": _direct(name), "again": _direct(name), "blocks of 37": _direct(name, block_cells=37)}
    front, base = device_record(name), runs["whole"]
    for label, out in list(runs.items()) + [("multiBatchPCA", front)]:
        same = {k: bool(np.array_equal(base[k], out[k])) for k in ("centers", "rotation", "d")}
        same["pcs"] = all(np.array_equal(p, q) for p, q in zip(base["pcs"], out["pcs"]))
        print(f"case {name}, {label}: bitwise equal to one whole upload {same}")
        assert all(same.values()), (label, same)


def test_bad_pattern_is_refused_by_the_fit():
    """A row index equal to n_rows, and a descending pair, handed straight to the handle: the entries are skipped by
    every kernel by construction, and the fit says what is wrong.  In a column of 66 entries or more the pair sits at
    positions 63 / 64 and the high index at the last position (>= 64): the order check looks back across the lane
    stride, and the second 64-entry pass of the column is checked like the first."""
    _refusals("g65-d5-i2", 11, 2, 5)       # column 11: its first two entries
    long_col = int(np.flatnonzero(np.diff(ref.case("g1025-d60-cos-w-i1")[1][0].indptr) >= 66)[0])
    _refusals("g1025-d60-cos-w-i1", long_col, 66, 60)


def _refusals(name, col, col_len, d):
    c, B, subset1 = ref.case(name)
    G = c.G_all
    good = [canonical_csc(m)[0] for m in B]

    def run(bad):
        pca = bx.DeviceSparsePCA(G)
        try:
            for m in [bad] + good[1:]:
                pca.add_batch(m)
            pca.fit(d=d, iters=1)
        finally:
            pca.close()

    k, end = int(good[0].indptr[col]), int(good[0].indptr[col + 1])
    assert end - k >= col_len
    a = k if col_len == 2 else k + 63      # the descending pair: the column's first two entries, or positions 63 / 64
    def stand_in(indices):   # (what add_batch reads of a CSC matrix, without scipy's own checks in the way)
        return SimpleNamespace(ndim=2, shape=good[0].shape, nnz=good[0].nnz, indptr=good[0].indptr, indices=indices,
                               data=good[0].data)

    high = good[0].indices.copy()
    high[end - 1] = G
    assert col_len == 2 or end - 1 - k >= 64
    with pytest.raises(_lib.BatchelorMI355XError, match=r"a row index is outside \[0, number of genes\)"):
        run(stand_in(high))
    desc = good[0].indices.copy()
    desc[a], desc[a + 1] = good[0].indices[a + 1], good[0].indices[a]
    with pytest.raises(_lib.BatchelorMI355XError, match="strictly ascending"):
        run(stand_in(desc))
    run(good[0])                            # and the same calls with the good pattern go through


def test_misuse_of_the_handle():
    c, B, subset1 = ref.case("g65-d5-i2")
    m = canonical_csc(B[0])[0]
    pca = bx.DeviceSparsePCA(65)
    try:
        with pytest.raises(_lib.BatchelorMI355XError, match="bmx_pca_sparse_begin_batch has not been called"):
            pca.add_block(*next(csc_blocks(m, 10)))
        with pytest.raises(_lib.BatchelorMI355XError, match="at least one batch"):
            pca.fit(d=5, iters=1)
        pca.add_batch(m)
        with pytest.raises(_lib.BatchelorMI355XError, match="bmx_pca_sparse_fit has not been run"):
            pca.project(0)
        with pytest.raises(_lib.BatchelorMI355XError, match="rank below the subspace width"):
            pca.fit(d=60, iters=1)          # 65 genes: fewer than the block of 128 that d = 60 needs
    finally:
        pca.close()
    with pytest.raises(ValueError, match="number of rows is not the same"):
        bx.multiBatchPCA(B[0], B[1][:60], d=5)


def _with_an_empty_block(n_rows, n_pca, block_cells, more_cells):
    """A batch of 10 cells whose cells 4-7 hold no entry, uploaded whole or in blocks of block_cells, then (more_cells > 0)
    a second batch; fit with a fixed count, the projections and the rows outside the PCA's."""
    rng = np.random.default_rng(4)
    a = rng.poisson(1.0, (n_rows, 10)).astype(np.float64)
    a[:, 4:8] = 0
    mats = [sp.csc_matrix(a)] + ([sp.csc_matrix(rng.poisson(0.7, (n_rows, more_cells)).astype(np.float64))] if more_cells else [])
    assert np.array_equal(np.diff(mats[0].indptr)[4:8], [0, 0, 0, 0]) and np.all(np.diff(mats[0].indptr)[:4] > 0)
    pca = bx.DeviceSparsePCA(n_rows, n_pca)
    try:
        pca.add_batch(canonical_csc(mats[0])[0], block_cells=block_cells)
        for m in mats[1:]:
            pca.add_batch(canonical_csc(m)[0])
        out = pca.fit(d=5, iters=2)
        return [out["centers"], out["rotation"], out["d"], *pca.genes()] + [pca.project(b) for b in range(len(mats))]
    finally:
        pca.close()


def test_an_upload_block_without_entries_gives_the_bits_of_a_whole_upload():
    """block_cells = 4 cuts the 10 cells into 4 + 4 (no stored entry) + 2.  At 70 rows of which 40 are the PCA's, and 10
    cells, both uploads are taken and the fit refuses either alike: the iteration's block needs 64 PCA rows and more than
    64 cells.  The smallest shape it takes -- 94 rows of which 64 are the PCA's, a second batch of 60 cells -- gives the
    same bits from either upload."""
    for block_cells in (None, 4):
        with pytest.raises(_lib.BatchelorMI355XError, match="rank below the subspace width"):
            _with_an_empty_block(70, 40, block_cells, 0)
    whole, blocked = (_with_an_empty_block(94, 64, block_cells, 60) for block_cells in (None, 4))
    same = [bool(np.array_equal(p, q)) for p, q in zip(whole, blocked)]
    print(f"centers, rotation, d, centers and rotation of the other rows, projections: bitwise equal {same}")
    assert len(whole) == 7 and all(np.all(np.isfinite(p)) for p in whole) and all(same), same


# ------------------------------------------------------------------------------------- fastMNN end to end
def _aligned_rel(got, want, rot_got, rot_want):
    """max |got - want| / max |want| after giving every column of `got` the sign of its rotation column in `want`."""
    sign = np.sign((rot_got * rot_want).sum(axis=0))
    return float(np.abs(got * sign[None, :] - want).max() / np.abs(want).max())


def _check_fastmnn(sparse, dense):
    assert len(sparse.merge_info.pairs) == len(dense.merge_info.pairs)
    for (a, b), (p, q) in zip(sparse.merge_info.pairs, dense.merge_info.pairs):
        assert np.array_equal(a, p) and np.array_equal(b, q)
    assert np.array_equal(sparse.batch, dense.batch)
    rel = _aligned_rel(sparse.corrected, dense.corrected, sparse.rotation, dense.rotation)
    print(f"fastMNN on sparse batches against their toarray(): {sum(p[0].size for p in dense.merge_info.pairs)} pairs equal, "
          f"corrected coordinates differ by {rel:.3g} of their range (bound 1e-5)")
    assert rel <= 1e-5


def test_fastmnn_list_of_sparse_batches():
    B, d = ref.planted_sparse()
    _check_fastmnn(bx.fastMNN(*B, d=d, k=5), bx.fastMNN(*[m.toarray() for m in B], d=d, k=5))


def test_fastmnn_one_sparse_object_with_batch():
    B, d = ref.planted_sparse()
    n = sum(m.shape[1] for m in B)
    batch = np.array(["p", "q"])[(np.arange(n) * 7 % n >= B[0].shape[1]).astype(int)]      # interleaved
    assert (batch == "p").sum() == B[0].shape[1]
    dense = np.empty((B[0].shape[0], n))
    dense[:, batch == "p"], dense[:, batch == "q"] = B[0].toarray(), B[1].toarray()
    x = sp.csr_matrix(dense)
    _check_fastmnn(bx.fastMNN(x, batch=batch, d=d, k=5), bx.fastMNN(x.toarray(), batch=batch, d=d, k=5))
