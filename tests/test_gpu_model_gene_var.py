"""The gene-variance handles (csrc/gene_var.hip), modelGeneVar and quickCorrect on the device, at the smallest shapes at
which the kernels can go wrong: against the long-double restatement within the allowances of tests/model_gene_var_ref.py,
bit for bit across runs, block widths and batch positions, the sparse handle against the dense one, and the device flags."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import batchelor_amd as bx
from batchelor_amd import BatchelorMI355XError
from batchelor_amd import model_gene_var as mgv
from tests import model_gene_var_ref as ref
from tests import pca_sparse_ref

pytestmark = pytest.mark.gpu

CELLS = (2, 3, 4, 5, 255, 256, 257, 513)   # the edges of the walk over a chunk of 256 cells, four at a time


def gene_counts():
    # odd counts take the scalar form, even ones two genes a lane; 257 and 258 put a single lane into a second tile
    return (1, 2, 63, 64, 65, 255, 256, 257, 258, mgv.gene_tile() + 1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def stats(mats, block_bytes=None):
    mean, total, _ = mgv.device_statistics(list(mats), 0, block_bytes)
    return mean, total


def check_against_restatement(x, mean, total, what):
    want_mean, want_total = ref.mean_var(x)
    mean_allow, total_allow = ref.allowances(x)
    em = np.abs(mean.astype(ref.LD) - want_mean).astype(np.float64)
    et = np.abs(total.astype(ref.LD) - want_total).astype(np.float64)
    tiny = np.finfo(np.float64).tiny
    rm, rt = np.max(em / np.maximum(mean_allow, tiny)), np.max(et / np.maximum(total_allow, tiny))
    print(f"{what}: mean error up to {rm:.3g} of its allowance, total error up to {rt:.3g} of its allowance")
    assert (em <= mean_allow).all() and (et <= total_allow).all()


# ----------------------------------------------------------------------------------------------- dense
@pytest.mark.parametrize("n", CELLS)
def test_dense_against_the_restatement(n):
    for G in gene_counts():
        x = ref.gaussian(G, n, seed=G + n, offset=1.0)
        mean, total = stats([x])
        assert mean.shape == (G, 1) and total.shape == (G, 1)
        check_against_restatement(x, mean[:, 0], total[:, 0], f"{G} genes x {n} cells")


def test_one_cell_has_no_variance():
    x = ref.gaussian(5, 1, seed=1)
    mean, total = stats([x, ref.gaussian(5, 3, seed=2)])
    assert same_bits(mean[:, 0], x[:, 0]) and np.isnan(total[:, 0]).all() and np.isfinite(total[:, 1]).all()


@pytest.mark.parametrize("offset,scale", [(10.0, 1e-3), (1e6, 1.0)])
def test_values_far_from_zero(offset, scale):
    for G in (64, 65):
        x = ref.gaussian(G, 513, seed=3, offset=offset, scale=scale)
        mean, total = stats([x])
        check_against_restatement(x, mean[:, 0], total[:, 0], f"{offset:g} + {scale:g} N(0, 1), {G} genes")


def test_the_same_bits_every_time():
    G = 65
    a, b, c = ref.gaussian(G, 300, 11), ref.gaussian(G, 1100, 12, offset=3.0), ref.gaussian(G, 257, 13)
    mean, total = stats([a, b, c])
    again = stats([a, b, c])
    assert same_bits(mean, again[0]) and same_bits(total, again[1])
    # three or more blocks of batch b: 256 cells each
    blocked = stats([a, b, c], block_bytes=256 * 8 * G)
    assert same_bits(mean, blocked[0]) and same_bits(total, blocked[1])
    h = mgv._GeneVarHandle(G, 0)
    try:
        h.add_batch(b, block_bytes=512 * 8 * G)   # 512, 512, 76
        wide = h.run()
    finally:
        h.close()
    alone = stats([b])
    for got in (alone, wide):
        assert same_bits(got[0][:, 0], mean[:, 1]) and same_bits(got[1][:, 0], total[:, 1])
    even = stats([ref.gaussian(64, 1100, 12)])
    assert same_bits(even[0], stats([ref.gaussian(64, 1100, 12)], block_bytes=256 * 8 * 64)[0])


# ----------------------------------------------------------------------------------------------- CSC
def sparse_shapes():
    gt = mgv.gene_tile()
    return ((5, 2), (65, 257), (gt + 1, 255), (gt + 70, 513))


@functools.lru_cache(maxsize=None)
def sparse_inputs(G, n, empty_cell=False):
    x, stored = ref.sparse_case(G, n, seed=G + n, empty_cell=empty_cell)
    return x, ref.to_csc(x, stored)


@pytest.mark.parametrize("G,n", sparse_shapes())
def test_csc_against_the_dense_handle_and_the_restatement(G, n):
    """Two batches: one with a gene stored in every cell, one with a cell that has no entry; both with an empty gene and
    stored zeros."""
    (x, c), (y, e) = sparse_inputs(G, n), sparse_inputs(G, n, True)
    assert c.nnz > np.count_nonzero(x) and c[[0]].nnz == 0 and c[[G - 1]].nnz == n and c[G - 1, n - 1] == 0
    assert e[:, [1]].nnz == 0 and e[[0]].nnz == 0 and (e.nnz > np.count_nonzero(y) or G * n < 100)
    if G > mgv.gene_tile():   # a cell's entries on both sides of a gene-tile edge
        rows = c[:, [0]].indices
        assert rows.min() < mgv.gene_tile() <= rows.max()
    smean, stotal = stats([c, e])
    dmean, dtotal = stats([x, y])
    assert np.array_equal(smean, dmean)                                   # (+0 == -0)
    for b, m in enumerate((x, y)):
        _, total_allow = ref.allowances(m)
        assert (np.abs(stotal[:, b] - dtotal[:, b]) <= total_allow).all()
        check_against_restatement(m, smean[:, b], stotal[:, b], f"CSC {G} genes x {n} cells, batch {b}")
        check_against_restatement(m, dmean[:, b], dtotal[:, b], "its dense form")


def test_csc_blocks_and_an_empty_batch():
    G = mgv.gene_tile() + 70
    _, c = sparse_inputs(G, 513)
    _, c2 = sparse_inputs(G, 255, True)
    empty = sp.csc_matrix((G, 300), dtype=np.float64)
    whole = stats([c2, empty, c])
    assert (whole[0][:, 1] == 0).all() and (whole[1][:, 1] == 0).all()
    per_cell = 12 * c.nnz // 513
    blocked = stats([c2, empty, c], block_bytes=256 * per_cell)            # 256 + 256 + 1 cells
    assert same_bits(whole[0], blocked[0]) and same_bits(whole[1], blocked[1])
    alone = stats([c])
    assert same_bits(alone[0][:, 0], whole[0][:, 2]) and same_bits(alone[1][:, 0], whole[1][:, 2])


# ----------------------------------------------------------------------------------------------- flags
def test_data_errors_come_back_as_errors():
    """What only the data can show: reported by run, and the next handle works.  All of it goes through add_block, whose
    host checks have passed the block's indptr; the kernels skip a bad entry and never use it as an address."""
    G, n = 40, 300
    x, c = sparse_inputs(65, 257)
    good = stats([c])

    bad = ref.gaussian(G, n, 5)
    bad[7, 280] = np.nan
    with pytest.raises(BatchelorMI355XError, match="values should be finite"):
        stats([bad])
    bad[7, 280] = np.inf
    with pytest.raises(BatchelorMI355XError, match="values should be finite"):
        stats([bad])

    def broken(change):
        k = c.copy()
        change(k)
        return k

    def nan_value(k):
        k.data[5] = np.nan

    def row_at_G(k):
        assert k.indptr[3] > k.indptr[2]
        k.indices[k.indptr[3] - 1] = 65        # the last entry of cell 2: still ascending, outside [0, G)

    def descending(k):
        a = k.indptr[4]
        assert k.indptr[5] - a >= 2
        k.indices[a], k.indices[a + 1] = k.indices[a + 1], k.indices[a]

    for change, text in ((nan_value, "values should be finite"), (row_at_G, "a row index is outside"),
                         (descending, "strictly ascending")):
        h = mgv._SparseGeneVarHandle(65, 0)
        try:
            h._upload_csc(broken(change), 256)
            with pytest.raises(BatchelorMI355XError, match=text) as err:
                h.run()
            assert err.value.code == -6
        finally:
            h.close()
        after = stats([c])
        assert same_bits(after[0], good[0]) and same_bits(after[1], good[1])


# ----------------------------------------------------------------------------------------------- modelGeneVar
def test_model_gene_var_blocks_and_subset():
    G, n = 70, 700
    x = ref.gaussian(G, n, 21, offset=2.0)
    block = np.array(["b", "a", "c"])[np.arange(n) % 3].astype(object)
    block[5] = "lonely"                                                    # a level of one cell
    fit = lambda mean, total: (lambda m: 0.5 * m)  # noqa: E731
    got = bx.modelGeneVar(x, block=block, trend_fit=fit)
    levels = sorted(set(block.tolist()))
    cells = [int((block == lev).sum()) for lev in levels]
    assert levels == ["a", "b", "c", "lonely"] and cells == [233, 234, 232, 1]
    assert [t.n_cells for t in got.per_block] == cells
    by_hand = bx.combineVar(*[bx.modelGeneVar(x[:, block == lev], trend_fit=fit) for lev in ("a", "b", "c")])
    for f in ("mean", "total", "tech", "bio"):
        assert same_bits(getattr(got, f), getattr(by_hand, f)), f
    assert np.isnan(got.per_block[3].total).all() and got.n_cells == 699
    want = ref.combine_var([ref.mean_var(x[:, block == lev])[1] for lev in levels], cells).astype(np.float64)
    # (the average of the levels' allowances, and four roundings of the average itself)
    allow = np.mean([ref.allowances(x[:, block == lev])[1] for lev in ("a", "b", "c")], axis=0) + 4 * ref.U * want
    assert (np.abs(got.total - want) <= allow).all()
    weighted = bx.modelGeneVar(x, block=np.arange(n) < 100, equiweight=False)
    halves = (x[:, 100:], x[:, :100])                                      # the levels sorted: False, True
    w = ref.combine_var([ref.mean_var(h)[0] for h in halves], [600, 100], equiweight=False).astype(np.float64)
    allow = (600 * ref.allowances(halves[0])[0] + 100 * ref.allowances(halves[1])[0]) / 700 + 6 * ref.U * np.abs(x).max()
    assert (np.abs(weighted.mean - w) <= allow).all()
    assert not np.array_equal(weighted.mean, bx.modelGeneVar(x, block=np.arange(n) < 100).mean)

    rows = np.array([70, 3, 3, 41])
    sub = bx.modelGeneVar(x, subset_row=rows)
    sliced = bx.modelGeneVar(x[rows - 1])
    assert same_bits(sub.mean, sliced.mean) and same_bits(sub.total, sliced.total) and sub.gene_index.tolist() == rows.tolist()
    assert bx.getTopHVGs(sub, n=1).tolist() == [int(rows[np.argmax(sub.total)])]
    sparse = bx.modelGeneVar(sp.csr_matrix(x), block=block, subset_row=rows)
    assert np.array_equal(sparse.mean, bx.modelGeneVar(x, block=block, subset_row=rows).mean)
    assert set(got.stats["stage_ms"]) == set(mgv.STAGES)


# ----------------------------------------------------------------------------------------------- quickCorrect
HVG = {"n": ref.QUICK_N}
FAST = {"d": 10, "k": 10}


@functools.lru_cache(maxsize=None)
def quick_dense():
    return bx.quickCorrect(*ref.quick_counts(), hvg_args=HVG, PARAM=bx.FastMnnParam(**FAST))


def test_quick_correct_is_the_manual_chain():
    counts = ref.quick_counts()
    out = quick_dense()
    normed = bx.multiBatchNorm(*counts)
    want, _, gap, allow = ref.quick_choice(normed.logcounts)
    assert gap > 1e6 * allow
    assert sorted(out.hvgs.tolist()) == sorted(want.tolist()) and out.hvgs.size == ref.QUICK_N
    dec = bx.combineVar(*[bx.modelGeneVar(m) for m in normed.logcounts])
    hvgs = bx.getTopHVGs(dec, n=ref.QUICK_N)
    assert np.array_equal(out.hvgs, hvgs) and same_bits(out.dec.total, dec.total) and out.universe is None
    manual = bx.fastMNN(*normed.logcounts, subset_row=hvgs, correct_all=True, **FAST)
    assert same_bits(out.corrected.corrected, manual.corrected) and same_bits(out.corrected.rotation, manual.rotation)
    assert out.corrected.rotation.shape == (ref.QUICK_GENES, FAST["d"])
    # the order within the chosen set: the restatement's, wherever its values are further apart than the allowance
    comb = ref.quick_choice(normed.logcounts)[1]
    picked = comb[want - 1]
    clear = np.flatnonzero(np.abs(np.diff(picked)) > 2 * allow)
    assert clear.size > ref.QUICK_N // 2 and all(out.hvgs[i] == want[i] for i in clear if i - 1 in clear)


def test_quick_correct_one_object_with_batch():
    counts = ref.quick_counts()
    n = sum(ref.QUICK_SIZES)
    batch = np.array(["p", "q"])[(np.arange(n) * 9 % n >= ref.QUICK_SIZES[0]).astype(int)]    # interleaved
    assert (batch == "p").sum() == ref.QUICK_SIZES[0]
    x = np.empty((ref.QUICK_GENES, n), order="F")
    x[:, batch == "p"], x[:, batch == "q"] = counts
    out = bx.quickCorrect(x, batch=batch, hvg_args=HVG, PARAM=bx.FastMnnParam(**FAST))
    normed = bx.multiBatchNorm(x, batch=batch)
    dec = bx.modelGeneVar(normed.logcounts, block=batch)
    hvgs = bx.getTopHVGs(dec, n=ref.QUICK_N)
    manual = bx.fastMNN(normed.logcounts, batch=batch, subset_row=hvgs, correct_all=True, **FAST)
    assert np.array_equal(out.hvgs, hvgs) and same_bits(out.corrected.corrected, manual.corrected)
    assert sorted(out.hvgs.tolist()) == sorted(quick_dense().hvgs.tolist())   # the batches are the same cells
    assert np.array_equal(out.corrected.batch, manual.batch)


def test_quick_correct_sparse_counts():
    counts = ref.quick_counts()
    dense = quick_dense()
    out = bx.quickCorrect(*[sp.csc_matrix(c) for c in counts], hvg_args=HVG, PARAM=bx.FastMnnParam(**FAST))
    assert sorted(out.hvgs.tolist()) == sorted(dense.hvgs.tolist())
    s, d = out.corrected, dense.corrected
    sign = np.sign((s.rotation * d.rotation).sum(axis=0))
    rel = float(np.abs(s.corrected * sign[None, :] - d.corrected).max() / np.abs(d.corrected).max())
    print(f"quickCorrect on CSC counts against dense counts: corrected coordinates differ by {rel:.3g} of their range "
          f"(bound {pca_sparse_ref.TOL:g})")
    assert rel <= pca_sparse_ref.TOL
    # pseudo_count != 1: multiBatchNorm returns dense values and the dense path is taken
    other = bx.quickCorrect(*[sp.csc_matrix(c) for c in counts], hvg_args=HVG, PARAM=bx.NoCorrectParam(),
                            multi_norm_args={"norm_args": {"pseudo_count": 2}})
    assert isinstance(other.corrected.corrected, np.ndarray)


def test_quick_correct_other_params():
    counts = ref.quick_counts()
    dense = quick_dense()
    normed = bx.multiBatchNorm(*counts)
    res = bx.quickCorrect(*counts, hvg_args=HVG, PARAM=bx.RescaleParam(), correct_all=False)
    assert np.array_equal(res.hvgs, dense.hvgs)
    want = bx.rescaleBatches(*normed.logcounts, subset_row=dense.hvgs)
    assert res.corrected.corrected.shape == (ref.QUICK_N, sum(ref.QUICK_SIZES))
    assert same_bits(res.corrected.corrected, want.corrected)
    no = bx.quickCorrect(*counts, hvg_args=HVG, PARAM=bx.NoCorrectParam(), names=["first", "second"])
    assert no.corrected.corrected.shape == (ref.QUICK_GENES, sum(ref.QUICK_SIZES))   # correct_all=True by default
    assert same_bits(no.corrected.corrected, np.hstack(normed.logcounts))
    assert no.corrected.batch.tolist() == ["first"] * ref.QUICK_SIZES[0] + ["second"] * ref.QUICK_SIZES[1]
    pre = bx.quickCorrect(*counts, hvg_args=HVG, PARAM=bx.NoCorrectParam(), precomputed=dense.dec.per_block)
    assert np.array_equal(pre.hvgs, dense.hvgs)
    with pytest.raises(TypeError, match="sparse"):
        bx.quickCorrect(*[sp.csc_matrix(c) for c in counts], hvg_args=HVG, PARAM=bx.RescaleParam())
