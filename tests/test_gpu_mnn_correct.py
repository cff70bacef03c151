"""mnnCorrect() on the device against the CPU restatement (tests/mnn_correct_ref.py), and the gene-space kernels behind it
(wide averaging, the literal wide adjust_shift_variance, findMutualNN on 2 000 columns) against the oracle."""
import ctypes

import numpy as np
import pytest

import batchelor_amd as bx
from batchelor_amd import _lib
from oracle import fastmnn_oracle as orc
from tests import mnn_correct_ref as ref
from tests.test_cpu_mnn_correct import RESTRICT_ARGS, check_restriction

pytestmark = pytest.mark.gpu
REL = 1e-5


def _batches(seed, ncells, G, shift=1.0):
    rng = np.random.default_rng(seed)
    base = rng.normal(size=(G, 4))
    out = []
    for i, n in enumerate(ncells):
        lat = rng.normal(size=(4, n))
        out.append(np.abs(base @ lat + rng.normal(scale=0.3, size=(G, n)) + shift * i * rng.normal(size=(G, 1))))
    return out


def _compare(dev, cpu, what=""):
    assert len(dev.merge_info.pairs) == len(cpu["pairs"])
    for (dl, dr), (cl, cr) in zip(dev.merge_info.pairs, cpu["pairs"]):
        assert np.array_equal(np.asarray(dl), np.asarray(cl)) and np.array_equal(np.asarray(dr), np.asarray(cr)), what
    assert dev.merge_info.left == cpu["left"] and dev.merge_info.right == cpu["right"]
    assert np.array_equal(np.asarray(dev.batch), np.asarray(cpu["batch"]))
    c = np.asarray(cpu["corrected"])
    assert dev.corrected.shape == c.shape
    rel = np.abs(dev.corrected - c).max() / np.abs(c).max()
    assert rel < REL, (what, rel)
    return rel


CASES = [
    # (cells, genes, kwargs)
    ([100, 200, 300], 10, dict()),
    ([100, 200, 300], 10, dict(cos_norm_in=False)),
    ([100, 200, 300], 10, dict(cos_norm_out=False, var_adj=False)),
    ([100, 200, 300], 10, dict(cos_norm_in=False, cos_norm_out=False, var_adj=False)),
    ([100, 200, 300], 10, dict(subset_row=[1, 3, 5, 7, 9, 10])),
    ([100, 200, 300], 10, dict(subset_row=[2, 4, 6, 8, 9], correct_all=True)),
    ([100, 200, 300], 10, dict(subset_row=[2, 4, 6, 8, 9], correct_all=True, cos_norm_out=False, var_adj=False)),
    ([100, 200, 300], 10, dict(merge_order=[3, 1, 2])),
    ([100, 200, 300], 10, dict(prop_k=0.1)),
    ([100, 200, 300], 10, dict(k=1)),
    ([150, 120, 130, 110], 10, dict(merge_order=[[1, 3], [4, 2]])),
    ([100, 200, 300], 10, dict(subset_row=[1, 2, 3, 4, 5, 6], cos_norm_in=False)),
    ([1000, 2000, 3000], 500, dict()),
    ([3000, 1000, 2000], 500, dict(var_adj=False, merge_order=[[1, 3], 2])),
    ([1500, 2500, 1000], 500, dict(subset_row=list(range(1, 301)), correct_all=True)),
]


@pytest.mark.parametrize("cells,G,kw", CASES)
def test_mnn_correct_matches_restatement(cells, G, kw):
    B = _batches(len(cells) * 7 + G, cells, G)
    dev = bx.mnnCorrect(*B, **kw)
    cpu = ref.mnn_correct(*B, **kw)
    rel = _compare(dev, cpu, str(kw))
    print(f"cells={cells} G={G} {kw}: max rel {rel:.2e}")


def test_mnn_correct_2x3000x2000_var_adj_sampled():
    """2 batches x 3 000 cells x 2 000 genes with var.adj: search, averaging and smoothing in full, the restatement's
    adjust_shift_variance on a sample of the right batch's cells (its loop is per cell; all 3 000 would take minutes);
    pairs bitwise, the left batch and the sampled right cells to 1e-5."""
    B = _batches(2 * 7 + 2000, [3000, 3000], 2000)
    cells = np.sort(np.random.default_rng(4).choice(3000, 48, replace=False))
    dev = bx.mnnCorrect(*B)
    cpu = ref.mnn_correct(*B, asv_cells=cells)
    for (dl, dr), (cl, cr) in zip(dev.merge_info.pairs, cpu["pairs"]):
        assert np.array_equal(dl, cl) and np.array_equal(dr, cr)
    c = cpu["corrected"]
    cols = np.r_[np.arange(3000), 3000 + cells]
    assert np.isfinite(c[:, cols]).all()
    rel = np.abs(dev.corrected[:, cols] - c[:, cols]).max() / np.abs(c[:, cols]).max()
    print(f"2 x 3000 x 2000, var.adj, {cells.size} sampled cells: max rel {rel:.2e}")
    assert rel < REL


def _as_dict(out):
    return {"corrected": out.corrected, "batch": out.batch}


@pytest.mark.parametrize("args", RESTRICT_ARGS)
def test_mnn_correct_restriction_identical(args):
    """test-mnn-correct.R:380-442 on the device: restricted to the original cells of batches with appended copies, the kept
    cells are the unrestricted result and the copies their originals', bit for bit; the single shuffled object with a
    logical restrict gives the same result in its column order."""
    B, C, picks, keep, o = check_restriction(lambda *b, **kw: _as_dict(bx.mnnCorrect(*b, **kw)), args)
    DY = np.hstack(C)
    n = [c.shape[1] for c in C]
    batch = np.repeat([1, 2, 3], n)
    shuffle = np.random.default_rng(7).permutation(DY.shape[1])
    kept = np.concatenate([keep[0], keep[1] + n[0], keep[2] + n[0] + n[1]])
    mask = np.isin(shuffle + 1, kept)
    out2 = bx.mnnCorrect(DY[:, shuffle], batch=batch[shuffle], restrict=[mask], **args)
    ref2 = o["corrected"][:, shuffle]
    assert np.abs(out2.corrected - ref2).max() <= 1e-8 * np.abs(ref2).max()  # expect_equal
    assert list(out2.batch) == [str(x) for x in np.asarray(o["batch"])[shuffle]]


def test_mnn_correct_raw_output_var_adj():
    """cos.norm.out=FALSE with var.adj: the output genes keep their raw scale, adjust_shift_variance's weights are then
    concentrated on one or two cells and its quantile walk turns on the last bits of the smoothed correction vectors
    (asv.hip's header; tests/testthat/test-mnn-correct.R:141 upstream).  Measured on these inputs: last-bit noise in the
    restatement's own correction vectors moves 303 of the 600 cells, the device differs from it in 299 -- so only the pairs
    are held here; the same path without var.adj is held to 1e-5 in test_mnn_correct_matches_restatement."""
    B = _batches(2 * 7 + 10, [100, 200, 300], 10)
    dev = bx.mnnCorrect(*B, cos_norm_out=False)
    cpu = ref.mnn_correct(*B, cos_norm_out=False)
    for (dl, dr), (cl, cr) in zip(dev.merge_info.pairs, cpu["pairs"]):
        assert np.array_equal(dl, cl) and np.array_equal(dr, cr)
    assert dev.corrected.shape == cpu["corrected"].shape and np.isfinite(dev.corrected).all()


def test_mnn_correct_restrict_duplicates():
    B = _batches(5, [100, 200, 300], 10)
    rng = np.random.default_rng(1)
    restrict = [np.sort(rng.choice(100, 60, replace=False)) + 1, None,
                np.concatenate([np.arange(1, 201), np.arange(1, 51)])]  # cells named twice
    dev = bx.mnnCorrect(*B, restrict=restrict)
    cpu = ref.mnn_correct(*B, restrict=restrict)
    _compare(dev, cpu, "restrict")
    # every cell named twice: each cell is two points to the search, one cell to the averaging
    dev2 = bx.mnnCorrect(*B, restrict=[None, None, np.concatenate([np.arange(1, 301), np.arange(1, 301)])])
    cpu2 = ref.mnn_correct(*B, restrict=[None, None, np.concatenate([np.arange(1, 301), np.arange(1, 301)])])
    _compare(dev2, cpu2, "restrict all twice")


def test_mnn_correct_single_object_with_names():
    B = _batches(9, [120, 180, 150], 10)
    x = np.hstack(B)
    lab = np.repeat(np.array(["b", "c", "a"]), [120, 180, 150])
    perm = np.random.default_rng(3).permutation(x.shape[1])
    x, lab = x[:, perm], lab[perm]
    dev = bx.mnnCorrect(x, batch=lab)
    parts = [x[:, lab == v] for v in ["a", "b", "c"]]
    cpu = ref.mnn_correct(*parts, names=["a", "b", "c"])
    # back to the caller's column order
    reorder = np.zeros(x.shape[1], dtype=np.int64)
    last = 0
    for v in ["a", "b", "c"]:
        keep = lab == v
        reorder[keep] = last + np.arange(1, keep.sum() + 1)
        last += keep.sum()
    c = cpu["corrected"][:, reorder - 1]
    assert list(dev.batch) == list(lab)
    assert dev.merge_info.left == [["a"], ["a", "b"]] and dev.merge_info.right == [["b"], ["c"]]
    assert np.abs(dev.corrected - c).max() / np.abs(c).max() < REL
    rev = np.zeros(reorder.size + 1, dtype=np.int64)
    rev[reorder] = np.arange(1, reorder.size + 1)
    for (dl, dr), (cl, cr) in zip(dev.merge_info.pairs, cpu["pairs"]):
        assert np.array_equal(dl, rev[cl]) and np.array_equal(dr, rev[cr])


@pytest.mark.parametrize("n1,n2,k", [(300, 250, 10), (700, 650, 600)])
def test_wide_average_correction_d1000(n1, n2, k):
    # (k = 600: right cells with more than 512 partners -- average_correction_wide stages them in several steps)
    rng = np.random.default_rng(11)
    d = 1000
    base = rng.normal(size=(3, d))
    d1 = rng.normal(size=(n1, 3)) @ base + rng.normal(scale=0.2, size=(n1, d))
    d2 = rng.normal(size=(n2, 3)) @ base + rng.normal(scale=0.2, size=(n2, d)) + 0.5
    L = _lib.lib()
    f, s, av, su = (ctypes.POINTER(ctypes.c_int32)(), ctypes.POINTER(ctypes.c_int32)(), ctypes.POINTER(ctypes.c_double)(),
                    ctypes.POINTER(ctypes.c_int32)())
    P, U = ctypes.c_int64(0), ctypes.c_int32(0)
    a1, a2 = np.asfortranarray(d1), np.asfortranarray(d2)
    _lib.check(L.bmx_mnn_average_correction(_lib.f64p(a1), n1, _lib.f64p(a2), n2, d, k, k, ctypes.byref(f), ctypes.byref(s),
                                            ctypes.byref(P), ctypes.byref(av), ctypes.byref(su), ctypes.byref(U)))
    first, second = _lib.take_i32(f, P.value), _lib.take_i32(s, P.value)
    u = U.value
    avg = np.ctypeslib.as_array(av, shape=(u * d,)).copy().reshape(d, u).T
    L.bmx_free(av)
    sec_u = _lib.take_i32(su, u)
    rf, rs = orc.find_mutual_nn(d1, d2, k, k)
    if k > 512:
        assert np.bincount(rs).max() > 512
    assert np.array_equal(first, rf) and np.array_equal(second, rs)
    ravg, rsec = orc.average_correction(d1, rf, d2, rs)
    assert np.array_equal(sec_u, rsec)
    assert np.abs(avg - ravg).max() / np.abs(ravg).max() <= 1e-12


def _asv_inputs(seed, g, n1, n2):
    rng = np.random.default_rng(seed)
    d1 = np.asfortranarray(rng.normal(size=(g, n1)))
    d2 = np.asfortranarray(rng.normal(size=(g, n2)) + 0.3)
    v = np.asfortranarray(rng.normal(scale=0.5, size=(n2, g)) + 0.2)
    return d1, d2, v


@pytest.mark.parametrize("g,n1,n2,r1,r2", [(10, 100, 200, None, None), (37, 150, 90, "sub", "dup"), (300, 64, 80, None, "sub")])
def test_asv_wide_hook_matches_exact(g, n1, n2, r1, r2):
    d1, d2, v = _asv_inputs(g + n1, g, n1, n2)
    rng = np.random.default_rng(5)
    R1 = np.arange(n1, dtype=np.int32) if r1 is None else np.sort(rng.choice(n1, n1 // 2, replace=False)).astype(np.int32)
    if r2 is None:
        R2 = np.arange(n2, dtype=np.int32)
    elif r2 == "dup":
        R2 = np.concatenate([np.arange(n2), np.arange(n2 // 3)]).astype(np.int32)
    else:
        R2 = np.sort(rng.choice(n2, n2 // 2, replace=False)).astype(np.int32)
    exact = bx.adjust_shift_variance(d1, d2, v, 0.1, R1, R2)
    _lib.dev_set("asv_wide", 1)
    try:
        wide = bx.adjust_shift_variance(d1, d2, v, 0.1, R1, R2)
        _lib.dev_set("asv_chunk", 7)  # several chunks sharing the scratch, c0 > 0
        chunked = bx.adjust_shift_variance(d1, d2, v, 0.1, R1, R2)
    finally:
        _lib.dev_set("asv_wide", 0)
        _lib.dev_set("asv_chunk", 0)
    assert np.array_equal(exact.view(np.int64), wide.view(np.int64))
    assert np.array_equal(exact.view(np.int64), chunked.view(np.int64))
    cpu = orc.adjust_shift_variance(d1, d2, v, 0.1, R1, R2)
    assert np.array_equal(cpu.view(np.int64), wide.view(np.int64))


def test_asv_wide_beyond_exact_size():
    # g = 300, n2 (nr1 + nr2) > 4e7: the tiled form's size, which refused g > 256; the literal wide form runs instead
    g, n1, n2 = 300, 4000, 6000
    d1, d2, v = _asv_inputs(3, g, n1, n2)
    R1 = np.arange(n1, dtype=np.int32)
    R2 = np.arange(n2, dtype=np.int32)
    assert n2 * (n1 + n2) > 4e7
    out = bx.adjust_shift_variance(d1, d2, v, 0.1, R1, R2)
    cells = np.random.default_rng(2).choice(n2, 24, replace=False).astype(np.int32)
    cpu = orc.adjust_shift_variance(d1, d2, v, 0.1, R1, R2, cells=cells)
    assert np.array_equal(out[cells].view(np.int64), cpu.view(np.int64))


def test_find_mutual_nn_d2000():
    rng = np.random.default_rng(8)
    d = 2000
    base = rng.normal(size=(4, d))
    d1 = rng.normal(size=(400, 4)) @ base + rng.normal(scale=0.3, size=(400, d))
    d2 = rng.normal(size=(350, 4)) @ base + rng.normal(scale=0.3, size=(350, d)) + 0.2
    f, s = bx.find_mutual_nn(d1, d2, 15, 15)
    rf, rs = orc.find_mutual_nn(d1, d2, 15, 15)
    assert np.array_equal(np.asarray(f), rf) and np.array_equal(np.asarray(s), rs)
