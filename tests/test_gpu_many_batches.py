"""Merges beyond 16 batches and 8 batch vectors on the device against the FP64 CPU oracle.

The engine walks a node's segments (its original batches) in groups of 16 and applies its batch vectors (its earlier
non-skipped merges) in launches of 8, the statistics riding on the last launch (correct.hip: rows_multi); above 16 segments
the column means fall back from the cached segment statistics to a reduction over the node (engine.hip: node_mean,
node_means).  The cases (tests/many_batches_cases.py) cross each of these boundaries; tests/test_cpu_many_batches.py shows
that their pair lists are no near-ties.  The bar is the project's own, assert_same_result: pairs bit-exact in order,
corrected within 1e-5 relative, batch_size within 1e-9, skipped equal, lost_var (one column per batch: every group's
per-segment statistics) within 1e-7.  Every test prints the worst relative errors it measured before it asserts."""
import copy
import time

import numpy as np
import pytest

from oracle import pca_oracle
from tests import many_batches_cases as mb
from tests import mnn_correct_ref
from tests.conftest import synth_batches
from tests.test_gpu_engine import assert_same_result
from tests.test_gpu_mnn_correct import _compare as compare_mnn_correct

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bx():
    import batchelor_amd
    return batchelor_amd


def measured(what, out_corrected, ref_corrected, out_info, ref_info, seconds):
    """Print the worst relative error of corrected (per column, over the column's largest entry: assert_same_result's
    measure) and of lost_var (over its non-zero entries), and the device call's wall time."""
    scale = np.abs(ref_corrected).max(axis=0)
    err_c = (np.abs(out_corrected - ref_corrected).max(axis=0) / scale).max()
    lv_o, lv_r = np.asarray(out_info.lost_var), np.asarray(ref_info.lost_var)
    nz = lv_r != 0
    err_v = (np.abs(lv_o - lv_r)[nz] / np.abs(lv_r[nz])).max() if lv_o.shape == lv_r.shape and nz.any() else float("nan")
    print(f"\n[many-batches] {what}: corrected max rel {err_c:.2e}, lost_var max rel {err_v:.2e}, device call {seconds:.2f} s")


def assert_reaches(case, info):
    shape = mb.merge_shape(info)
    assert case.reach(shape), (case.id, mb.max_segments(shape), mb.max_vectors(shape))


def numbered(out, nb):
    """A labelled result (batch= names s00, s01, ...: sorted, so level i is batch i + 1) with the oracle's batch numbers."""
    num = {f"s{b:02d}": b + 1 for b in range(nb)}
    res = copy.copy(out)
    res.batch = np.asarray([num[x] for x in out.batch], dtype=np.int32)
    res.merge_info = copy.copy(out.merge_info)
    res.merge_info.left = [[num[x] for x in side] for side in out.merge_info.left]
    res.merge_info.right = [[num[x] for x in side] for side in out.merge_info.right]
    return res


@pytest.mark.parametrize("case", mb.CASES, ids=lambda c: c.id)
def test_many_batches_match_oracle(bx, case):
    B = case.batches()
    ref = mb.reference(case.id)
    t0 = time.perf_counter()
    out = case.call(bx.reducedMNN, B)      # the Python front end: bmx_fast_mnn
    dt = time.perf_counter() - t0
    if case.labels:
        out = numbered(out, case.nb)
    measured(case.id, out.corrected, ref.corrected, out.merge_info, ref.merge_info, dt)
    assert_reaches(case, ref.merge_info)   # conditions on the input: from the oracle's result and from the device's
    assert_reaches(case, out.merge_info)
    assert tuple(int(m) for m in np.flatnonzero(ref.merge_info.skipped)) == (case.skips or ())
    assert_same_result(out, ref)


def test_nineteen_batches_twice_on_one_engine_then_three(bx, oracle):
    """Bitwise the same twice on one MnnEngine; then a 3-batch upload on the same engine still matches the oracle (the
    statistics slots and the vector pool are sized per upload and counted per run)."""
    case = mb.by_id("seq19_d100")
    ref = mb.reference(case.id)
    eng = bx.MnnEngine()
    try:
        eng.upload(case.batches())
        t0 = time.perf_counter()
        eng.run()
        dt = time.perf_counter() - t0
        a = eng.download()
        eng.run()
        b = eng.download()
        measured(case.id + " (engine, first run)", a.corrected, ref.corrected, a.merge_info, ref.merge_info, dt)
        assert np.array_equal(a.corrected, b.corrected)
        assert len(a.merge_info.pairs) == len(b.merge_info.pairs) == case.nb - 1
        for (al, ar), (bl, br) in zip(a.merge_info.pairs, b.merge_info.pairs):
            assert np.array_equal(al, bl) and np.array_equal(ar, br)
        assert np.array_equal(a.merge_info.lost_var, b.merge_info.lost_var)
        assert_reaches(case, a.merge_info)
        assert_same_result(a, ref)
        small = synth_batches(7, [300, 250, 350], 20)
        eng.upload(small)
        eng.run()
        c = eng.download()
    finally:
        eng.close()
    sref = oracle.reduced_mnn(*small)
    measured("3 batches after 19 on one engine", c.corrected, sref.corrected, c.merge_info, sref.merge_info, float("nan"))
    assert_same_result(c, sref)
    assert_same_result(bx.reducedMNN(*small), sref)   # and a fresh engine in the same process


def test_fast_mnn_front_end_eighteen_batches(bx):
    """fastMNN(): the multiBatchPCA of 18 batches on the device, then the engine -- compared as
    tests/test_gpu_fastmnn.py::test_fast_mnn_front_end does."""
    B = mb.fastmnn_batches()
    ref, meta = pca_oracle.fast_mnn(*B, d=8)
    t0 = time.perf_counter()
    out = bx.fastMNN(*B, d=8)
    dt = time.perf_counter() - t0
    sgn = np.sign((out.rotation * meta["rotation"]).sum(axis=0))
    measured("fastMNN, 18 batches", out.corrected * sgn[None, :], ref.corrected, out.merge_info, ref.merge_info, dt)
    shape = mb.merge_shape(out.merge_info)
    assert mb.max_segments(shape) > mb.SEG_GROUP and mb.max_vectors(shape) > mb.VEC_LAUNCH
    np.testing.assert_allclose(out.rotation * sgn[None, :], meta["rotation"], rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(out.corrected * sgn[None, :], ref.corrected, rtol=1e-5, atol=1e-8)
    assert len(out.merge_info.pairs) == len(ref.merge_info.pairs) == 17
    for (ol, orr), (rl, rr) in zip(out.merge_info.pairs, ref.merge_info.pairs):
        assert np.array_equal(ol, rl) and np.array_equal(orr, rr)
    assert list(out.batch) == list(ref.batch)


@pytest.mark.parametrize("var_adj", [True, False])
def test_mnn_correct_eighteen_batches(bx, var_adj):
    """mnnCorrect() over 18 batches of about 150 cells, 10 genes, against the CPU restatement, as
    tests/test_gpu_mnn_correct.py::test_mnn_correct_matches_restatement does."""
    B = mb.mnncorrect_batches()
    cpu = mnn_correct_ref.mnn_correct(*B, var_adj=var_adj)
    t0 = time.perf_counter()
    dev = bx.mnnCorrect(*B, var_adj=var_adj)
    dt = time.perf_counter() - t0
    c = np.asarray(cpu["corrected"])
    rel = np.abs(dev.corrected - c).max() / np.abs(c).max() if dev.corrected.shape == c.shape else float("nan")
    print(f"\n[many-batches] mnnCorrect, 18 batches, var_adj={var_adj}: corrected max rel {rel:.2e}, device call {dt:.2f} s")
    assert len(dev.merge_info.pairs) == 17
    compare_mnn_correct(dev, cpu, f"18 batches, var_adj={var_adj}")
