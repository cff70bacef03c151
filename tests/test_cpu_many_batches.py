"""The inputs of tests/test_gpu_many_batches.py are not near-ties: the FP64 oracle's MNN pair lists, merge sets and skip
pattern are unchanged when every input is multiplied by 1 + 1e-11 N(0, 1) -- a hundred times the device's distance from
the oracle -- and every case reaches the segment-group / vector-launch boundary it is there for (tests/many_batches_cases.py).
A pair mismatch of the device on these inputs is therefore a finding.  Oracle only: no device, no extension."""
import types

import numpy as np
import pytest

from oracle import fastmnn_oracle as orc
from oracle import pca_oracle
from tests import many_batches_cases as mb
from tests import mnn_correct_ref


def _same_pairs(a, b):
    assert len(a) == len(b)
    for (al, ar), (bl, br) in zip(a, b):
        assert np.array_equal(al, bl) and np.array_equal(ar, br)


def test_merge_shape_counts_segments_and_vectors():
    # ((1, 2), 3) with the first merge skipped, then 4 | 5, then the two halves
    info = types.SimpleNamespace(left=[[1], [1, 2], [4], [1, 2, 3]], right=[[2], [3], [5], [4, 5]],
                                 skipped=np.array([True, False, False, False]))
    shape = mb.merge_shape(info)
    assert [m["segments"] for m in shape] == [2, 3, 2, 5]
    assert [(m["vec_left"], m["vec_right"]) for m in shape] == [(0, 0), (0, 0), (0, 0), (1, 1)]
    assert mb.max_segments(shape) == 5 and mb.max_vectors(shape) == 1
    assert mb.balanced_tree(1, 5) == [[[1, 2], 3], [4, 5]]


@pytest.mark.parametrize("case", mb.CASES, ids=lambda c: c.id)
def test_oracle_pairs_do_not_move_under_perturbation(case):
    ref = mb.reference(case.id)
    got = case.call(orc.reduced_mnn, mb.perturb(case.batches()))
    info = ref.merge_info
    assert len(info.pairs) == case.nb - 1 and all(p[0].size > 0 for p in info.pairs)
    assert got.merge_info.left == info.left and got.merge_info.right == info.right   # (auto-merge: the same choices)
    _same_pairs(got.merge_info.pairs, info.pairs)
    skipped = tuple(int(m) for m in np.flatnonzero(info.skipped))
    assert skipped == (case.skips or ())
    assert np.array_equal(got.merge_info.skipped, info.skipped)
    if case.skips:  # in the middle of the chain, the rest corrected; the threshold is far from every batch size
        assert 0 < min(skipped) and max(skipped) < case.nb - 2
        assert np.abs(info.batch_size - case.kw["min_batch_skip"]).min() > 0.03
    shape = mb.merge_shape(info)
    assert case.reach(shape), (mb.max_segments(shape), mb.max_vectors(shape))


def test_fastmnn_front_end_inputs_are_stable():
    B = mb.fastmnn_batches()
    ref, _ = pca_oracle.fast_mnn(*B, d=8)
    got, _ = pca_oracle.fast_mnn(*mb.perturb(B), d=8)
    assert not ref.merge_info.skipped.any()
    _same_pairs(got.merge_info.pairs, ref.merge_info.pairs)
    shape = mb.merge_shape(ref.merge_info)
    assert mb.max_segments(shape) > mb.SEG_GROUP and mb.max_vectors(shape) > mb.VEC_LAUNCH


@pytest.mark.parametrize("var_adj", [True, False])
def test_mnn_correct_inputs_are_stable(var_adj):
    B = mb.mnncorrect_batches()
    assert len(B) == 18 and all(b.shape[0] == 10 for b in B)
    ref = mnn_correct_ref.mnn_correct(*B, var_adj=var_adj)
    got = mnn_correct_ref.mnn_correct(*mb.perturb(B), var_adj=var_adj)
    _same_pairs(got["pairs"], ref["pairs"])
    assert np.isfinite(ref["corrected"]).all()
