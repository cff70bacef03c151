"""mnnCorrect's CPU restatement (tests/mnn_correct_ref.py) against numpy transcriptions of the reference's own REF
functions and its property tests (tests/testthat/test-mnn-correct.R), and the argument checks of the device entry point,
which need no device."""
import ctypes

import numpy as np
import pytest

from tests import mnn_correct_ref as ref


def _ref_correction(data1, data2, mnn1, mnn2, s2):
    """REF of test-mnn-correct.R:36-63."""
    d2 = ((data2[:, None, :] - data2[None, :, :]) ** 2).sum(-1)
    w = np.exp(-d2 / s2)
    u = np.unique(mnn2)
    dens = w[:, u - 1].sum(1)
    N = np.bincount(mnn2, minlength=data2.shape[0] + 1)[1:]
    with np.errstate(divide="ignore", invalid="ignore"):
        kern = (w / (N * dens)[:, None]).T[:, mnn2 - 1]
    kern = kern / kern.sum(1, keepdims=True)
    return kern @ (data1[mnn1 - 1] - data2[mnn2 - 1])


@pytest.mark.parametrize("mnn1,mnn2,s2", [
    (np.arange(1, 11), np.arange(30, 20, -1), 0.1),
    (np.r_[11, 12, 13, np.arange(1, 11)], np.r_[30, 30, 30, np.arange(30, 20, -1)], 0.1),
    (np.arange(1, 201), np.arange(500, 300, -1), 0.1),
    (np.arange(1, 11), np.arange(30, 20, -1), 0.5),
])
def test_correction_vectors_against_ref(mnn1, mnn2, s2):
    rng = np.random.default_rng(0)
    data1 = rng.normal(scale=0.1, size=(400, 25))
    data2 = rng.normal(scale=0.1, size=(1000, 25))
    xx = ref.compute_correction_vectors(data1, data2, mnn1, mnn2, np.asfortranarray(data2.T), s2)
    np.testing.assert_allclose(xx, _ref_correction(data1, data2, mnn1, mnn2, s2), rtol=1e-6, atol=1e-12)


def _batches(seed=0):
    rng = np.random.default_rng(seed)
    return [rng.normal(size=(10, n)) + i * 0.5 for i, n in enumerate([100, 200, 300])]


def test_subsetting_properties():
    """test-mnn-correct.R:177-202."""
    B = _batches(1)
    sub = np.array([1, 3, 4, 6, 8, 10])
    a = ref.mnn_correct(*B, subset_row=sub)
    b = ref.mnn_correct(*[x[sub - 1] for x in B])
    assert np.array_equal(a["corrected"], b["corrected"])
    c = ref.mnn_correct(*B, subset_row=sub, correct_all=True)
    assert c["corrected"].shape[0] == 10
    for (l1, r1), (l2, r2) in zip(a["pairs"], c["pairs"]):
        assert np.array_equal(l1, l2) and np.array_equal(r1, r2)


def test_cosine_switches():
    """test-mnn-correct.R:204-253: cos.norm.out=FALSE keeps the pairs; cos.norm.in=FALSE equals pre-normalised inputs."""
    B = _batches(2)
    a = ref.mnn_correct(*B)
    b = ref.mnn_correct(*B, cos_norm_out=False)
    for (l1, r1), (l2, r2) in zip(a["pairs"], b["pairs"]):
        assert np.array_equal(l1, l2) and np.array_equal(r1, r2)
    normed = [ref.cosine_norm(x)[0] for x in B]
    c = ref.mnn_correct(*normed, cos_norm_in=False, cos_norm_out=False)
    np.testing.assert_allclose(a["corrected"], c["corrected"], rtol=1e-10, atol=1e-12)


def test_prop_k():
    """test-mnn-correct.R:255-274."""
    rng = np.random.default_rng(3)
    B1 = rng.normal(0, 1, size=(100, 100))
    B2 = rng.normal(1, 1, size=(100, 100))
    ref0 = ref.mnn_correct(B1, B2)
    assert np.array_equal(ref0["corrected"], ref.mnn_correct(B1, B2, k=10, prop_k=20 / B1.shape[1])["corrected"])
    assert np.array_equal(ref0["corrected"], ref.mnn_correct(B1, B2, prop_k=0)["corrected"])  # max() kicks in
    B2a = rng.normal(1, 1, size=(100, 200))  # prop.k gives k = 40 for the larger batch: another result
    assert not np.array_equal(ref.mnn_correct(B1, B2a)["corrected"],
                              ref.mnn_correct(B1, B2a, prop_k=20 / B1.shape[1])["corrected"])


def test_merge_order():
    """test-mnn-correct.R:276-305: a merge order equals the batches handed over in that order, columns back in place."""
    B = _batches(4)
    a = ref.mnn_correct(*B, merge_order=[3, 1, 2])
    b = ref.mnn_correct(B[2], B[0], B[1])
    n = [x.shape[1] for x in B]
    ref_cols = np.hstack([b["corrected"][:, n[2]:n[2] + n[0]], b["corrected"][:, n[2] + n[0]:], b["corrected"][:, :n[2]]])
    assert np.array_equal(a["corrected"], ref_cols)
    assert a["left"] == [[3], [3, 1]] and a["right"] == [[1], [2]]


def restriction_inputs(seed=0):
    """test-mnn-correct.R:380-393: each batch with copies of some of its cells appended, restricted to the originals."""
    rng = np.random.default_rng(seed)
    B = [rng.normal(0, 1, size=(100, 100)), rng.normal(2, 1, size=(100, 200)), rng.normal(3, 1, size=(100, 150))]
    picks = [np.arange(20, 9, -1), np.arange(30, 101), np.arange(100, 19, -1)]  # i1, i2, i3 (1-based)
    C = [np.hstack([b, b[:, i - 1]]) for b, i in zip(B, picks)]
    keep = [np.arange(1, b.shape[1] + 1) for b in B]
    return B, C, picks, keep


# the argument sets of test-mnn-correct.R:399-410 without svd.dim
RESTRICT_ARGS = [dict(var_adj=False), dict(), dict(subset_row=np.arange(50, 0, -1), correct_all=True)]


def check_restriction(run, args, seed=0):
    """test-mnn-correct.R:412-419: the kept cells are the unrestricted result, the copies their originals' -- identical."""
    B, C, picks, keep = restriction_inputs(seed)
    r = run(*B, **args)
    o = run(*C, restrict=keep, **args)
    rc, oc = np.asarray(r["corrected"]), np.asarray(o["corrected"])
    rb, ob = np.asarray(r["batch"]), np.asarray(o["batch"])
    for b in range(3):
        rcol, ocol = rc[:, rb == b + 1], oc[:, ob == b + 1]
        n = B[b].shape[1]
        assert np.array_equal(rcol, ocol[:, :n])
        assert np.array_equal(rcol[:, picks[b] - 1], ocol[:, n:])
    return B, C, picks, keep, o


@pytest.mark.parametrize("args", RESTRICT_ARGS)
def test_restriction_bitwise(args):
    check_restriction(ref.mnn_correct, args)


def test_names():
    """test-mnn-correct.R:444-477."""
    B = _batches(6)
    a = ref.mnn_correct(*B, names=["x", "y", "z"])
    assert list(np.unique(a["batch"])) == ["x", "y", "z"]
    assert a["left"] == [["x"], ["x", "y"]] and a["right"] == [["y"], ["z"]]


def test_entry_point_exported():
    import batchelor_amd as bx
    from batchelor_amd import _lib
    assert callable(bx.mnnCorrect)
    for sym in ("bmx_mnn_correct", "bmx_mnn_result_sizes", "bmx_mnn_result_into", "bmx_mnn_result_free"):
        assert hasattr(_lib.lib(), sym)


@pytest.mark.parametrize("call,msg", [
    (lambda bx, B: bx.mnnCorrect(B[0]), "'batch' must be specified"),
    (lambda bx, B: bx.mnnCorrect(B[0], B[1], svd_dim=2), "svd.dim"),
    (lambda bx, B: bx.mnnCorrect(B[0], B[1], auto_merge=True), "auto.merge"),
    (lambda bx, B: bx.mnnCorrect(B[0], B[1][:5]), "number of rows is not the same across batches"),
    (lambda bx, B: bx.mnnCorrect(B[0], B[1], names=["a", "a"]), "names of batches should be unique"),
])
def test_bad_arguments(call, msg):
    import batchelor_amd as bx
    with pytest.raises(ValueError, match=msg.replace("(", r"\(").replace(".", r"\.")):
        call(bx, _batches(7))


def test_abi_checks_before_device():
    from batchelor_amd import _lib
    from batchelor_amd.mnn_correct import BmxMnnParams
    L = _lib.lib()
    x = np.asfortranarray(np.ones((4, 3)))
    data = (ctypes.c_void_p * 1)(x.ctypes.data)
    n = np.array([3], dtype=np.int32)
    tree = np.array([1], dtype=np.int32)
    p = BmxMnnParams(ctypes.sizeof(BmxMnnParams), 20, float("nan"), 0.1, 1, 1, 1, 0, 0, 0, None, 0, tree.ctypes.data, 1)
    h = ctypes.c_void_p()
    rc = L.bmx_mnn_correct(1, 4, data, _lib.i32p(n), None, None, ctypes.byref(p), ctypes.byref(h))
    assert rc != 0 and L.bmx_last_error() == b"at least two batches must be specified"
    data2 = (ctypes.c_void_p * 2)(x.ctypes.data, x.ctypes.data)
    n2 = np.array([3, 3], dtype=np.int32)
    tree2 = np.array([1, 2, 0], dtype=np.int32)
    p2 = BmxMnnParams(ctypes.sizeof(BmxMnnParams), 20, float("nan"), 0.1, 1, 1, 1, 0, 2, 0, None, 0, tree2.ctypes.data, 3)
    rc = L.bmx_mnn_correct(2, 4, data2, _lib.i32p(n2), None, None, ctypes.byref(p2), ctypes.byref(h))
    assert rc != 0 and b"svd.dim" in L.bmx_last_error()
