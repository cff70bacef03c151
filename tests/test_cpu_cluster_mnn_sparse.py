"""clusterMNN() on scipy.sparse batches without a GPU: the bmx_cluster_sparse_* symbols, the entry points' refusals that need
no device, and the front end's argument errors, which are the dense call's and are raised before a device is asked for."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests.test_cpu_cluster_mnn import mock_batches
from tests.test_cpu_inputs import _refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("bmx_cluster_sparse_create", "bmx_cluster_sparse_destroy", "bmx_cluster_sparse_begin_batch",
           "bmx_cluster_sparse_add_block", "bmx_cluster_sparse_centroids", "bmx_cluster_sparse_propagate",
           "bmx_cluster_sparse_stage_ms")
FORMS = [sp.csc_matrix, sp.csr_array]


def sparse_mock(form, **kw):
    """mock_batches with about two thirds of the values set to zero, in the given scipy.sparse form."""
    batches, clusters = mock_batches(**kw)
    rng = np.random.default_rng(77)
    return [form(b * (rng.random(b.shape) < 0.35)) for b in batches], clusters


def test_abi_exports():
    import __graft_entry__ as g
    g.build()
    lib = ctypes.CDLL(os.path.join(ROOT, "batchelor_amd", "libbatchelor_mi355x.so"))
    header = open(os.path.join(ROOT, "include", "batchelor_mi355x.h")).read()
    for sym in SYMBOLS:
        assert hasattr(lib, sym), sym
        assert sym + "(" in header, sym


def test_entries_refuse_a_null_handle_and_bad_arguments_without_a_device():
    from batchelor_amd import _lib
    L = _lib.lib()
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    h = ctypes.c_void_p()
    assert L.bmx_cluster_sparse_create(i32(0), i32(0), None, i32(0), ctypes.byref(h)) == -6
    assert "gene" in L.bmx_last_error().decode()
    sub = np.array([1, 99], dtype=np.int32)
    assert L.bmx_cluster_sparse_create(i32(0), i32(10), _lib.i32p(sub), i32(2), ctypes.byref(h)) == -4
    assert "out of range" in L.bmx_last_error().decode()
    assert L.bmx_cluster_sparse_create(i32(0), i32(10), None, i32(2), ctypes.byref(h)) == -6
    assert "subset_row" in L.bmx_last_error().decode()
    assert L.bmx_cluster_sparse_create(i32(0), i32(10), None, i32(0), None) == -6
    assert not h
    ids = np.zeros(1, dtype=np.int32)
    out = np.zeros(4)
    for call in (lambda: L.bmx_cluster_sparse_begin_batch(None, i64(1), i64(0), _lib.i32p(ids), i32(1), None, i64(-1), i32(0)),
                 lambda: L.bmx_cluster_sparse_add_block(None, i64(1), None, None, None, i64(0)),
                 lambda: L.bmx_cluster_sparse_centroids(None, i32(0), _lib.f64p(out)),
                 lambda: L.bmx_cluster_sparse_propagate(None, i32(0), _lib.f64p(out), i32(1), _lib.f64p(out), _lib.f64p(out),
                                                        _lib.f64p(out), _lib.f64p(out), None),
                 lambda: L.bmx_cluster_sparse_stage_ms(None, _lib.f64p(out))):
        assert call() == -6
        assert L.bmx_last_error()


def test_a_mixture_of_sparse_and_dense_is_refused():
    import batchelor_amd as bx
    (b1, b2), (c1, c2) = mock_batches(n=(60, 70), genes=30)
    for args in ((sp.csc_matrix(b1), b2), (b1, sp.csr_array(b2))):
        with pytest.raises(TypeError, match="all sparse or all dense, not a mixture"):
            bx.clusterMNN(*args, clusters=[c1, c2])


@pytest.mark.parametrize("form", FORMS, ids=["csc_matrix", "csr_array"])
def test_argument_errors_are_the_dense_call_s_and_need_no_device(form):
    from batchelor_amd import KmeansParam
    (b1, b2), (c1, c2) = mock_batches(n=(60, 70), genes=30)
    s1, s2 = form(b1), form(b2)
    one = form(np.hstack([b1, b2]))
    batch = np.repeat([1, 2], [60, 70])
    big = [form(np.random.default_rng(5).normal(size=(30, 200))) for _ in range(2)]
    cases = [
        ((s1, s2), {"clusters": [c1]}, "should be of the same length"),
        ((s1, s2), {"clusters": [c1, c2[:-1]]}, "should have the same number of cells"),
        ((s1, s2), {"clusters": 1}, "must be either a list or a BlusterParam object"),
        ((one,), {"batch": batch, "clusters": [c1, c2]}, "must be a list of length 1"),
        ((one,), {"batch": batch[:-1], "clusters": [np.r_[c1, c2]]}, "'length(batch)' and 'ncol(x)' are not the same"),
        ((s1, s2), {"clusters": [c1, c2], "restrict": [None]}, "'restrictions' must of length equal to the number of batches"),
        ((s1, s2), {"clusters": [c1, c2], "restrict": [np.zeros(0, dtype=int), None]},
         "no cells remaining in a batch after restriction"),
        ((one,), {"batch": batch, "clusters": [np.r_[c1, c2]], "restrict": [np.arange(1, 61)]},
         "no cells remaining in a batch after restriction"),
        ((s1, s2), {"clusters": [c1, c2], "restrict": [np.flatnonzero(c1 != c1[0]) + 1, None]},
         "no cells remaining after restriction"),
        ((s1, form(b2[:-1])), {"clusters": [c1, c2]}, "number of rows is not the same across batches"),
        ((s1,), {"clusters": [c1]}, "'batch' must be specified if '...' has only one object"),
        (tuple(big), {"clusters": [np.arange(200) % 130, np.arange(200) % 130]}, "at most 256"),
        (tuple(big), {"clusters": KmeansParam(130)}, "at most 256"),
        ((s1, s2), {"clusters": KmeansParam(3), "cluster_d": 0}, "'cluster_d' must be a positive integer or None"),
        ((s1, s2), {"clusters": KmeansParam(3), "cluster_d": 2.5}, "'cluster_d' must be a positive integer or None"),
        ((s1, s2), {"clusters": [c1, c2], "subset_row": [0, 1]}, "subset indices out of range"),
        ((s1, s2), {"clusters": [c1, c2], "subset_row": []}, "'subset_row' selects no genes"),
    ]
    for args, kwargs, msg in cases:
        dense = tuple(a.toarray() for a in args)
        _refused("clusterMNN", dense, kwargs, msg)   # what the dense call says ...
        _refused("clusterMNN", args, kwargs, msg)    # ... the sparse call says, and before a device is asked for
