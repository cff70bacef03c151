"""mnnCorrect() on scipy.sparse batches without a GPU: the bmx_mnn_correct_sparse symbol, the entry point's refusals that
need no device, the front end's argument errors, which are raised before a device is asked for, and the canonical CSC
the library is handed."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from tests.test_cpu_inputs import _refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "batchelor_mi355x.h")).read()
ERR_ARG, ERR_TREE = (int(re.search(rf"#define {name} \((-\d+)\)", HEADER).group(1)) for name in ("BMX_ERR_ARG", "BMX_ERR_TREE"))


def _sparse_batches(seed=0, cells=(30, 40, 50), G=10, density=0.3):
    rng = np.random.default_rng(seed)
    return [sp.csc_matrix(rng.normal(size=(G, n)) * (rng.random((G, n)) < density)) for n in cells]


def test_abi_export():
    import __graft_entry__ as g
    g.build()
    lib = ctypes.CDLL(os.path.join(ROOT, "batchelor_amd", "libbatchelor_mi355x.so"))
    assert hasattr(lib, "bmx_mnn_correct_sparse")
    assert "bmx_mnn_correct_sparse(" in HEADER


class _Call:
    """The arguments of one bmx_mnn_correct_sparse call over two small CSC batches of 4 genes; a test edits a field, then
    run() returns (status, message)."""

    def __init__(self):
        from batchelor_amd.mnn_correct import BmxMnnParams
        self.B, self.G = 2, 4
        self.indptr = [np.array([0, 2, 3, 3], dtype=np.int64), np.array([0, 1, 2], dtype=np.int64)]
        self.indices = [np.array([0, 3, 1], dtype=np.int32), np.array([2, 0], dtype=np.int32)]
        self.data = [np.array([1.0, 2.0, 3.0]), np.array([4.0, 5.0])]
        self.ncells = np.array([3, 2], dtype=np.int32)
        self.tree = np.array([1, 2, 0], dtype=np.int32)
        self.svd_dim = self.auto_merge = 0
        self.null = ()   # names of the arrays handed over as NULL
        self.params = BmxMnnParams

    def run(self):
        from batchelor_amd import _lib
        L = _lib.lib()

        def ptrs(name):
            if name in self.null:
                return None
            return (ctypes.c_void_p * self.B)(*[a.ctypes.data for a in getattr(self, name)[:self.B]])

        p = self.params(ctypes.sizeof(self.params), 20, float("nan"), 0.1, 1, 1, 1, 0, self.svd_dim, self.auto_merge, None,
                        0, self.tree.ctypes.data, int(self.tree.size))
        h = ctypes.c_void_p()
        rc = L.bmx_mnn_correct_sparse(ctypes.c_int32(self.B), ctypes.c_int32(self.G), ptrs("indptr"), ptrs("indices"),
                                      ptrs("data"), None if "ncells" in self.null else _lib.i32p(self.ncells), None, None,
                                      ctypes.byref(p), ctypes.byref(h))
        assert not h   # (nothing to free: no call here gets as far as a result)
        return rc, L.bmx_last_error().decode()


@pytest.mark.parametrize("null", ["indptr", "indices", "data", "ncells"])
def test_entry_refuses_a_null_array(null):
    c = _Call()
    c.null = (null,)
    rc, msg = c.run()
    assert rc == ERR_ARG and "null batch arrays" in msg


def test_entry_refuses_a_batch_whose_entries_are_missing():
    """indices[b] / data[b] may be null only when the batch has no stored entry."""
    from batchelor_amd import _lib
    from batchelor_amd.mnn_correct import BmxMnnParams
    L = _lib.lib()
    c = _Call()
    for missing in ("indices", "data"):
        arrs = {k: (ctypes.c_void_p * 2)(*[a.ctypes.data for a in getattr(c, k)]) for k in ("indptr", "indices", "data")}
        arrs[missing][1] = None
        p = BmxMnnParams(ctypes.sizeof(BmxMnnParams), 20, float("nan"), 0.1, 1, 1, 1, 0, 0, 0, None, 0, c.tree.ctypes.data, 3)
        h = ctypes.c_void_p()
        rc = L.bmx_mnn_correct_sparse(ctypes.c_int32(2), ctypes.c_int32(4), arrs["indptr"], arrs["indices"], arrs["data"],
                                      _lib.i32p(c.ncells), None, None, ctypes.byref(p), ctypes.byref(h))
        assert rc == ERR_ARG and "'indices' or 'data' is missing" in L.bmx_last_error().decode() and not h


def test_entry_refuses_fewer_than_two_batches():
    c = _Call()
    c.B = 1
    c.tree = np.array([1], dtype=np.int32)
    rc, msg = c.run()
    assert rc == ERR_ARG and msg == "at least two batches must be specified"


@pytest.mark.parametrize("indptr,msg", [
    ([1, 2, 3, 3], "'indptr' does not start at 0"),
    ([0, 2, 1, 3], "'indptr' decreases"),
    ([0, 2, 3, -1], "negative"),
])
def test_entry_refuses_a_bad_indptr(indptr, msg):
    c = _Call()
    c.indptr[0] = np.array(indptr, dtype=np.int64)
    rc, text = c.run()
    assert rc == ERR_ARG and msg in text


def test_entry_refuses_an_indptr_that_does_not_end_at_the_entries_given():
    """One batch without stored entries (null indices and data, as the header allows) whose indptr ends at 1."""
    from batchelor_amd import _lib
    from batchelor_amd.mnn_correct import BmxMnnParams
    L = _lib.lib()
    c = _Call()
    for last, want in ((0, None), (1, "'indices' or 'data' is missing")):
        empty = np.array([0, 0, last], dtype=np.int64)
        indptr = (ctypes.c_void_p * 2)(c.indptr[0].ctypes.data, empty.ctypes.data)
        indices = (ctypes.c_void_p * 2)(c.indices[0].ctypes.data, None)
        data = (ctypes.c_void_p * 2)(c.data[0].ctypes.data, None)
        # (the batch whose indptr ends at 0 is accepted: a bad tree, checked after the batches, ends that call)
        tree = np.array([1, 1, 0] if want is None else [1, 2, 0], dtype=np.int32)
        p = BmxMnnParams(ctypes.sizeof(BmxMnnParams), 20, float("nan"), 0.1, 1, 1, 1, 0, 0, 0, None, 0, tree.ctypes.data, 3)
        h = ctypes.c_void_p()
        rc = L.bmx_mnn_correct_sparse(ctypes.c_int32(2), ctypes.c_int32(4), indptr, indices, data, _lib.i32p(c.ncells), None,
                                      None, ctypes.byref(p), ctypes.byref(h))
        assert rc == (ERR_TREE if want is None else ERR_ARG) and (want or "merge.order") in L.bmx_last_error().decode()
        assert not h


def test_entry_refuses_svd_dim_auto_merge_and_a_bad_tree():
    c = _Call()
    c.svd_dim = 2
    rc, msg = c.run()
    assert rc == ERR_ARG and "svd.dim" in msg
    c = _Call()
    c.auto_merge = 1
    rc, msg = c.run()
    assert rc == ERR_ARG and "auto.merge" in msg
    for tree in ([1, 1, 0], [1, 0, 2], [1, 2], [1, 3, 0]):
        c = _Call()
        c.tree = np.array(tree, dtype=np.int32)
        rc, msg = c.run()
        assert rc == ERR_TREE and "merge" in msg, tree


def test_a_mixture_of_sparse_and_dense_is_refused():
    import batchelor_amd as bx
    b = _sparse_batches()
    for args in ((b[0], b[1].toarray()), (b[0].toarray(), sp.csr_array(b[1]), b[2])):
        with pytest.raises(TypeError, match="mnnCorrect takes batches that are all sparse or all dense, not a mixture"):
            bx.mnnCorrect(*args)
    with pytest.raises(TypeError, match="all sparse or all dense, not a mixture"):
        bx.batchCorrect(b[0], b[1].toarray(), PARAM=bx.ClassicMnnParam())


@pytest.mark.parametrize("form", [sp.csc_matrix, sp.csr_array, sp.coo_matrix], ids=["csc_matrix", "csr_array", "coo_matrix"])
def test_argument_errors_are_the_dense_call_s_and_need_no_device(form):
    b = _sparse_batches()
    s = [form(m) for m in b]
    one = form(sp.hstack(b))
    batch = np.repeat([1, 2, 3], [30, 40, 50])
    cases = [
        ((s[0], form(b[1][:5])), {}, "number of rows is not the same across batches"),
        ((s[0], s[1]), {"names": ["a", "a"]}, "names of batches should be unique"),
        ((s[0], s[1]), {"svd_dim": 2}, "svd.dim"),
        ((s[0], s[1]), {"auto_merge": True}, "auto.merge"),
        ((s[0], s[1]), {"restrict": [[1, 31], None]}, "'restrict' indices out of range"),
        ((s[0], s[1]), {"restrict": [[0], None]}, "'restrict' indices out of range"),
        ((s[0], s[1]), {"restrict": [None]}, "'restrictions' must of length equal to the number of batches"),
        ((s[0], s[1]), {"restrict": [np.zeros(0, dtype=int), None]}, "no cells remaining in a batch after restriction"),
        ((s[0],), {}, "'batch' must be specified if '...' has only one object"),
        ((one,), {"batch": batch[:-1]}, "'length(batch)' and 'ncol(x)' are not the same"),
        ((one,), {"batch": batch, "svd_dim": 2}, "svd.dim"),
        ((one,), {"batch": batch, "restrict": [np.arange(1, 31)]}, "no cells remaining in a batch after restriction"),
        ((s[0], s[1]), {"subset_row": [0, 1]}, "subset indices out of range"),
        ((s[0], s[1]), {"merge_order": [1, 1]}, None),
    ]
    for args, kwargs, msg in cases:
        dense = tuple(a.toarray() for a in args)
        if msg is None:   # whatever the dense call says of this merge order, the sparse call says
            import batchelor_amd as bx
            with pytest.raises(ValueError) as want:
                bx.mnnCorrect(*dense, **kwargs)
            msg = str(want.value)
        else:
            _refused("mnnCorrect", dense, kwargs, msg)   # what the dense call says ...
        _refused("mnnCorrect", args, kwargs, msg)        # ... the sparse call says, and before a device is asked for
    _refused("batchCorrect", (s[0], s[1]), {"PARAM": __import__("batchelor_amd").ClassicMnnParam(svd_dim=2)}, "svd.dim")


class _Handed(Exception):
    pass


def _capture(monkeypatch, args, **kw):
    """What mnnCorrect hands to bmx_mnn_correct_sparse for these arguments, with the library and the device stubbed:
    (G, per batch (indptr, indices, data) as copies, ncells)."""
    import batchelor_amd as bx
    from batchelor_amd import _lib
    seen = {}

    class Stub:
        @staticmethod
        def bmx_set_device(_dev):
            return 0

        @staticmethod
        def bmx_mnn_correct(*_a):
            raise AssertionError("sparse batches went to the dense entry point")

        @staticmethod
        def bmx_mnn_correct_sparse(B, G, indptr, indices, data, ncells, _r, _rn, _p, _h):
            n = np.ctypeslib.as_array(ncells, shape=(B.value,)).copy()
            out = []
            for b in range(B.value):
                ip = np.ctypeslib.as_array(ctypes.cast(indptr[b], _lib.c_i64p), shape=(int(n[b]) + 1,)).copy()
                nnz = int(ip[-1])
                ix = np.ctypeslib.as_array(ctypes.cast(indices[b], _lib.c_i32p), shape=(nnz,)).copy() if nnz else np.zeros(0, np.int32)
                v = np.ctypeslib.as_array(ctypes.cast(data[b], _lib.c_f64p), shape=(nnz,)).copy() if nnz else np.zeros(0)
                out.append((ip, ix, v))
            seen.update(G=G.value, batches=out, ncells=n)
            raise _Handed()

    monkeypatch.setattr(_lib, "require_gpu", lambda: None)
    monkeypatch.setattr(_lib, "lib", lambda: Stub)
    with pytest.raises(_Handed):
        bx.mnnCorrect(*args, **kw)
    return seen


def _assert_is_csc_of(handed, dense):
    ip, ix, v = handed
    want = sp.csc_matrix(dense)
    want.sort_indices()
    got = sp.csc_matrix((v, ix, ip), shape=dense.shape)
    assert ip.dtype == np.int64 and ix.dtype == np.int32 and v.dtype == np.float64
    assert got.has_canonical_format
    assert np.array_equal(got.toarray(), dense)
    return got


def test_the_library_is_handed_canonical_csc_and_the_caller_keeps_its_object(monkeypatch):
    rng = np.random.default_rng(3)
    G, n = 7, 12
    # COO with duplicate entries (which add up) and rows in no order
    r = rng.integers(0, G, size=60)
    c = rng.integers(0, n, size=60)
    v = rng.normal(size=60)
    coo = sp.coo_matrix((v, (r, c)), shape=(G, n))
    assert len(set(zip(r.tolist(), c.tolist()))) < 60
    csr = sp.csr_matrix(rng.normal(size=(G, 9)) * (rng.random((G, 9)) < 0.4))
    # CSC whose rows descend within every column, int64 indices, float32 data
    base = sp.csc_matrix((rng.normal(size=(G, 5)) * (rng.random((G, 5)) < 0.6)).astype(np.float32))
    order = np.concatenate([np.arange(base.indptr[j + 1] - 1, base.indptr[j] - 1, -1) for j in range(5)]).astype(np.int64)
    rev = sp.csc_matrix((base.data[order], base.indices[order].astype(np.int64), base.indptr.astype(np.int64)), shape=base.shape)
    assert not rev.has_sorted_indices or base.nnz < 2
    keep = [(coo.row.copy(), coo.col.copy(), coo.data.copy()), (csr.indptr.copy(), csr.indices.copy(), csr.data.copy()),
            (rev.indptr.copy(), rev.indices.copy(), rev.data.copy())]
    seen = _capture(monkeypatch, (coo, csr, rev))
    assert seen["G"] == G and seen["ncells"].tolist() == [12, 9, 5]
    for handed, m in zip(seen["batches"], (coo, csr, rev)):
        _assert_is_csc_of(handed, m.toarray().astype(np.float64))
    # the caller's objects: same arrays, same contents, same format
    assert coo.format == "coo" and csr.format == "csr" and rev.format == "csc"
    for got, want in zip([(coo.row, coo.col, coo.data), (csr.indptr, csr.indices, csr.data), (rev.indptr, rev.indices, rev.data)],
                         keep):
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and np.array_equal(a, b)


def test_stored_zeros_stay_and_one_object_is_split_by_batch(monkeypatch):
    G = 5
    x = sp.csc_matrix((np.array([0.0, -0.0, 2.0, 3.0]), np.array([1, 4, 0, 2]), np.array([0, 2, 2, 3, 4])), shape=(G, 4))
    seen = _capture(monkeypatch, (x, x))
    ip, ix, v = seen["batches"][0]
    assert ip.tolist() == [0, 2, 2, 3, 4] and ix.tolist() == [1, 4, 0, 2]
    assert np.array_equal(v.view(np.int64), np.array([0.0, -0.0, 2.0, 3.0]).view(np.int64))   # (the sign of the zero too)
    batch = np.array(["b", "a", "b", "a"])
    seen = _capture(monkeypatch, (sp.coo_matrix(x),), batch=batch)
    assert seen["ncells"].tolist() == [2, 2]
    d = x.toarray()
    _assert_is_csc_of(seen["batches"][0], d[:, [1, 3]])   # level "a" first
    _assert_is_csc_of(seen["batches"][1], d[:, [0, 2]])
