"""The Python side of a library handle that keeps genes x cells batches in HBM, dense (bmx_pca_t, bmx_cluster_t,
bmx_linear_t, bmx_norm_t, bmx_delta_t) or as CSC (bmx_pca_sparse_t, bmx_norm_sparse_t, bmx_delta_sparse_t,
bmx_cluster_sparse_t), or that streams them through block buffers
(bmx_genevar_t, bmx_genevar_sparse_t)."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .inputs import csc_blocks


class ResidentHandle:
    """Create / destroy by entry-point prefix, the blocked upload of a batch and the stage times.  A subclass names its
    PREFIX ("bmx_pca": bmx_pca_create, bmx_pca_destroy, bmx_pca_begin_batch, ...) and the STAGES of its stage_ms."""
    PREFIX = ""
    STAGES = ()

    def __init__(self, n_genes, device, *create_args):
        destroy = self._entry("destroy")
        destroy.argtypes = [ctypes.c_void_p]
        destroy.restype = None
        self._h = ctypes.c_void_p()
        self.G = int(n_genes)
        self.ncells = []
        _lib.check(self._entry("create")(ctypes.c_int32(int(device)), ctypes.c_int32(self.G), *create_args,
                                         ctypes.byref(self._h)))

    def _entry(self, name):
        return getattr(_lib.lib(), f"{self.PREFIX}_{name}")

    def _call(self, name, *args):
        _lib.check(self._entry(name)(self._h, *args))

    def close(self):
        if self._h:
            self._entry("destroy")(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _upload(self, x, block_bytes, *begin_args):
        """x: genes x cells, announced with begin_batch(n, *begin_args).  Above block_bytes (None: never) the batch goes
        over in column blocks, converted to column-major one block at a time (the whole matrix never exists twice on the
        host)."""
        n = int(x.shape[1])
        block = n if block_bytes is None else max(1, int(block_bytes) // (8 * self.G))
        self._call("begin_batch", ctypes.c_int64(n), *begin_args)
        for a in range(0, n, max(1, block)):
            xb = _lib.as_f(x[:, a:a + block])
            self._call("add_block", _lib.f64p(xb), ctypes.c_int64(xb.shape[1]))
        self.ncells.append(n)

    def _upload_csc(self, c, per, *begin_args, nnz_first=False):
        """c: canonical CSC (inputs.canonical_csc), announced with begin_batch(n, *begin_args, nnz) -- nnz_first:
        begin_batch(n, nnz, *begin_args), as bmx_cluster_sparse_begin_batch takes it --; it goes over in column blocks of
        `per` cells."""
        n = int(c.shape[1])
        nnz = ctypes.c_int64(int(c.nnz))
        self._call("begin_batch", ctypes.c_int64(n), *((nnz, *begin_args) if nnz_first else (*begin_args, nnz)))
        self.ncells.append(n)
        for block in csc_blocks(c, per):
            self._add_csc_block(*block)

    def _add_csc_block(self, m, indptr, indices, data):
        self._call("add_block", ctypes.c_int64(int(m)), indptr.ctypes.data_as(_lib.c_i64p), _lib.i32p(indices),
                   _lib.f64p(data), ctypes.c_int64(int(data.size)))

    def stage_ms(self):
        st = np.zeros(len(self.STAGES), dtype=np.float64)
        self._call("stage_ms", _lib.f64p(st))
        return dict(zip(self.STAGES, st.tolist()))
