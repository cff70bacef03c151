"""mnnCorrect() (R/mnnCorrect.R:125-168): the classic gene-space MNN correction, end to end on the device behind
bmx_mnn_correct (csrc/mnn_correct.hip).

Batches are genes x cells, as in R.  `names` plays the role of the argument names of `...`.

The batches are all dense or all scipy.sparse (any format, matrix or array: what multiBatchNorm returns for sparse counts
goes straight in).  Sparse ones are made canonical CSC on the host and go up as CSC, 12 bytes a stored entry, behind
bmx_mnn_correct_sparse; the device expands them into the rows the correction works on -- the `subset_row` genes, and all
genes only with `correct_all` -- and everything from the first merge on is the dense call's, so the result is the dense
call's bit for bit: `corrected` is dense.

Out of scope here (a clear error): svd.dim > 0, auto.merge = TRUE, SingleCellExperiment inputs, a mixture of sparse and
dense batches.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Any, List, Optional

import numpy as np

from . import _lib
from .inputs import (all_sparse, apply_names, canonical_csc, check_same_dim, check_same_rows, check_unique_names,
                     divide_into_batches, pack_restrictions, reindex_pairings, restrict_list, subset_index, unpack_batches)
from .merge_tree import encode_postorder, resolve_merge_order


class BmxMnnParams(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_int32), ("k", ctypes.c_int32), ("prop_k", ctypes.c_double),
                ("sigma", ctypes.c_double), ("cos_norm_in", ctypes.c_int32), ("cos_norm_out", ctypes.c_int32),
                ("var_adj", ctypes.c_int32), ("correct_all", ctypes.c_int32), ("svd_dim", ctypes.c_int32),
                ("auto_merge", ctypes.c_int32), ("subset_row", ctypes.c_void_p), ("n_subset_row", ctypes.c_int32),
                ("tree", ctypes.c_void_p), ("tree_len", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("var_adj_strict", ctypes.c_int32)]


@dataclass
class MnnCorrectMergeInfo:
    """metadata(output)$merge.info (R/mnnCorrect.R:383-391)."""
    left: List[List[Any]]
    right: List[List[Any]]
    pairs: List[Any]          # per merge: (left, right) 1-based columns of `corrected`


@dataclass
class MnnCorrectResult:
    corrected: np.ndarray     # genes x cells, cells in the caller's order
    batch: np.ndarray         # batch id (1-based) or name per cell
    merge_info: MnnCorrectMergeInfo
    stage_ms: Optional[dict] = None  # device time over all merges by stage (bmx_mnn_result_stage_ms)
    # var_adj_strict: per merge, cells the strict pass recomputed in its two adjust_shift_variance calls -- on the input genes
    # and on the output genes ([nbatches - 1, 2]; -1: strict off, no such call, or the call did not take the tiled form)
    strict_cells: Optional[np.ndarray] = None


def _check(batches, restrict, svd_dim, auto_merge, sparse=False):
    """The argument checks of .mnn_correct; returns the restrictions as 1-based int32 indices (or None)."""
    if len(batches) < 2:
        raise ValueError("at least two batches must be specified")  # R/mnnCorrect.R:187
    if sparse:
        check_same_rows(batches)
    else:
        check_same_dim(batches, byrow=False, see_batch=True)
    restrict = restrict_list(restrict, [b.shape[1] for b in batches])
    if svd_dim and int(svd_dim) > 0:
        raise ValueError("svd.dim > 0 is not supported by mnnCorrect on the device")
    if auto_merge:
        raise ValueError("auto.merge=TRUE is not supported by mnnCorrect on the device")
    return restrict


def _csc_arrays(c):
    """Canonical CSC `c` as the library takes a batch: (indptr int64, indices int32, data float64), each contiguous."""
    return (np.ascontiguousarray(c.indptr, dtype=np.int64), np.ascontiguousarray(c.indices, dtype=np.int32),
            np.ascontiguousarray(c.data, dtype=np.float64))


def _mnn_correct(batches, restrict, k, prop_k, sigma, cos_norm_in, cos_norm_out, var_adj, subset_row, correct_all,
                 merge_order, names, device, sparse=False, var_adj_strict=False):
    """.mnn_correct (R/mnnCorrect.R:179-231) through bmx_mnn_correct, or for scipy.sparse batches through
    bmx_mnn_correct_sparse."""
    check_unique_names(names)  # R/mnnCorrect.R:222
    B = len(batches)
    G = batches[0].shape[0]
    tree = resolve_merge_order(B, merge_order, names)
    code = encode_postorder(tree)
    if sparse:
        mats = [canonical_csc(b)[0] for b in batches]  # (the caller's objects stay as they are)
        csc = [_csc_arrays(c) for c in mats]
    else:
        mats = [np.asfortranarray(b, dtype=np.float64) for b in batches]  # genes x cells, column-major: R's layout
    sub = subset_index(subset_row, G)
    _rkeep, rptr, rn = pack_restrictions(restrict, B)  # (_rkeep: what rptr points into)
    _lib.require_gpu()
    _lib.check(_lib.lib().bmx_set_device(int(device)))
    ncells = np.asarray([m.shape[1] for m in mats], dtype=np.int32)
    p = BmxMnnParams(ctypes.sizeof(BmxMnnParams), int(k), float("nan") if prop_k is None else float(prop_k), float(sigma),
                     int(bool(cos_norm_in)), int(bool(cos_norm_out)), int(bool(var_adj)), int(bool(correct_all)), 0, 0,
                     None if sub is None else sub.ctypes.data, 0 if sub is None else int(sub.size), code.ctypes.data,
                     int(code.size), 0, int(bool(var_adj_strict)))
    L = _lib.lib()
    h = ctypes.c_void_p()
    if sparse:
        indptr, indices, data = ((ctypes.c_void_p * B)(*[a[i].ctypes.data for a in csc]) for i in range(3))
        _lib.check(L.bmx_mnn_correct_sparse(ctypes.c_int32(B), ctypes.c_int32(G), indptr, indices, data, _lib.i32p(ncells),
                                            rptr, _lib.i32p(rn), ctypes.byref(p), ctypes.byref(h)))
    else:
        data = (ctypes.c_void_p * B)(*[m.ctypes.data for m in mats])
        _lib.check(L.bmx_mnn_correct(ctypes.c_int32(B), ctypes.c_int32(G), data, _lib.i32p(ncells),
                                     rptr, _lib.i32p(rn), ctypes.byref(p), ctypes.byref(h)))
    try:
        go = ctypes.c_int32(0)
        n = ctypes.c_int64(0)
        npairs = np.zeros(B - 1, dtype=np.int64)
        _lib.check(L.bmx_mnn_result_sizes(h, ctypes.byref(go), ctypes.byref(n), npairs.ctypes.data_as(_lib.c_i64p)))
        corrected = np.empty((go.value, n.value), dtype=np.float64, order="F")
        batch = np.empty(n.value, dtype=np.int32)
        ml = np.zeros((B - 1, B), dtype=np.int32)
        mr = np.zeros((B - 1, B), dtype=np.int32)
        pl = [np.empty(int(c), dtype=np.int32) for c in npairs]
        pr = [np.empty(int(c), dtype=np.int32) for c in npairs]
        lp = (ctypes.c_void_p * (B - 1))(*[a.ctypes.data for a in pl])
        rp = (ctypes.c_void_p * (B - 1))(*[a.ctypes.data for a in pr])
        _lib.check(L.bmx_mnn_result_into(h, _lib.f64p(corrected), _lib.i32p(batch), _lib.i32p(ml), _lib.i32p(mr), lp, rp))
        st = np.zeros(5, dtype=np.float64)
        _lib.check(L.bmx_mnn_result_stage_ms(h, _lib.f64p(st)))
        sc = np.full((B - 1, 2), -1, dtype=np.int64)
        _lib.check(L.bmx_mnn_result_strict_cells(h, sc.ctypes.data_as(_lib.c_i64p)))
    finally:
        L.bmx_mnn_result_free(h)
    info = MnnCorrectMergeInfo(left=[[int(x) for x in row if x] for row in ml],
                               right=[[int(x) for x in row if x] for row in mr], pairs=list(zip(pl, pr)))
    out = MnnCorrectResult(corrected=corrected, batch=batch, merge_info=info,
                           stage_ms=dict(zip(("search", "averaging", "smoothing", "asv", "apply"), st.tolist())),
                           strict_cells=sc)
    return apply_names(out, names)  # R/mnnCorrect.R:219-226


def mnnCorrect(*batches, batch=None, restrict=None, k=20, prop_k=None, sigma=0.1, cos_norm_in=True, cos_norm_out=True,
               svd_dim=0, var_adj=True, subset_row=None, correct_all=False, merge_order=None, auto_merge=False, names=None,
               device=0, var_adj_strict=False) -> MnnCorrectResult:
    """mnnCorrect(..., batch=, restrict=, k=, prop.k=, sigma=, cos.norm.in=, cos.norm.out=, svd.dim=, var.adj=,
    subset.row=, correct.all=, merge.order=, auto.merge=) (R/mnnCorrect.R:125-168).  Each batch is genes x cells; the batches
    are all dense or all scipy.sparse (implicit zeros are zeros), and the result is the same dense one either way (the
    module docstring).  var_adj_strict (with var_adj): where a call of adjust_shift_variance is large enough for the tiled
    form, the cells that form flags as ill-conditioned and cannot re-run get the reference's own chains, bit for bit."""
    if var_adj_strict and not var_adj:
        raise ValueError("'var_adj_strict' needs 'var_adj'")
    batches = unpack_batches(batches)
    sparse = all_sparse(batches, "mnnCorrect")  # (before anything is converted)
    mats = list(batches) if sparse else [np.asarray(b, dtype=np.float64) for b in batches]
    if len(mats) == 0:
        raise ValueError("at least two batches must be specified")
    if len(mats) == 1:
        if batch is None:
            raise ValueError("'batch' must be specified if '...' has only one object")  # R/checkInputs.R:128
        if np.asarray(batch).shape[0] != mats[0].shape[1]:
            raise ValueError("'length(batch)' and 'ncol(x)' are not the same")
        if restrict is not None and len(restrict) != 1:
            raise ValueError("'restrictions' must of length equal to the number of batches")
        x = canonical_csc(mats[0])[0] if sparse else mats[0]  # (a format that takes a column mask)
        div = divide_into_batches(x, batch, None if restrict is None else restrict[0])
        rparts = _check(div.parts, div.restricted, svd_dim, auto_merge, sparse)
        out = _mnn_correct(div.parts, rparts, k, prop_k, sigma, cos_norm_in, cos_norm_out, var_adj, subset_row, correct_all,
                           merge_order, [str(l) for l in div.levels], device, sparse, var_adj_strict)
        # the caller's column order (R/mnnCorrect.R:161-165)
        out.corrected = out.corrected[:, div.reorder - 1]
        out.batch = out.batch[div.reorder - 1]
        out.merge_info.pairs = reindex_pairings(out.merge_info.pairs, div.reorder)
        return out
    restrict = _check(mats, restrict, svd_dim, auto_merge, sparse)
    return _mnn_correct(mats, restrict, k, prop_k, sigma, cos_norm_in, cos_norm_out, var_adj, subset_row, correct_all,
                        merge_order, names, device, sparse, var_adj_strict)
