"""mnnCorrect() (R/mnnCorrect.R:125-168): the classic gene-space MNN correction, end to end on the device behind
bmx_mnn_correct (csrc/mnn_correct.hip).

Batches are genes x cells, as in R.  `names` plays the role of the argument names of `...`.  Out of scope here (a clear
error): svd.dim > 0, auto.merge = TRUE, sparse / SingleCellExperiment inputs.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Any, List, Optional

import numpy as np

from . import _lib
from .merge_tree import encode_postorder, resolve_merge_order


class BmxMnnParams(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_int32), ("k", ctypes.c_int32), ("prop_k", ctypes.c_double),
                ("sigma", ctypes.c_double), ("cos_norm_in", ctypes.c_int32), ("cos_norm_out", ctypes.c_int32),
                ("var_adj", ctypes.c_int32), ("correct_all", ctypes.c_int32), ("svd_dim", ctypes.c_int32),
                ("auto_merge", ctypes.c_int32), ("subset_row", ctypes.c_void_p), ("n_subset_row", ctypes.c_int32),
                ("tree", ctypes.c_void_p), ("tree_len", ctypes.c_int32)]


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


def _subset_index(subset_row, G):
    """.row_subset_to_index for integer (1-based) or logical vectors."""
    if subset_row is None:
        return None
    r = np.asarray(subset_row)
    if r.dtype == bool:
        if r.size != G:
            raise ValueError("subset indices out of range")
        return (np.flatnonzero(r) + 1).astype(np.int32)
    r = r.astype(np.int64)
    if r.size and (r.min() < 1 or r.max() > G):
        raise ValueError("subset indices out of range")
    return np.ascontiguousarray(r, dtype=np.int32)


def _check(batches, restrict, svd_dim, auto_merge):
    if len(batches) < 2:
        raise ValueError("at least two batches must be specified")  # R/mnnCorrect.R:187
    G = batches[0].shape[0]
    for i, b in enumerate(batches):
        if b.ndim != 2 or b.shape[0] != G:
            raise ValueError(f"number of rows is not the same across batches (see batch {i + 1})")  # R/checkInputs.R:64
    if restrict is not None and len(restrict) != len(batches):
        raise ValueError("'restrictions' must of length equal to the number of batches")  # R/checkInputs.R:101
    if svd_dim and int(svd_dim) > 0:
        raise ValueError("svd.dim > 0 is not supported by mnnCorrect on the device")
    if auto_merge:
        raise ValueError("auto.merge=TRUE is not supported by mnnCorrect on the device")


def _mnn_correct(batches, restrict, k, prop_k, sigma, cos_norm_in, cos_norm_out, var_adj, subset_row, correct_all,
                 merge_order, names, device):
    """.mnn_correct (R/mnnCorrect.R:179-231) through bmx_mnn_correct."""
    if names is not None and len(set(names)) != len(names):
        raise ValueError("names of batches should be unique")  # R/mnnCorrect.R:222
    B = len(batches)
    G = batches[0].shape[0]
    tree = resolve_merge_order(B, merge_order, names)
    code = encode_postorder(tree)
    mats = [np.asfortranarray(b, dtype=np.float64) for b in batches]  # genes x cells, column-major: R's layout
    sub = _subset_index(subset_row, G)
    rlist, rptr, rn = [], (ctypes.c_void_p * B)(), np.full(B, -1, dtype=np.int32)
    if restrict is not None:
        for b, r in enumerate(restrict):
            if r is None:
                continue
            r = np.asarray(r)
            r = (np.flatnonzero(r) + 1) if r.dtype == bool else r
            r = np.ascontiguousarray(r, dtype=np.int32)
            if r.size == 0:
                raise ValueError("no cells remaining in a batch after restriction")  # R/checkInputs.R:116
            rlist.append(r)
            rptr[b] = r.ctypes.data
            rn[b] = r.size
    _lib.require_gpu()
    _lib.check(_lib.lib().bmx_set_device(int(device)))
    data = (ctypes.c_void_p * B)(*[m.ctypes.data for m in mats])
    ncells = np.asarray([m.shape[1] for m in mats], dtype=np.int32)
    p = BmxMnnParams(ctypes.sizeof(BmxMnnParams), int(k), float("nan") if prop_k is None else float(prop_k), float(sigma),
                     int(bool(cos_norm_in)), int(bool(cos_norm_out)), int(bool(var_adj)), int(bool(correct_all)), 0, 0,
                     None if sub is None else sub.ctypes.data, 0 if sub is None else int(sub.size), code.ctypes.data,
                     int(code.size))
    L = _lib.lib()
    h = ctypes.c_void_p()
    _lib.check(L.bmx_mnn_correct(ctypes.c_int32(B), ctypes.c_int32(G), data, _lib.i32p(ncells),
                                 rptr if restrict is not None else None, _lib.i32p(rn), ctypes.byref(p), ctypes.byref(h)))
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
    finally:
        L.bmx_mnn_result_free(h)
    info = MnnCorrectMergeInfo(left=[[int(x) for x in row if x] for row in ml],
                               right=[[int(x) for x in row if x] for row in mr], pairs=list(zip(pl, pr)))
    out = MnnCorrectResult(corrected=corrected, batch=batch, merge_info=info,
                           stage_ms=dict(zip(("search", "averaging", "smoothing", "asv", "apply"), st.tolist())))
    if names is not None:  # R/mnnCorrect.R:219-226
        nm = np.asarray(list(names), dtype=object)
        out.batch = nm[batch - 1]
        info.left = [[names[i - 1] for i in s] for s in info.left]
        info.right = [[names[i - 1] for i in s] for s in info.right]
    return out


def mnnCorrect(*batches, batch=None, restrict=None, k=20, prop_k=None, sigma=0.1, cos_norm_in=True, cos_norm_out=True,
               svd_dim=0, var_adj=True, subset_row=None, correct_all=False, merge_order=None, auto_merge=False, names=None,
               device=0) -> MnnCorrectResult:
    """mnnCorrect(..., batch=, restrict=, k=, prop.k=, sigma=, cos.norm.in=, cos.norm.out=, svd.dim=, var.adj=,
    subset.row=, correct.all=, merge.order=, auto.merge=) (R/mnnCorrect.R:125-168).  Each batch is genes x cells."""
    if len(batches) == 1 and isinstance(batches[0], (list, tuple)):
        batches = tuple(batches[0])
    mats = [np.asarray(b, dtype=np.float64) for b in batches]
    if len(mats) == 0:
        raise ValueError("at least two batches must be specified")
    if len(mats) == 1:
        if batch is None:
            raise ValueError("'batch' must be specified if '...' has only one object")  # R/checkInputs.R:128
        x = mats[0]
        batch = np.asarray(batch)
        if batch.shape[0] != x.shape[1]:
            raise ValueError("'length(batch)' and 'ncol(x)' are not the same")
        if restrict is not None and len(restrict) != 1:
            raise ValueError("'restrictions' must of length equal to the number of batches")
        # divideIntoBatches (R/divideIntoBatches.R:36-84) by column: levels are the sorted unique values
        levels = sorted(set(batch.tolist()))
        mask = None
        if restrict is not None:
            r = np.asarray(restrict[0])
            mask = np.zeros(x.shape[1], dtype=bool)
            if r.dtype == bool:
                mask[:] = r
            else:
                mask[r.astype(np.int64) - 1] = True
        parts, rparts = [], ([] if mask is not None else None)
        reorder = np.zeros(x.shape[1], dtype=np.int64)
        last = 0
        for lev in levels:
            keep = batch == lev
            parts.append(x[:, keep])
            if mask is not None:
                cr = np.flatnonzero(mask[keep]) + 1
                if cr.size == 0:
                    raise ValueError("no cells remaining in a batch after restriction")
                rparts.append(cr.astype(np.int32))
            reorder[keep] = last + np.arange(1, int(keep.sum()) + 1)
            last += int(keep.sum())
        _check(parts, rparts, svd_dim, auto_merge)
        out = _mnn_correct(parts, rparts, k, prop_k, sigma, cos_norm_in, cos_norm_out, var_adj, subset_row, correct_all,
                           merge_order, [str(l) for l in levels], device)
        # the caller's column order (R/mnnCorrect.R:161-165)
        out.corrected = out.corrected[:, reorder - 1]
        out.batch = out.batch[reorder - 1]
        rev = np.zeros(reorder.size + 1, dtype=np.int64)
        rev[reorder] = np.arange(1, reorder.size + 1)
        out.merge_info.pairs = [(rev[l], rev[r]) for l, r in out.merge_info.pairs]
        return out
    _check(mats, restrict, svd_dim, auto_merge)
    return _mnn_correct(mats, restrict, k, prop_k, sigma, cos_norm_in, cos_norm_out, var_adj, subset_row, correct_all,
                        merge_order, names, device)
