"""What every front end does to its arguments before any arithmetic: R/checkInputs.R, R/divideIntoBatches.R and
R/utils_reorder.R, once.  Conventions follow R: 1-based indices, `None` for NULL, levels in sorted order.  Nothing here
needs the library or a device.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional

import numpy as np
import scipy.sparse as sp


def unpack_batches(batches):
    """`f(a, b)` and `f([a, b])` name the same batches."""
    if len(batches) == 1 and isinstance(batches[0], (list, tuple)):
        return tuple(batches[0])
    return tuple(batches)


def check_same_dim(mats, byrow, see_batch=False):
    """checkBatchConsistency (R/checkInputs.R:64-71): batches of cells x dims (byrow) agree in their columns, batches of
    genes x cells in their rows.  Returns that number."""
    axis, what = (1, "columns") if byrow else (0, "rows")
    first = np.asarray(mats[0])
    dim = first.shape[axis] if first.ndim == 2 else -1
    for i, m in enumerate(mats):
        m = np.asarray(m)
        if m.ndim != 2 or m.shape[axis] != dim:
            raise ValueError(f"number of {what} is not the same across batches" + (f" (see batch {i + 1})" if see_batch else ""))
    return dim


def all_sparse(batches, who):
    """Whether the batches are scipy.sparse objects: all of them (True) or none (False); a mixture is refused."""
    flags = [sp.issparse(b) for b in batches]
    if any(flags) and not all(flags):
        raise TypeError(f"{who} takes batches that are all sparse or all dense, not a mixture")
    return len(flags) > 0 and all(flags)


def check_same_rows(mats):
    """check_same_dim(byrow=False) for scipy.sparse batches."""
    for m in mats:
        if m.ndim != 2 or m.shape[0] != mats[0].shape[0]:
            raise ValueError("number of rows is not the same across batches")
    return mats[0].shape[0]


def canonical_csc(m):
    """A scipy.sparse matrix or array of any format as canonical CSC: duplicates summed, rows ascending within a column,
    float64 data, int32 indices; stored zeros stay.  Returns (csc, owned): the caller's object is never modified, and
    `owned` is False when the result still shares its index arrays with it."""
    c = m.tocsc()
    owned = c is not m
    if not c.has_canonical_format:
        if not owned:
            c, owned = c.copy(), True
        c.sum_duplicates()  # (sorts the indices first)
    if c.data.dtype != np.float64:
        c = sp.csc_matrix((c.data.astype(np.float64), c.indices, c.indptr), shape=c.shape)
    if c.indices.dtype != np.int32:
        c = sp.csc_matrix((c.data, c.indices.astype(np.int32), c.indptr), shape=c.shape)
        owned = True
    return c, owned


def csc_blocks(c, width):
    """The column blocks of canonical CSC `c`, `width` cells each (the last one fewer), as the library takes them:
    (cells, indptr relative to the block as int64, indices, data)."""
    n = c.shape[1]
    for a in range(0, n, width):
        b = min(n, a + width)
        k0, k1 = int(c.indptr[a]), int(c.indptr[b])
        yield b - a, c.indptr[a:b + 1].astype(np.int64) - k0, c.indices[k0:k1], c.data[k0:k1]


def csc_block_width(c, block_bytes):
    """Cells per column block of `c` that hold about block_bytes of stored entries (12 bytes each) at its mean density."""
    return max(1, int(block_bytes) * int(c.shape[1]) // max(1, 12 * int(c.nnz)))


def check_unique_names(names):
    if names is not None and len(set(names)) != len(names):
        raise ValueError("names of batches should be unique")  # R/fastMNN.R:422


def subset_index(subset_row, G):
    """.row_subset_to_index for integer (1-based) or logical vectors: 1-based int32, None for NULL."""
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


def restrict_index(restrict, n):
    """One batch's restrict (1-based positions or a logical mask over its n cells) as 1-based int32 positions; None = all
    cells."""
    if restrict is None:
        return None
    r = np.asarray(restrict)
    if r.dtype == bool:
        if r.size != n:
            raise ValueError("'restrict' indices out of range")
        r = np.flatnonzero(r) + 1
    r = np.ascontiguousarray(r, dtype=np.int64)
    if r.size == 0:
        raise ValueError("no cells remaining in a batch after restriction")  # R/checkInputs.R:116
    if r.min() < 1 or r.max() > n:
        raise ValueError("'restrict' indices out of range")
    return r.astype(np.int32)


def check_restrict_length(restrict, nbatches):
    if restrict is not None and len(restrict) != nbatches:
        raise ValueError("'restrictions' must of length equal to the number of batches")  # R/checkInputs.R:101


def restrict_list(restrict, ncells):
    """checkRestrictions (R/checkInputs.R:95-121): one restrict_index per batch, or None when there is no restriction."""
    check_restrict_length(restrict, len(ncells))
    return None if restrict is None else [restrict_index(r, n) for r, n in zip(restrict, ncells)]


def pack_restrictions(rlist, nbatches):
    """A restrict_list for the C ABI: (keepalive, void* [B] or None, int32 n [B]); a batch without a restriction has a null
    pointer and n = -1.  The pointers are into the arrays of `keepalive`, which the caller holds while the library reads."""
    counts = np.full(nbatches, -1, dtype=np.int32)
    if rlist is None:
        return [], None, counts
    keep = [None if r is None else np.ascontiguousarray(r, dtype=np.int32) for r in rlist]
    ptrs = (ctypes.c_void_p * nbatches)()
    for b, r in enumerate(keep):
        if r is not None:
            ptrs[b] = r.ctypes.data
            counts[b] = r.size
    return keep, ptrs, counts


class Divided(NamedTuple):
    parts: list                 # x split by level, in the order of `levels`
    restricted: Optional[list]  # per part: 1-based int32 positions within the part; None without a restriction
    levels: list                # sorted unique values of `batch`
    reorder: np.ndarray         # concatenate(parts)[reorder - 1] is x again (1-based)
    also: list                  # for every vector of `also`: its pieces, part by part


def divide_into_batches(x, batch, restrict=None, byrow=False, also=()):
    """divideIntoBatches (R/divideIntoBatches.R:36-84): the cells of x (its rows if byrow, else its columns) split by the
    levels of factor(batch).  `restrict` is ONE batch's restriction over the cells of x; `also` holds further per-cell
    vectors that are split alongside."""
    batch = np.asarray(batch)
    n = x.shape[0 if byrow else 1]
    if batch.ndim != 1 or batch.shape[0] != n:
        raise ValueError(f"'length(batch)' and '{'nrow' if byrow else 'ncol'}(x)' are not the same")  # :41, :50
    levels = sorted(set(batch.tolist()))
    mask = None
    if restrict is not None:
        mask = np.zeros(n, dtype=bool)
        mask[restrict_index(restrict, n) - 1] = True
    parts, restricted, extra = [], (None if mask is None else []), [[] for _ in also]
    reorder = np.zeros(n, dtype=np.int64)
    last = 0
    for lev in levels:
        keep = batch == lev
        parts.append(x[keep] if byrow else x[:, keep])
        for pieces, v in zip(extra, also):
            pieces.append(v[keep])
        if mask is not None:
            cur = np.flatnonzero(mask[keep]) + 1
            if cur.size == 0:
                raise ValueError("no cells remaining in a batch after restriction")  # :71-73
            restricted.append(cur.astype(np.int32))
        count = int(keep.sum())
        reorder[keep] = last + np.arange(1, count + 1)
        last += count
    return Divided(parts, restricted, levels, reorder, extra)


def reindex_pairings(pairings, new_order):
    """R/utils_reorder.R:23-36: pairs that index the divided cells, in the caller's order."""
    new_order = np.asarray(new_order, dtype=np.int64)
    rev = np.zeros(new_order.size + 1, dtype=np.int64)
    rev[new_order] = np.arange(1, new_order.size + 1)
    return [(rev[l], rev[r]) for l, r in pairings]


def apply_names(out, names):
    """Batch ids to the names of `...` in a result's `batch` and `merge_info.left` / `right` (R/fastMNN.R:419-427)."""
    if names is None:
        return out
    nm = np.asarray(list(names), dtype=object)
    out.batch = nm[out.batch - 1]
    out.merge_info.left = [[names[i - 1] for i in s] for s in out.merge_info.left]
    out.merge_info.right = [[names[i - 1] for i in s] for s in out.merge_info.right]
    return out
