"""CPU restatement of mnnCorrect() (R/mnnCorrect.R:170-481), line by line, from oracle.fastmnn_oracle's primitives.
A helper module of the mnnCorrect tests (not a conftest).  Batches are genes x cells, indices 1-based, None = NULL.
Group order of the averaging: ascending right-cell index (sumCountsAcrossCells' factor levels)."""
from __future__ import annotations

import numpy as np

from oracle import fastmnn_oracle as orc


def cosine_norm(x):
    """cosineNorm(x, mode="all") (R/cosineNorm.R:63-82): columns over pmax(1e-8, l2)."""
    l2 = np.sqrt((x * x).sum(axis=0))
    return x / np.maximum(l2, 1e-8), l2


def prepare_input_data(batches, cos_norm_in, cos_norm_out, subset_row, correct_all):
    """.prepare_input_data (R/mnnCorrect.R:398-445)."""
    in_b = list(batches)
    out_b = list(batches)
    same = True
    if subset_row is not None:  # :404-415
        subset_row = np.asarray(subset_row, dtype=np.int64)
        if np.array_equal(subset_row, np.arange(1, batches[0].shape[0] + 1)):
            subset_row = None
        else:
            in_b = [b[subset_row - 1] for b in in_b]
            if correct_all:
                same = False
            else:
                out_b = in_b
    scaling = None
    if cos_norm_in:  # :419-427
        res = [cosine_norm(b) for b in in_b]
        in_b = [r[0] for r in res]
        scaling = [r[1] for r in res]
    if cos_norm_out:  # :428-433
        if not cos_norm_in:
            scaling = [cosine_norm(b)[1] for b in in_b]
        out_b = [b / np.maximum(l2, 1e-8) for b, l2 in zip(out_b, scaling)]
    if bool(cos_norm_out) != bool(cos_norm_in):  # :435-437
        same = False
    return in_b, out_b, subset_row, same


def average_vectors(data1, data2, mnn1, mnn2):
    """sumCountsAcrossCells(t(vect), DataFrame(ID=mnn2), average=TRUE) (R/mnnCorrect.R:454-455): groups ascending, each
    group's rows added in pair order, then divided by their number."""
    vect = data1[np.asarray(mnn1) - 1] - data2[np.asarray(mnn2) - 1]
    ids, inv = np.unique(mnn2, return_inverse=True)
    summed = np.zeros((ids.size, vect.shape[1]))
    np.add.at(summed, inv, vect)
    return summed / np.bincount(inv)[:, None], ids


def compute_correction_vectors(data1, data2, mnn1, mnn2, tdata2, sigma):
    """.compute_correction_vectors (R/mnnCorrect.R:451-460); data rows are cells, tdata2 genes x cells."""
    averaged, ids = average_vectors(data1, data2, mnn1, mnn2)
    cell_vect = orc.smooth_gaussian_kernel(averaged.T, ids - 1, tdata2, sigma)
    return np.ascontiguousarray(cell_vect.T)


def adjust_shift_variance(data1, data2, correction, sigma, subset_row=None, restrict1=None, restrict2=None, cells=None):
    """.adjust_shift_variance (R/mnnCorrect.R:462-481); data1 / data2 genes x cells, correction cells x genes.
    `cells` (0-based): the scaling of those cells only (the reference's loop treats every cell on its own); the other rows
    come out NaN."""
    cell_vect = correction
    if subset_row is not None:
        cell_vect = cell_vect[:, subset_row - 1]
        data1 = data1[subset_row - 1]
        data2 = data2[subset_row - 1]
    r1 = (np.arange(data1.shape[1]) if restrict1 is None else np.asarray(restrict1) - 1).astype(np.int32)
    r2 = (np.arange(data2.shape[1]) if restrict2 is None else np.asarray(restrict2) - 1).astype(np.int32)
    if cells is None:
        scaling = orc.adjust_shift_variance(data1, data2, cell_vect, sigma, r1, r2)
    else:
        scaling = np.full(data2.shape[1], np.nan)
        scaling[cells] = orc.adjust_shift_variance(data1, data2, cell_vect, sigma, r1, r2, cells=cells)
    return np.maximum(scaling, 1)[:, None] * correction


def _set_extras(tree, out_b):
    if isinstance(tree, list):
        for ch in tree:
            _set_extras(ch, out_b)
    else:
        tree.extras = [None if out_b is None else out_b[tree.index[0] - 1]]


def mnn_correct(*batches, k=20, prop_k=None, sigma=0.1, cos_norm_in=True, cos_norm_out=True, var_adj=True,
                subset_row=None, correct_all=False, restrict=None, merge_order=None, names=None, nthreads=0, asv_cells=None):
    """.mnn_correct + .mnn_correct_core (R/mnnCorrect.R:179-393) with a predefined tree and svd.dim = 0.
    asv_cells (two batches only, 0-based cells of the right batch): adjust_shift_variance on those cells alone, the other
    right cells come out NaN -- a sample of the reference's per-cell loop at sizes where all of it would take too long."""
    if asv_cells is not None and len(batches) != 2:
        raise ValueError("asv_cells samples the one merge of two batches")
    batches = [np.asarray(b, dtype=np.float64) for b in batches]
    if len(batches) < 2:
        raise ValueError("at least two batches must be specified")
    in_b, out_b, subset_row, same = prepare_input_data(batches, cos_norm_in, cos_norm_out, subset_row, correct_all)
    in_b = [np.ascontiguousarray(b.T) for b in in_b]  # :197-200
    if not same:
        out_b = [np.ascontiguousarray(b.T) for b in out_b]
    tree = orc.create_tree_predefined(in_b, restrict, merge_order, names)  # :204
    _set_extras(tree, None if same else out_b)  # :209
    nm = len(batches) - 1
    pairings, left_set, right_set = [], [], []
    for _ in range(nm):  # :258
        left, right, path = orc.get_next_merge(tree)
        ld, rd = left.data, right.data
        s1, s2 = orc.restricted_mnn(ld, left.restrict, rd, right.restrict, k, prop_k, nthreads)  # :290-293
        pairings.append((s1, s2))
        left_set.append(list(left.index))
        right_set.append(list(right.index))
        trans_right = np.asfortranarray(rd.T)
        corr_in = compute_correction_vectors(ld, rd, s1, s2, trans_right, sigma)  # :300
        if not same:
            corr_out = compute_correction_vectors(left.extras[0], right.extras[0], s1, s2, trans_right, sigma)  # :305
        if var_adj:  # :333-342
            corr_in = adjust_shift_variance(ld.T, rd.T, corr_in, sigma, None, left.restrict, right.restrict, asv_cells)
            if not same:
                corr_out = adjust_shift_variance(left.extras[0].T, right.extras[0].T, corr_out, sigma, subset_row,
                                                 left.restrict, right.restrict, asv_cells)
        rd = rd + corr_in  # :345
        rx = None
        if not same:
            rx = right.extras[0] + corr_out
        node = orc.TreeNode(index=list(left.index) + list(right.index), data=np.vstack([ld, rd]),
                            restrict=orc.combine_restrict(ld, left.restrict, rd, right.restrict),
                            origin=np.concatenate([left.origin, right.origin]),
                            extras=[None if same else np.vstack([left.extras[0], rx])])
        tree = orc.update_tree(tree, path, node)  # :352-357
    full_order = list(tree.index)
    full_origin = np.asarray(tree.origin)
    full_data = tree.data if same else tree.extras[0]
    for m in range(nm):  # :365-370
        b1 = int(np.flatnonzero(full_origin == left_set[m][0])[0])
        b2 = int(np.flatnonzero(full_origin == right_set[m][0])[0])
        pairings[m] = (pairings[m][0] + b1, pairings[m][1] + b2)
    if any(full_order[i] > full_order[i + 1] for i in range(len(full_order) - 1)):  # :373-379
        ncells = np.bincount(full_origin, minlength=len(batches) + 1)[1:]
        ordering = orc.restore_original_order(full_order, ncells)
        full_data = full_data[ordering - 1]
        full_origin = full_origin[ordering - 1]
        pairings = orc.reindex_pairings(pairings, ordering)
    out = {"corrected": full_data.T, "batch": full_origin, "left": left_set, "right": right_set, "pairs": pairings}
    if names is not None:  # :219-226
        nmv = np.asarray(list(names), dtype=object)
        out["batch"] = nmv[full_origin - 1]
        out["left"] = [[names[i - 1] for i in s] for s in left_set]
        out["right"] = [[names[i - 1] for i in s] for s in right_set]
    return out
