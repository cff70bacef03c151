"""What multiBatchPCA on scipy.sparse batches (csrc/pca_sparse.hip, DeviceSparsePCA) is held to in
tests/test_cpu_pca_sparse.py and tests/test_gpu_pca_sparse.py.  A helper module (not a conftest); it builds the sparse cases
and hands their dense equivalents to the exact / allowance machinery of tests/pca_ref.py (Ritz identity, R^T R = I,
projection identity, centres, residual) and tests/pca_genes_ref.py (leftover rotation rows, their centres, var_total).
Those identities hold for whatever a fit returned, so they need no sign alignment and no spectral gap, and the allowances
bound a dense sum in any order: a sparse sum leaves the zero terms out, has fewer roundings and stays inside them.

`sparse_f64` restates the sparse algorithm in float64 -- rows [subset; left], the cut at n_rows_pca, norms over the
prefix, by-cell and by-gene products on the stored entries, the per-gene centred form of var_total -- with one planted
fault on request; tests/test_cpu_pca_sparse.py shows that it meets the allowances on every case and that each fault is
far outside them.
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp

from tests import pca_genes_ref, pca_ref

TOL = pca_ref.TOL


class Case:
    """twice: the subset names one row twice (nS - 1 different rows).  f64_iters: the plain steps that take the float64
    restatement of a converged case below TOL (None: pca_ref.F64_ITERS_CONVERGED).  signal: factor on the low-rank part.
    empty_prefix: the batch of that index stores nothing in the PCA rows (every entry lies in a leftover row)."""

    def __init__(self, G_all, nS, sizes, d, density, weights=None, cos_norm=False, iters=None, seed=0, twice=True,
                 f64_iters=None, signal=1.0, empty_prefix=None):
        self.G_all, self.nS, self.sizes, self.d, self.density = G_all, nS, sizes, d, density
        self.weights, self.cos_norm, self.iters, self.seed = weights, cos_norm, iters, seed
        self.twice, self.f64_iters, self.signal, self.empty_prefix = twice, f64_iters, signal, empty_prefix

    def kwargs(self):
        return {"d": self.d, "weights": self.weights, "cos_norm": self.cos_norm}


# PCA rows: 65 and 130 (a ragged last tile of 64 genes in the dense blocks); batches of 67, 200 and 513 cells (513 > twice
# the row segment of 256: the full row below has three segments, the last of one entry); d = 5 (block of 64) and 60 (block
# of 128); densities 0.05 and 0.3.  nS < G_all: an unordered subset with one row named twice and the other rows
# resident behind it (66 rows of which 65 differ: one more than the block, so that the data keeps the block's rank).
# Tree weights [[1, 2], 3] are (1/4, 1/4, 1/2).
TREE = [[1, 2], 3]
CASES = {
    "g65-d5-i2":            Case(65, None, (67, 200, 513), 5, 0.3, iters=2),
    "g130-d60-cos-w-i2":    Case(130, None, (67, 200, 513), 60, 0.05, weights=(1.0, 3.0, 0.5), cos_norm=True, iters=2),
    "g130-d5-cos-tree":     Case(130, None, (67, 200, 513), 5, 0.3, weights=TREE, cos_norm=True),
    "g65-d5-conv":          Case(65, None, (200, 513), 5, 0.05),
    "sub66of90-d5-cos-i2":  Case(90, 66, (67, 200, 513), 5, 0.3, cos_norm=True, iters=2),
    "sub130of150-d60-w":    Case(150, 130, (200, 513), 60, 0.3, weights=(2.0, 1.0)),
}

# Beyond one tile of the counting sort (GT = 4096 rows), one row a thread of the row scan (1024), one 64-entry pass of a
# column's prefix, one block of mu_dot (256 rows) and one split of the Gram products (512 rows); what each case reaches
# is asserted from its pattern in tests/test_cpu_pca_sparse.py::test_edge_cases_reach_their_branches.  (257, 512, 513)
# cells: the full row has exactly SEG, 2 SEG and 2 SEG + 1 entries, batch 0 having the empty cell.
# One step (-i1): Q is still the random start block, so a fault that zeroes whole rows of the by-gene product shows at
# full size; after two steps such rows are zero in Q as well, R is supported on the surviving rows and R^T M R = diag(s^2)
# holds to rounding (test_rows_lost_by_gene_show_after_one_step_only).  A one-step case names no subset row twice: R = Q V
# still carries the random start block, the two copies of a row differ, and the assembly over all rows keeps the later.
SEG, TILE = 256, 4096     # entries a row segment holds; rows a tile of the counting sort holds
EDGE_CASES = {
    "g65-d5-i1":             Case(65, None, (67, 200, 513), 5, 0.3, iters=1),
    "g1025-d60-cos-w-i1":    Case(1025, None, (257, 512), 60, 0.1, weights=(1.0, 3.0), cos_norm=True, iters=1),
    "g4097-i1":              Case(4097, None, (257, 513), 5, 0.1, iters=1),
    "g4300-i1":              Case(4300, None, (257, 512, 513), 5, 0.1, iters=1),
    "g4300-i2":              Case(4300, None, (257, 512, 513), 5, 0.1, iters=2),
    # density 0.1 leaves 40 plain steps at residual 2e-6 (the mask's noise fills the block); at 0.9 the restatement is at
    # 2.6e-8 after 12 steps and falls by 0.28 a step: 16 steps, 1.4e-10
    "g4300-conv":            Case(4300, None, (257, 513), 5, 0.9, f64_iters=16),
    "sub130of4300-i2":       Case(4300, 130, (257, 513), 5, 0.3, iters=2),
    "sub4200of8300-cos-i2":  Case(8300, 4200, (257, 513), 5, 0.03, cos_norm=True, iters=2),
    "sub4200of8300-i1":      Case(8300, 4200, (257, 513), 5, 0.03, iters=1, twice=False),
    # a third batch with nothing stored in the PCA rows: its cuts are the columns' starts, it has no segment in the PCA
    # rows, and under cos_norm every one of its scales is 1e8
    "sub130of4300-empty-i2":     Case(4300, 130, (257, 513, 150), 5, 0.3, iters=2, empty_prefix=2),
    "sub130of4300-empty-cos-i2": Case(4300, 130, (257, 513, 150), 5, 0.3, cos_norm=True, iters=2, empty_prefix=2),
}
EDGE = list(EDGE_CASES)
TWO_TILES = ["g4097-i1", "g4300-i1", "g4300-i2", "g4300-conv"]
CASES.update(EDGE_CASES)
FIXED = [k for k, c in CASES.items() if c.iters is not None]
CONVERGED = [k for k, c in CASES.items() if c.iters is None]
SUBSETS = [k for k, c in CASES.items() if c.nS is not None]
EMPTY_CELL = (0, 3)     # (batch, cell): no stored entry at all (scale 1e8 under cos_norm)
ZERO_ROW, FULL_ROW = 7, 11   # 0-based rows of the PCA rows' source: never stored / stored in every cell of every batch


def weight_vector(c):
    """A case's weights as the vector pca_ref takes (the tree form resolved)."""
    return (0.25, 0.25, 0.5) if c.weights is TREE else c.weights


@functools.lru_cache(maxsize=None)
def case(name):
    """(Case, CSC batches over all G_all rows, subset1 or None).  Non-negative log-count-like values: a low-rank
    non-negative signal plus noise where a Bernoulli(density) mask stores an entry, zero elsewhere."""
    c = CASES[name]
    rng = np.random.default_rng([c.G_all, c.d, sum(c.sizes), c.seed, int(c.density * 100)])
    subset1 = None
    if c.nS is not None:
        if c.twice:
            subset1 = rng.permutation(c.G_all)[:c.nS - 1] + 1
            subset1 = np.concatenate([subset1, subset1[3:4]])   # one row named twice
        else:
            subset1 = rng.permutation(c.G_all)[:c.nS] + 1
        assert np.any(np.diff(subset1) < 0)
        subset1.setflags(write=False)
    src = np.arange(c.G_all) if subset1 is None else subset1 - 1
    zero_row, full_row = int(src[ZERO_ROW]), int(src[FULL_ROW])
    rank = 8
    load = np.abs(rng.standard_normal((c.G_all, rank))) * np.linspace(2.0, 0.5, rank) * c.signal
    out = []
    for i, n in enumerate(c.sizes):
        x = load @ np.abs(rng.standard_normal((rank, n))) + 0.3 * np.abs(rng.standard_normal((c.G_all, n))) + 0.1 * i
        mask = rng.random((c.G_all, n)) < c.density
        mask[full_row] = True
        mask[zero_row] = False
        if i == EMPTY_CELL[0]:
            mask[:, EMPTY_CELL[1]] = False
            mask[full_row, EMPTY_CELL[1]] = False
        if i == c.empty_prefix:
            mask[src] = False
        m = sp.csc_matrix(np.where(mask, np.log2(1.0 + x), 0.0))
        assert m.has_canonical_format and m.indices.dtype == np.int32
        out.append(m)
    return c, out, subset1


def dense_pca_rows(name):
    """The dense batches restricted to the rows the PCA runs on, in its order."""
    c, B, subset1 = case(name)
    return [m.toarray() if subset1 is None else m.toarray()[subset1 - 1] for m in B]


@functools.lru_cache(maxsize=None)
def reference(name):
    """(pca_ref.exact, pca_ref.allowances) over the PCA rows."""
    c = CASES[name]
    ex = pca_ref.exact(dense_pca_rows(name), weight_vector(c), c.cos_norm)
    return ex, pca_ref.allowances(ex)


@functools.lru_cache(maxsize=None)
def genes_reference(name):
    """pca_genes_ref.exact over all rows (cases with a subset)."""
    c, B, subset1 = case(name)
    return pca_genes_ref.exact([m.toarray() for m in B], subset1, weight_vector(c), c.cos_norm)


def subset_fit(fit, name):
    """The PCA rows' part of a record over all rows, in the subset's order (a row named twice: both copies)."""
    c, B, subset1 = case(name)
    if subset1 is None or fit["rotation"].shape[0] == subset1.size:
        return fit
    out = dict(fit)
    out["rotation"], out["centers"] = fit["rotation"][subset1 - 1], fit["centers"][subset1 - 1]
    return out


def all_ratios(name, fit, tol=None):
    """error / allowance of everything a record of multiBatchPCA(get_all_genes, get_variance) on case `name` claims."""
    ex, al = reference(name)
    fs = subset_fit(fit, name)
    out = dict(pca_ref.fit_ratios(ex, al, fs))
    out["projection"] = pca_ref.projection_ratio(ex, al, fs)
    if tol is not None:
        r = pca_ref.residual_ratios(ex, al, fs, tol)
        out["over_tol"], out["reported_off"] = r["over_tol"], r["reported_off"]
    if CASES[name].nS is not None and "var_total" in fit:
        # pca_genes_ref.ratios term by term (its shape check does not expect a row named twice)
        gx, LD = genes_reference(name), pca_ref.LD
        assert fit["rotation"].shape == (CASES[name].G_all, len(fit["d"]))
        out["rotation_left"] = pca_ref.worst(np.asarray(fit["rotation"][gx.left], dtype=LD) - gx.rotation_left(fit),
                                             gx.rotation_left_allow(fit))
        out["centers_left"] = pca_ref.worst(np.asarray(fit["centers"][gx.left], dtype=LD) - gx.centers_left(),
                                            gx.centers_left_allow())
        allow = gx.var_total_allow(fit)
        out["var_total"] = float(abs(LD(fit["var_total"]) - gx.var_total(fit)) / allow)
        out["explained_over_total"] = float(max(LD(0), LD(np.sum(fit["var_explained"])) - LD(fit["var_total"])) / allow)
    return out


# ---------------------------------------------------------------------------------------------- float64 restatement
FAULTS = ("drop_last_entry", "cut_at_n_rows", "no_zero_term", "scale_all_rows",
          # edge-shaped: what a kernel that mishandles a tile, a lane stride or a segment boundary would do
          "tile_rows_lost_by_gene",     # the by-gene product (not the centres) loses every row >= TILE
          "first_row_of_tile_entry",    # the by-gene product loses one entry of row TILE
          "entry_65_by_cell",           # the by-cell product loses the 65th entry of one column's prefix
          "cut_at_tile_edge",           # the prefix (product and norm) ends at the last tile edge below n_rows_pca
          "third_segment")              # a row of exactly 2 SEG entries loses its second segment in the by-gene product


def rows_first(m, subset1, get_all=True):
    """[x[subset]; the other rows, ascending] of a CSC batch, and the number of PCA rows."""
    if subset1 is None:
        return m, m.shape[0]
    sub, left = pca_genes_ref.split_rows(m.shape[0], subset1)
    order = np.concatenate([sub, left]) if get_all else sub
    out = m[order].tocsc()
    out.sort_indices()
    return out, sub.size


def sparse_f64(name, iters, fault=None, seed=0):
    """multiBatchPCA on case `name` as the sparse handle does it, float64 on the stored entries, `iters` plain subspace
    steps: a record over all rows with "pcs", "var_total", "var_explained", "residual".  `fault`: one of FAULTS."""
    assert fault is None or fault in FAULTS
    c, B, subset1 = case(name)
    w = pca_ref.weight_vector(c.sizes, weight_vector(c))
    mats, Gp = zip(*[rows_first(m, subset1) for m in B])
    Gp, G = Gp[0], mats[0].shape[0]
    L = pca_ref.width(c.d)
    cells, rowsP, by_gene, scaled = [], [], [], []
    for m in mats:
        pre = m[:Gp].tocsc()                                      # the PCA prefix of every column
        if fault == "cut_at_tile_edge":
            assert Gp % TILE not in (0, Gp)
            pre = sp.vstack([m[:Gp - Gp % TILE], sp.csr_matrix((Gp % TILE, m.shape[1]))]).tocsc()
        over = m if fault == "scale_all_rows" else pre
        l2 = np.sqrt(np.asarray(over.multiply(over).sum(axis=0)).ravel())
        inv = 1.0 / np.maximum(1e-8, l2) if c.cos_norm else np.ones(m.shape[1])
        by_cell = pre.copy()
        if fault == "drop_last_entry":                            # the last stored entry of the last non-empty column
            col = np.flatnonzero(np.diff(by_cell.indptr))[-1]
            by_cell.data[by_cell.indptr[col + 1] - 1] = 0.0
        if fault == "cut_at_n_rows" and G > Gp:                   # the leftover rows read on into the block (wrapped)
            wrap = sp.csr_matrix((np.ones(G - Gp), (np.arange(G - Gp), np.arange(G - Gp) % Gp)), shape=(G - Gp, Gp))
            by_cell = (pre + (wrap.T @ m[Gp:]).tocsc()).tocsc()
        if fault == "entry_65_by_cell" and len(cells) == 0:       # (batch 0) the first column with 65 entries or more
            col = np.flatnonzero(np.diff(by_cell.indptr) >= 65)[0]
            by_cell.data[by_cell.indptr[col] + 64] = 0.0
        comp = (m @ sp.diags(inv)).tocsr()                        # the companion: scaled values by row
        gene = comp[:Gp].copy()                                   # what the by-gene product reads of the companion
        if fault == "first_row_of_tile_entry" and len(cells) == 0:
            assert gene.indptr[TILE + 1] > gene.indptr[TILE]
            gene.data[gene.indptr[TILE]] = 0.0
        if fault == "third_segment":
            for g in np.flatnonzero(np.diff(gene.indptr) == 2 * SEG):
                gene.data[gene.indptr[g] + SEG:gene.indptr[g + 1]] = 0.0
        cells.append((by_cell, inv))
        rowsP.append(comp[:Gp])
        by_gene.append(gene)
        scaled.append(comp)
    mu = np.zeros(G)
    for wb, s in zip(w, scaled):
        mu += (wb / w.sum()) * (np.asarray(s.sum(axis=1)).ravel() / s.shape[1])
    muP = mu[:Gp]
    coef = [wb / m.shape[1] for wb, m in zip(w, mats)]

    def project(i, Q):
        x, inv = cells[i]
        return inv[:, None] * (x.T @ Q) - (muP @ Q)[None, :]

    def apply(Q):
        Y = np.zeros_like(Q)
        for i in range(len(mats)):
            Z = project(i, Q)
            Y += coef[i] * (by_gene[i] @ Z - np.outer(muP, Z.sum(axis=0)))
        if fault == "tile_rows_lost_by_gene":
            assert Gp > TILE
            Y[TILE:] = 0.0
        return Y

    Q = np.linalg.qr(np.random.default_rng(seed).standard_normal((Gp, L)))[0]
    for it in range(iters):
        Y = apply(Q)
        if it + 1 < iters:
            Q = np.linalg.qr(Y)[0]
    T = Q.T @ Y
    theta, V = np.linalg.eigh(0.5 * (T + T.T))
    order = np.argsort(theta)[::-1]
    theta, V = theta[order], V[:, order]
    Xr, Yr = Q @ V, Y @ V
    R, s = np.ascontiguousarray(Xr[:, :c.d]), np.sqrt(np.maximum(theta[:c.d], 0.0))
    D = Yr[:, :c.d] - Xr[:, :c.d] * theta[None, :c.d]
    pcs = [project(i, R) for i in range(len(mats))]
    rec = {"rotation": R, "centers": muP.copy(), "d": s, "pcs": pcs,
           "residual": float(np.sqrt((D * D).sum(axis=0)).max() / theta[0]), "var_explained": s ** 2 / len(mats)}
    total = 0.0
    for i, rp in enumerate(rowsP):                                # per gene, centred: stored entries, then the zeros
        cen = sp.csr_matrix((rp.data - np.repeat(muP, np.diff(rp.indptr)), rp.indices, rp.indptr), shape=rp.shape)
        per = np.asarray(cen.multiply(cen).sum(axis=1)).ravel()
        if fault != "no_zero_term":
            per += (rp.shape[1] - np.diff(rp.indptr)) * muP ** 2
        total += coef[i] * per.sum()
    rec["var_total"] = total / len(mats)
    if G > Gp:
        A = sum(coef[i] * (scaled[i][Gp:] @ pcs[i]) for i in range(len(mats)))
        t = sum(coef[i] * pcs[i].sum(axis=0) for i in range(len(mats)))
        sub, left = pca_genes_ref.split_rows(c.G_all, subset1)
        rot, cen = np.zeros((c.G_all, c.d)), np.zeros(c.G_all)
        rot[sub], cen[sub] = R, muP
        rot[left], cen[left] = (A - np.outer(mu[Gp:], t)) / (s ** 2)[None, :], mu[Gp:]
        rec["rotation"], rec["centers"] = rot, cen
    return rec


# ---------------------------------------------------------------------------------------------- fastMNN input
def planted_sparse(seed=3, G=130, sizes=(150, 170), d=5, density=0.3):
    """Sparse batches in the style of pca_genes_ref.planted_case: d non-negative directions of strengths 12, 10, 8, ...
    over a little noise, stored where a Bernoulli(density) mask per entry allows.  The directions are strong enough that
    the top d singular values of the masked data stay separated from each other and from the rest by a large fraction
    of themselves, so two converged PCAs span the same subspace to rounding."""
    rng = np.random.default_rng([seed, G])
    dirs = np.abs(np.linalg.qr(rng.standard_normal((G, d)))[0])
    strength = 12.0 - 2.0 * np.arange(d)
    out = []
    for i, n in enumerate(sizes):
        f = np.abs(rng.standard_normal((d, n))) * strength[:, None]
        x = dirs @ f + 0.05 * np.abs(rng.standard_normal((G, n))) + 0.2 * i
        mask = rng.random((G, n)) < density
        out.append(sp.csc_matrix(np.where(mask, x, 0.0)))
    return out, d
