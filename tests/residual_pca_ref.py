"""What regressBatches(d=, deferred=True) (csrc/linear_correct.hip: ResidualPca::fit, R/regressBatches.R:148-155 with
deferred=TRUE) is held to in tests/test_cpu_residual_pca.py and tests/test_gpu_residual_pca.py.  A helper module (not a
conftest); it imports nothing from the package under test, only tests/pca_ref.py, whose checks it reuses.

The PCA is multiBatchPCA of the residuals  R_b = x_b - K Dd_b^T  (K = coef[, drop], Dd_b the dropped design columns of batch
b's cells), so `exact` below is pca_ref.exact with, in numpy.longdouble,
    C_b = x_b - K Dd_b^T - mu 1^T,    mu = sum_b (w_b / W) mean_c R_b   (the mean over ALL cells of a batch).
K and the design are INPUTS: the GPU tests hand in the coefficients the device returned, so only the PCA is under test.
Without a design the term is rank one per batch: K is then given per batch (its restricted mean, one column) with Dd_b a
column of ones.  Batches here hold the PCA rows only.

The allowances follow pca_ref's rule -- (number of roundings on the way) x 2^-53 x (the same expression with every term
replaced by its absolute value) -- with three changes, derived from the operator and not fitted to any result:

  * wherever pca_ref.allowances uses |C_b| (or |x_b|), the magnitude is  |x_b| + |K| |Dd_b|^T + |mu| 1^T  (without the last
    term where pca_ref has |x_b|): the device never forms R_b, so nothing of x_b cancels against K Dd_b^T before it is
    rounded;
  * each low-rank product adds  LR = (pd + 1) + 2  roundings: its (pd + 1)-term sum (E_b = [Dd_b | 1], F = [K | mu]), the
    product with the factor in front and the subtraction from the big product.  Z = x_b^T Q - E_b (F^T Q) has one, Y += coef
    (x_b Z - F (E_b^T Z)) another:  K(L) = pca_ref's K(L) + 2 LR;  a projection is a Z:  G + 3 + LR.
  * centres: pca_ref's count plus  n_max + 1  (the mean design row d_b: n_b terms and a division) plus  pd + 2  (the
    pd-term sum K d_b, and its subtraction from the data's mean and the product in front), on the magnitude
    sum_b (w_b / W) (mean_c |x_gc| + |K| mean_c |Dd_b|).

`deferred_f64` restates the operator in plain float64 in the device's own form
    T = F^T Q,   Z_b = x_b^T Q - E_b T,   S_b = E_b^T Z_b,   Y += (w_b / n_b) (x_b Z_b - F S_b)
with one deliberate fault on request (FAULTS)."""
from __future__ import annotations

import functools

import numpy as np

from tests import pca_ref as P

U, LD = P.U, P.LD
D_WANTED = 5


def _per_batch(coefs, nb):
    return list(coefs) if isinstance(coefs, (list, tuple)) else [coefs] * nb


# ---------------------------------------------------------------------------------------------- exact side
class exact(P.exact):
    """pca_ref.exact on the residuals.  batches: PCA rows x n_b; coefs: [rows x p], or one such array per batch; designs:
    [n_b x p] per batch; drop: the 0-based columns that are regressed out."""

    def __init__(self, batches, coefs, designs, drop, weights=None):
        drop = np.asarray(drop, dtype=np.int64)
        self.cos_norm = False
        self.raw = [np.asarray(b, dtype=LD) for b in batches]
        self.G = self.raw[0].shape[0]
        self.n = [b.shape[1] for b in self.raw]
        self.w = P.weight_vector(self.n, weights).astype(LD)
        self.scale = [np.ones(n, dtype=LD) for n in self.n]
        self.pd = int(drop.size)
        self.K = [np.asarray(k, dtype=LD)[:, drop] for k in _per_batch(coefs, len(self.n))]
        self.Dd = [np.asarray(dm, dtype=LD)[:, drop] for dm in designs]
        self.x = self.xs = [x - k @ dm.T for x, k, dm in zip(self.raw, self.K, self.Dd)]   # the residuals
        self.coef = [w / LD(n) for w, n in zip(self.w, self.n)]
        self.mu = sum((w / self.w.sum()) * r.mean(axis=1) for w, r in zip(self.w, self.xs))
        self.C = [r - self.mu[:, None] for r in self.xs]


class allowances(P.allowances):
    """pca_ref.allowances with the magnitudes and counts of the module docstring."""

    def __init__(self, ex):
        super().__init__(ex)
        self.pd = ex.pd
        self.lowrank = ex.pd + 1 + 2
        self.absK = [np.abs(k).astype(np.float64) for k in ex.K]
        self.absDd = [np.abs(dm).astype(np.float64) for dm in ex.Dd]
        self.absxs = [np.abs(x).astype(np.float64) + k @ dm.T for x, k, dm in zip(ex.raw, self.absK, self.absDd)]
        self.absC = [a + self.absmu[:, None] for a in self.absxs]

    def centers(self):
        W = float(self.ex.w.sum())
        mag = sum(float(w) / W * a.mean(axis=1) for w, a in zip(self.ex.w, self.absxs))
        return (2 * self.nmax + 2 * self.B + 6 + 1 + self.pd + 2) * U * mag

    def projection(self, b, R, centers):
        aR = np.abs(np.asarray(R, dtype=np.float64))
        data = self.absxs[b].T @ aR
        cent = np.abs(np.asarray(centers, dtype=np.float64)) @ aR
        return (self.G + 3 + self.lowrank) * U * (data + cent[None, :])

    def K(self, L):
        return super().K(L) + 2 * self.lowrank


# ---------------------------------------------------------------------------------------------- float64 restatement
FAULTS = ("no_ET", "no_FS", "mu_restricted", "S_drop_last_cell", "drop_as_keep")
# no_ET / no_FS: E_b T left out of Z / F S_b left out of Y, in every batch.  They differ from the operator by
# sum_b coef_b C_b E_b F^T Q (and its transpose), and  C_b E_b = [R_b Dd_b - mu 1^T Dd_b | n_b (r_b - mu)]  vanishes where every
# batch's residuals sum to zero against its own E_b: without a design and without a restriction (R_b 1 = 0, mu = 0).  There
# they are no faults (test_cpu_residual_pca.py shows them inside the allowance) and are not planted.
# mu_restricted: the batch means taken over the restricted cells; planted where there is a restriction.
# S_drop_last_cell: the last cell of the last batch missing from S_b.   drop_as_keep: the kept columns regressed out instead
# of the dropped ones (without `keep`: nothing is regressed out).


def deferred_f64(batches, coefs, designs, drop, d, iters, weights=None, restrict=None, fault=None, seed=0):
    """multiBatchPCA of the residuals by `iters` plain subspace steps in the deferred form, float64 throughout.  restrict:
    0-based cells per batch (or None), used by the mu_restricted fault only.  Raises numpy.linalg.LinAlgError where a
    block's Gram matrix is not positive definite (the device would leave for the host path there)."""
    assert fault is None or fault in FAULTS
    x = [np.asarray(b, dtype=np.float64) for b in batches]
    G, n = x[0].shape[0], [b.shape[1] for b in x]
    p = np.asarray(designs[0]).shape[1]
    drop = np.asarray(drop, dtype=np.int64)
    if fault == "drop_as_keep":
        drop = np.setdiff1d(np.arange(p), drop)
    Ks = [np.asarray(k, dtype=np.float64)[:, drop] for k in _per_batch(coefs, len(x))]
    Dd = [np.asarray(dm, dtype=np.float64)[:, drop] for dm in designs]
    w = P.weight_vector(n, weights)
    mu = np.zeros(G)
    for i, (wb, b, k, dm) in enumerate(zip(w, x, Ks, Dd)):
        cells = slice(None)
        if fault == "mu_restricted" and restrict is not None and restrict[i] is not None:
            cells = np.asarray(restrict[i], dtype=np.int64)
        mu += (wb / w.sum()) * (b[:, cells].sum(axis=1) / b[:, cells].shape[1] - k @ dm[cells].mean(axis=0))
    E = [np.concatenate([dm, np.ones((nb, 1))], axis=1) for dm, nb in zip(Dd, n)]
    F = [np.concatenate([k, mu[:, None]], axis=1) for k in Ks]
    L = P.width(d)
    assert 1 <= d <= L - 8 and G >= L and sum(n) > L and iters >= 1
    coef = [wb / nb for wb, nb in zip(w, n)]

    def orth(Y):
        if fault is None:
            np.linalg.cholesky(Y.T @ Y)
        return np.linalg.qr(Y)[0]

    def apply(Q):
        Y = np.zeros_like(Q)
        for i, (b, e, f) in enumerate(zip(x, E, F)):
            Z = b.T @ Q
            if fault != "no_ET":
                Z -= e @ (f.T @ Q)
            S = e[:-1].T @ Z[:-1] if (fault == "S_drop_last_cell" and i == len(x) - 1) else e.T @ Z
            Y += coef[i] * (b @ Z)
            if fault != "no_FS":
                Y -= coef[i] * (f @ S)
        return Y

    Q = orth(np.random.default_rng(seed).standard_normal((G, L)))
    for it in range(iters):
        Y = apply(Q)
        if it + 1 < iters:
            Q = orth(Y)
    T = Q.T @ Y
    theta, V = np.linalg.eigh(0.5 * (T + T.T))
    order = np.argsort(theta)[::-1]
    theta, V = theta[order], V[:, order]
    Xr, Yr = Q @ V, Y @ V
    R = np.ascontiguousarray(Xr[:, :d])
    Dres = Yr[:, :d] - Xr[:, :d] * theta[None, :d]
    pcs = [b.T @ R - e @ (f.T @ R) for b, e, f in zip(x, E, F)]
    return {"rotation": R, "centers": mu, "d": np.sqrt(np.maximum(theta[:d], 0.0)), "pcs": pcs,
            "residual": float(np.sqrt((Dres * Dres).sum(axis=0)).max() / theta[0])}


# ---------------------------------------------------------------------------------------------- cases
class Case:
    """rows: the PCA rows; G: the rows of the input (more than `rows` only under subset_row + correct_all); design: None,
    "factor+covariate" (intercept, a two-level factor, a covariate; keep = [3]) or the number of random columns, all
    dropped."""

    def __init__(self, rows, sizes, design=None, restrict=False, G=None, seed=0):
        self.rows, self.sizes, self.design, self.restrict = rows, sizes, design, restrict
        self.G = rows if G is None else G
        self.seed = seed


SMALL, THREE, SPLIT = (1, 2, 63, 70), (70, 257, 130), (300, 4200)
# PCA rows 64 / 65 / 130: K % 32 of the NT product and the ragged gene tile of the TN product (pca_ref.py).  SMALL: cell
# counts below the 64-row tile and the 16-row wave of the low-rank kernel (1, 2, 63 = 3 * 16 + 15); THREE: two chunks of the
# gene sums; SPLIT: 4200 cells are two splits of both TN products (the main one and S_b = E_b^T Z).  Dropped columns 15 / 16
# / 64 give pd + 1 = 16 / 17 / 65 columns of E_b and F: one register tile exactly, one more, and one past the 64-wide tile
# of the TN product that forms S_b.  64 dropped columns go with THREE and SPLIT only: SMALL has 136 cells, of which 64
# regressed out would leave the residuals of 64 rows with a smallest eigenvalue near zero (pca_ref.py, "cells-L+1").
CASES = {
    "r64-small-none":             Case(64, SMALL),
    "r65-small-none-restrict":    Case(65, SMALL, restrict=True),
    "r130-three-none":            Case(130, THREE),
    "r130-three-none-restrict":   Case(130, THREE, restrict=True),
    "r64-three-fc":               Case(64, THREE, "factor+covariate"),
    "r65-small-fc":               Case(65, SMALL, "factor+covariate"),
    "r130-small-p15":             Case(130, SMALL, 15),
    "r64-small-p16-restrict":     Case(64, SMALL, 16, restrict=True),
    "r65-three-p15-restrict":     Case(65, THREE, 15, restrict=True),
    "r130-three-p16":             Case(130, THREE, 16),
    "r64-three-p64":              Case(64, THREE, 64),
    "r65-three-p64-restrict":     Case(65, THREE, 64, restrict=True),
    "r130-three-p64":             Case(130, THREE, 64),
    "r65-split-none":             Case(65, SPLIT),
    "r64-split-fc":               Case(64, SPLIT, "factor+covariate"),
    "r130-split-p64-restrict":    Case(130, SPLIT, 64, restrict=True),
    "sub70-three-none":           Case(70, THREE, G=130),
    "sub70-small-p16-restrict":   Case(70, SMALL, 16, restrict=True, G=130),
}
CONVERGED = ("r130-three-none-restrict", "r65-small-fc", "r130-three-p64", "r65-split-none", "sub70-small-p16-restrict")
TOL = 1e-9
F64_ITERS_CONVERGED = 40


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of a case, built once: {"batches" (G x n_b each), "design" (N x p or None), "keep" (1-based or None),
    "restrict" (1-based cells per batch, unsorted, or None), "subset_row" (1-based, permuted, or None)}.  Low-rank signal
    (rank 5 = d) + noise + a per-batch, per-gene offset of the signal's size + the design's effects of that size."""
    c = CASES[name]
    rng = np.random.default_rng([c.G, c.rows, sum(c.sizes), len(name), c.seed])
    N = sum(c.sizes)
    design = keep = None
    if c.design == "factor+covariate":
        level = (rng.random(N) < 0.5).astype(np.float64)
        level[:2] = (0.0, 1.0)
        design = np.column_stack([np.ones(N), level, rng.standard_normal(N)])
        keep = np.array([3])
    elif c.design is not None:
        design = np.column_stack([np.ones(N), rng.standard_normal((N, c.design - 1))])
    load = rng.standard_normal((c.G, D_WANTED)) * np.linspace(3.0, 1.5, D_WANTED)
    beta = None if design is None else 2.0 * rng.standard_normal((c.G, design.shape[1])) / np.sqrt(design.shape[1])
    batches, at = [], 0
    for n in c.sizes:
        x = load @ rng.standard_normal((D_WANTED, n)) + 0.3 * rng.standard_normal((c.G, n))
        x += 2.0 * rng.standard_normal((c.G, 1))
        if design is not None:
            x += beta @ design[at:at + n].T
        x.setflags(write=False)
        batches.append(x)
        at += n
    restrict = None
    if c.restrict:   # about half of a batch's cells, in no order
        restrict = [rng.permutation(n)[:max(1, (n + 1) // 2)].astype(np.int32) + 1 for n in c.sizes]
    subset_row = None if c.G == c.rows else rng.permutation(c.G)[:c.rows] + 1
    if design is not None:
        design.setflags(write=False)
    return {"batches": batches, "design": design, "keep": keep, "restrict": restrict, "subset_row": subset_row}


def coefficients_f64(name):
    """regressBatches' coefficients in float64 (G x B restricted means, or G x p least squares on the restricted cells)."""
    k = case(name)
    res = k["restrict"] or [None] * len(k["batches"])
    parts = [x if r is None else x[:, np.sort(r) - 1] for x, r in zip(k["batches"], res)]
    if k["design"] is None:
        return np.column_stack([p.mean(axis=1) for p in parts])
    at, rows = 0, []
    for x, r in zip(k["batches"], res):
        rows.append(at + (np.arange(x.shape[1]) if r is None else np.sort(r) - 1))
        at += x.shape[1]
    dr = k["design"][np.concatenate(rows)]
    return np.linalg.lstsq(dr, np.concatenate(parts, axis=1).T, rcond=None)[0].T


def operands(name, coefficients):
    """What `exact` and `deferred_f64` take for a case and regressBatches' coefficients (G x B or G x p, rows in the
    caller's order): (PCA-row batches, coefs, designs per batch, dropped columns 0-based, restrict 0-based)."""
    k = case(name)
    rows = slice(None) if k["subset_row"] is None else k["subset_row"] - 1
    batches = [x[rows] for x in k["batches"]]
    coef = np.asarray(coefficients)[rows]
    sizes = [x.shape[1] for x in batches]
    restrict = None if k["restrict"] is None else [np.sort(r).astype(np.int64) - 1 for r in k["restrict"]]
    if k["design"] is None:
        return batches, [coef[:, [b]] for b in range(len(batches))], [np.ones((n, 1)) for n in sizes], [0], restrict
    p = k["design"].shape[1]
    kept = np.zeros(0, dtype=np.int64) if k["keep"] is None else np.asarray(k["keep"]) - 1
    offs = np.concatenate([[0], np.cumsum(sizes)])
    designs = [k["design"][offs[i]:offs[i + 1]] for i in range(len(sizes))]
    return batches, coef, designs, np.setdiff1d(np.arange(p), kept), restrict


def reference(name, coefficients):
    """(exact, allowances) of a case for the given coefficients."""
    batches, coefs, designs, drop, _ = operands(name, coefficients)
    ex = exact(batches, coefs, designs, drop)
    return ex, allowances(ex)
