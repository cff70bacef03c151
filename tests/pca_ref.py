"""What the device multiBatchPCA (csrc/pca.hip, R/multiBatchPCA.R:211-322) and the stand-alone projection (csrc/prepca.hip)
are held to in tests/test_cpu_pca.py and tests/test_gpu_pca.py.  A helper module (not a conftest); it imports nothing from
the package under test.  Batches are genes x cells.

Three things live here.

* `exact(batches, weights, cos_norm)`: the operator  M = sum_b (w_b / n_b) C_b C_b^T,  C_b = x_b diag(scale_b) - mu 1^T,
  rebuilt from the inputs in numpy.longdouble, and what any `fit` must satisfy against it whatever its start block and
  however many times it applied the operator:
      Ritz identity        R^T M R = diag(s^2),  R^T R = I     (fit ends with Rayleigh-Ritz on (Q, Y = M Q))
      projection identity  pcs[b] = (x_b diag(scale_b) - centers 1^T)^T R    from the fit's OWN centers and R
  plus the centres and, for a converged fit, the residual  max_j |M r_j - s_j^2 r_j| / s_1^2.
* `fixed_count_f64(...)`: the same algorithm in plain float64 numpy, with one deliberate fault on request.  It shows that
  the allowances can be met in FP64 and that each planted fault is far outside them.
* The allowances and the case table.

The allowances, with u = 2^-53.  Every one is  (number of roundings on the way to the value) x u x (the same expression
with every term replaced by its absolute value): a sum of k terms is within k u sum|terms| of exact IN ANY ORDER (MFMA
order, split order, chunk order), each further product or quotient adds one u, and a per-cell factor scale_c = 1 /
max(1e-8, l2) computed in FP64 is within (G + 2) u of exact (G squares summed, a square root, a reciprocal).  The
longdouble side (2^-64) is 2^-11 of every allowance and is ignored.

  centers[g]       (n_max + 2 B + 6) u sum_b (w_b / W) mean_c |scale_c x_gc|
                   n_b terms of a gene sum; the product scale_c x_gc; the division by n_b; W from B terms; w_b / W; the
                   product with the mean; B terms into mu.  Under cos_norm + (G + 2) u for scale_c.
  projection[c,j]  (G + 3) u (scale_c sum_g |x_gc| |r_gj| + sum_g |mu_g| |r_gj|)
                   two G-term sums, the product with scale_c, the subtraction.  Under cos_norm + (G + 2) u on the first
                   term for the device's own scale_c (the exact side normalises in longdouble).
  R^T R - I [i,j]  (G |r_i|^T |r_j| + 90 L) u
                   the G-term Gram sum of the second Cholesky-QR pass, and L-term pieces: the Cholesky factor (L + 1), the
                   triangular inverse and the product with it (2 L), the product with the eigenvectors (2 L sqrt(L) / L
                   <= 23 at L = 128), and the eigenvectors' own orthogonality, 6 (L - 1) u a sweep (every column is rotated
                   L - 1 times a sweep; a rotation is 2 products and a sum with c, s each within 2 u) over at most 10
                   sweeps of a quadratically convergent cyclic Jacobi.
  Ritz defect[i,j] K u |r_i|^T (sum_b (w_b / n_b) |C_b| |C_b|^T) |r_j|  +  (120 L + 9 sqrt(L)) u s_1^2
                   K = 2 G + n_max + L + B + 10: Z = C^T Q (G terms, scale, centring: G + 3), Y += coef C Z (n_b terms in
                   any split, scale, coef, the rank-one term: n_max + 5, B batches), T = Q^T Y (G terms), the rotation
                   Q V (L terms), s = sqrt(theta) and its square (2).  Under cos_norm scale_c enters twice: + 2 (G + 2).
                   The second term is the eigen-solver on T (|T| = s_1^2): 12 (L - 1) u a sweep from both sides over 10
                   sweeps, and the Jacobi stop  offd^2 <= 1e-30 diag^2,  |offd| <= 1e-15 sqrt(L) s_1^2 = 9 sqrt(L) u s_1^2.
                   R^T M R = V^T (Q^T M Q) V = diag(theta) needs no orthonormal Q, so no such term enters.
  residual         max_j (K u |A |r_j||_2 + 120 L u s_1^2) / s_1^2 + G u residual,  A the matrix of absolute values
                   above: the same roundings per element of M r_j - s_j^2 r_j, and the G-term sum of its norm.
"""
from __future__ import annotations

import functools

import numpy as np

U = 2.0 ** -53
LD = np.longdouble


def width(d):
    """The subspace block the device uses for d wanted vectors."""
    return 64 if d <= 56 else 128


def weight_vector(ncells, weights):
    """.construct_weight_vector (R/multiBatchPCA.R:299-334) for None / True (equal), False (batch sizes) or a vector."""
    n = np.asarray(ncells, dtype=np.float64)
    if weights is None or weights is True:
        return np.ones_like(n)
    if weights is False:
        return n.copy()
    w = np.asarray(weights, dtype=np.float64)
    assert w.shape == n.shape
    return w


def scales(x, cos_norm):
    """1 / max(1e-8, l2) per cell (R/cosineNorm.R:63-82) in x's own precision, or ones."""
    if not cos_norm:
        return np.ones(x.shape[1], dtype=x.dtype)
    l2 = np.sqrt((x * x).sum(axis=0))
    return 1.0 / np.maximum(x.dtype.type(1e-8), l2)


# ---------------------------------------------------------------------------------------------- exact side
class exact:
    """The operator of the inputs in longdouble; R, s, centers are a fit's float64 results."""

    def __init__(self, batches, weights, cos_norm):
        self.cos_norm = bool(cos_norm)
        self.x = [np.asarray(b, dtype=LD) for b in batches]
        self.G = self.x[0].shape[0]
        self.n = [b.shape[1] for b in self.x]
        self.w = weight_vector(self.n, weights).astype(LD)
        self.scale = [scales(b, cos_norm) for b in self.x]
        self.xs = [b * s[None, :] for b, s in zip(self.x, self.scale)]
        self.coef = [w / LD(n) for w, n in zip(self.w, self.n)]
        self.mu = sum((w / self.w.sum()) * b.mean(axis=1) for w, b in zip(self.w, self.xs))
        self.C = [b - self.mu[:, None] for b in self.xs]

    def centers(self):
        return self.mu

    def ritz_defect(self, R, s):
        """R^T M R - diag(s^2), d x d, through Z_b = C_b^T R (M is not formed)."""
        R = np.asarray(R, dtype=LD)
        out = np.zeros((R.shape[1], R.shape[1]), dtype=LD)
        for c, C in zip(self.coef, self.C):
            Z = C.T @ R
            out += c * (Z.T @ Z)
        return out - np.diag(np.asarray(s, dtype=LD) ** 2)

    def gram_defect(self, R):
        R = np.asarray(R, dtype=LD)
        return R.T @ R - np.eye(R.shape[1], dtype=LD)

    def projection(self, b, R, centers):
        """(x_b diag(scale_b) - centers 1^T)^T R from the given (the fit's own) centers and rotation."""
        return (self.xs[b] - np.asarray(centers, dtype=LD)[:, None]).T @ np.asarray(R, dtype=LD)

    def apply(self, R):
        R = np.asarray(R, dtype=LD)
        return sum(c * (C @ (C.T @ R)) for c, C in zip(self.coef, self.C))

    def residual(self, R, s):
        """max_j |M r_j - s_j^2 r_j|_2 / s_1^2."""
        R, s2 = np.asarray(R, dtype=LD), np.asarray(s, dtype=LD) ** 2
        D = self.apply(R) - R * s2[None, :]
        return np.sqrt((D * D).sum(axis=0)).max() / s2[0]


# ---------------------------------------------------------------------------------------------- allowances
class allowances:
    """What FP64 may differ from `exact` by (module docstring); float64 arithmetic is ample for an allowance."""

    def __init__(self, ex):
        self.ex = ex
        self.G, self.B, self.nmax = ex.G, len(ex.n), max(ex.n)
        self.cos = (self.G + 2) if ex.cos_norm else 0
        self.absxs = [np.abs(b).astype(np.float64) for b in ex.xs]
        self.absC = [np.abs(C).astype(np.float64) for C in ex.C]
        self.coef = [float(c) for c in ex.coef]
        self.absmu = np.abs(ex.mu).astype(np.float64)

    def centers(self):
        W = float(self.ex.w.sum())
        mag = sum(float(w) / W * a.mean(axis=1) for w, a in zip(self.ex.w, self.absxs))
        return (self.nmax + 2 * self.B + 6 + self.cos) * U * mag

    def projection(self, b, R, centers):
        aR = np.abs(np.asarray(R, dtype=np.float64))
        data = self.absxs[b].T @ aR
        cent = np.abs(np.asarray(centers, dtype=np.float64)) @ aR
        return (self.G + 3 + self.cos) * U * data + (self.G + 3) * U * cent[None, :]

    def gram(self, R):
        aR = np.abs(np.asarray(R, dtype=np.float64))
        return (self.G * (aR.T @ aR) + 90 * width(aR.shape[1])) * U

    def K(self, L):
        return 2 * self.G + self.nmax + L + self.B + 10 + 2 * self.cos

    def ritz(self, R, s):
        aR = np.abs(np.asarray(R, dtype=np.float64))
        L = width(aR.shape[1])
        mag = np.zeros((aR.shape[1], aR.shape[1]))
        for c, aC in zip(self.coef, self.absC):
            Z = aC.T @ aR
            mag += c * (Z.T @ Z)
        return self.K(L) * U * mag + (120 * L + 9 * np.sqrt(L)) * U * float(s[0]) ** 2

    def residual(self, R, s, value):
        aR = np.abs(np.asarray(R, dtype=np.float64))
        L = width(aR.shape[1])
        img = sum(c * (aC @ (aC.T @ aR)) for c, aC in zip(self.coef, self.absC))
        s12 = float(s[0]) ** 2
        per = self.K(L) * U * np.sqrt((img * img).sum(axis=0)) + 120 * L * U * s12
        return float(per.max() / s12 + self.G * U * float(value))


def worst(err, allow):
    """Largest |err| / allowance over all elements (0 where the error is 0)."""
    err = np.abs(np.asarray(err, dtype=LD))
    allow = np.broadcast_to(np.asarray(allow, dtype=LD), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / allow)
    assert not np.any(np.isnan(r))
    return float(r.max())


def fit_ratios(ex, al, fit):
    """error / allowance of a fit {"rotation", "d", "centers"} for the Ritz defect, R^T R - I and the centres."""
    R, s = fit["rotation"], fit["d"]
    assert R.shape == (ex.G, len(s)) and np.all(np.isfinite(R)) and np.all(np.isfinite(s))
    return {"ritz": worst(ex.ritz_defect(R, s), al.ritz(R, s)),
            "orth": worst(ex.gram_defect(R), al.gram(R)),
            "centers": worst(np.asarray(fit["centers"], dtype=LD) - ex.centers(), al.centers())}


def projection_ratio(ex, al, fit, pcs=None):
    """error / allowance of every element of every batch's projection against the fit's own centers and rotation."""
    pcs = fit["pcs"] if pcs is None else pcs
    out = 0.0
    for b in range(len(ex.n)):
        assert pcs[b].shape == (ex.n[b], fit["rotation"].shape[1])
        want = ex.projection(b, fit["rotation"], fit["centers"])
        out = max(out, worst(np.asarray(pcs[b], dtype=LD) - want, al.projection(b, fit["rotation"], fit["centers"])))
    return out


def residual_ratios(ex, al, fit, tol):
    """(recomputed residual - tol) / allowance and |reported - recomputed| / allowance."""
    true = float(ex.residual(fit["rotation"], fit["d"]))
    allow = al.residual(fit["rotation"], fit["d"], true)
    return {"true": true, "reported": float(fit["residual"]), "allow": allow,
            "over_tol": max(0.0, true - tol) / allow, "reported_off": abs(float(fit["residual"]) - true) / allow}


# ---------------------------------------------------------------------------------------------- float64 restatement
FAULTS = ("drop_last_cell", "drop_last_gene", "no_centring_term", "no_centring_at_all", "scale_once", "n_minus_one",
          "projection_no_off", "projection_swap_cells")
# no_centring_term leaves  - coef mu (1^T Z)  out of the LAST batch only.  Left out of every batch it is no fault: the terms
# add up to  - mu (sum_b w_b (mean_b - mu))^T Q = 0  by the definition of mu, and so do the  - 1 (mu^T Q)  terms of Z; what the
# terms do is keep each batch's partial result small.  "all_batches" below is that harmless variant (test_cpu_pca.py shows
# it inside the allowance); no_centring_at_all drops both terms everywhere, the operator of the uncentred data.
HARMLESS = "no_centring_term_all_batches"


def fixed_count_f64(batches, weights, cos_norm, d, iters, fault=None, seed=0):
    """multiBatchPCA by `iters` plain subspace steps on a block of width(d) vectors, float64 throughout: the operator in the
    two-product form  Z = diag(scale) x^T Q - 1 (mu^T Q),  Y += coef (x diag(scale) Z - mu (1^T Z)),  QR between the steps,
    eigh of the symmetrised Q^T Y at the end; projections as  diag(scale) x^T R - 1 (mu^T R).  `fault`: one of FAULTS.
    Raises numpy.linalg.LinAlgError where a block's Gram matrix is not positive definite (the device would leave for the
    host path there)."""
    assert fault is None or fault in FAULTS or fault == HARMLESS
    x = [np.asarray(b, dtype=np.float64) for b in batches]
    G, n = x[0].shape[0], [b.shape[1] for b in x]
    w = weight_vector(n, weights)
    sc = [scales(b, cos_norm) for b in x]
    mu = np.zeros(G)
    for wb, b, s in zip(w, x, sc):
        mu += (wb / w.sum()) * ((b * s[None, :]).sum(axis=1) / b.shape[1])
    L = width(d)
    assert 1 <= d <= L - 8 and G >= L and sum(n) > L and iters >= 1
    coef = [wb / ((nb - 1) if fault == "n_minus_one" else nb) for wb, nb in zip(w, n)]

    def orth(Y):
        if fault is None:   # (a fault may well make the block singular: the operator without a gene at G = L)
            np.linalg.cholesky(Y.T @ Y)
        return np.linalg.qr(Y)[0]

    def apply(Q):
        Y = np.zeros_like(Q)
        g = slice(0, G - 1) if fault == "drop_last_gene" else slice(0, G)
        muQ = mu[g] @ Q[g]
        for i, (b, s) in enumerate(zip(x, sc)):
            if fault == "drop_last_cell" and i == len(x) - 1:
                b, s = b[:, :-1], s[:-1]
            Z = s[:, None] * (b[g].T @ Q[g])
            if fault != "no_centring_at_all":
                Z -= muQ[None, :]
            back = Z if fault == "scale_once" else s[:, None] * Z
            Y[g] += coef[i] * (b[g] @ back)
            if not (fault == "no_centring_at_all" or fault == HARMLESS or (fault == "no_centring_term" and i == len(x) - 1)):
                Y[g] -= coef[i] * np.outer(mu[g], Z.sum(axis=0))
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
    D = Yr[:, :d] - Xr[:, :d] * theta[None, :d]
    pcs = []
    for i, (b, s) in enumerate(zip(x, sc)):
        p = s[:, None] * (b.T @ R)
        if fault != "projection_no_off":
            p = p - (mu @ R)[None, :]
        if fault == "projection_swap_cells" and i == len(x) - 1 and p.shape[0] >= 2:
            k = p.shape[0] // 2
            p[[k - 1, k]] = p[[k, k - 1]]
        pcs.append(p)
    return {"rotation": R, "centers": mu, "d": np.sqrt(np.maximum(theta[:d], 0.0)), "pcs": pcs,
            "residual": float(np.sqrt((D * D).sum(axis=0)).max() / theta[0])}


# ---------------------------------------------------------------------------------------------- cases
class Case:
    def __init__(self, G, sizes, d, weights=None, cos_norm=False, iters=None, rank=12, zero=None, seed=0):
        self.G, self.sizes, self.d, self.weights, self.cos_norm, self.iters = G, sizes, d, weights, cos_norm, iters
        self.rank, self.zero, self.seed = rank, zero, seed

    def kwargs(self):
        return {"d": self.d, "weights": self.weights, "cos_norm": self.cos_norm}


TOL = 1e-9   # the default of fit(); the converged cases (iters=None) run to it

# iters 1 / 2: the fixed-count form, R still close to a random subspace, so a fault in the operator shows at full size.
# zero=(b, c): cell c of batch b is all zero (inv = 1e8 under cos_norm).  Splits of the TN product start at 4096 cells:
# (4100, 300) is two splits of 2080 + 2020 rows (the second ends in a 4-row K step), (6149,) three of 2080 + 2080 + 1989.
# Per-batch cell counts below 64 reach the row clamp of the NT product; 257 and 513 cells give two chunks of the gene sums
# and the column sums.  K % 32 of the NT product is G % 32; the TN gene tile is ragged where G % 64 != 0.
CASES = {
    # ---- L = 64
    "g64-clamp-i2":        Case(64, (1, 2, 63, 70), 10, iters=2),
    "g65-clamp-cos-w-i1":  Case(65, (1, 2, 63, 70), 10, weights=(1.0, 3.0, 0.5, 2.0), cos_norm=True, iters=1, zero=(2, 31)),
    "g95-small-d1-wn-i2":  Case(95, (31, 33, 64, 65), 1, weights=False, iters=2),
    "g96-small-cos-i2":    Case(96, (31, 33, 64, 65), 10, cos_norm=True, iters=2),
    "g130-chunks-w-i1":    Case(130, (257, 513), 10, weights=(2.0, 1.0), iters=1),
    "g333-chunks-d56-cos-wn-i2": Case(333, (257, 513), 56, weights=False, cos_norm=True, iters=2, zero=(1, 256)),
    "g64-split2-i1":       Case(64, (4100, 300), 10, iters=1),
    "g65-split2-d56-cos-w-i2": Case(65, (4100, 300), 56, weights=(1.0, 2.5), cos_norm=True, iters=2, zero=(0, 2050)),
    "g95-split2-d1-wn-i2": Case(95, (4100, 300), 1, weights=False, iters=2),
    "g96-split3-i1":       Case(96, (6149,), 10, iters=1),
    "g130-split3-cos-i2":  Case(130, (6149,), 10, cos_norm=True, iters=2),
    "g65-split3-d56-i2":   Case(65, (6149,), 56, iters=2),
    # 65 cells = L + 1 with G = 64 leaves M with a smallest eigenvalue near 0 (a 64 x 65 noise block), which the second
    # step's Gram matrix squares: the minimal-cell case is therefore one step (no Gram matrix of M Q) at G = 96
    "g96-cells-L+1-i1":    Case(96, (20, 45), 10, iters=1),
    "g130-three-w-i2":     Case(130, (70, 257, 300), 10, weights=(1.0, 3.0, 0.5), iters=2),
    "g130-three-cos-wn-i2": Case(130, (70, 257, 300), 10, weights=False, cos_norm=True, iters=2),
    # ---- L = 128 (d >= 57)
    "g128-clamp-d57-i1":   Case(128, (1, 2, 63, 70), 57, iters=1),
    "g129-chunks-d80-cos-w-i2": Case(129, (257, 513), 80, weights=(1.0, 3.0), cos_norm=True, iters=2, zero=(0, 128)),
    "g191-small-d120-i1":  Case(191, (31, 33, 64, 65), 120, iters=1),
    "g129-split2-d120-wn-i2": Case(129, (4100, 300), 120, weights=False, iters=2),
    "g128-split3-d57-cos-i1": Case(128, (6149,), 57, cos_norm=True, iters=1),
    "g191-cells-L+1-d80-i1": Case(191, (60, 69), 80, iters=1),
    # ---- genes beyond one split of the Gram / Rayleigh-Ritz products (TN over genes: a split per 512 rows, KC = 32 rows a
    # step): 1100 genes are two splits of 576 + 524 rows, the second ending in a 12-row step; 2100 four, 1600 three.  One
    # step: after two, a product that loses whole genes satisfies the Ritz identity (test_cpu_pca.py, drop_last_gene)
    "g1100-gsplit2-cos-w-i1": Case(1100, (257, 513), 10, weights=(2.0, 1.0), cos_norm=True, iters=1),
    "g2100-gsplit4-d57-i1": Case(2100, (70, 257, 300), 57, iters=1),
    # ---- converged (default tol): the filter recurrence and the reported residual
    "conv-g130-chunks":    Case(130, (257, 513), 10),
    "conv-g70-split2-cos-w": Case(70, (4100, 300), 10, weights=(1.0, 2.5), cos_norm=True, zero=(0, 2050)),
    "conv-g333-small-wn":  Case(333, (31, 33, 64, 65), 10, weights=False),
    "conv-g191-d57-cos":   Case(191, (257, 513), 57, cos_norm=True, rank=60),
    "conv-g96-split3-d1":  Case(96, (6149,), 1),
    "conv-g1600-gsplit3":  Case(1600, (257, 513), 10),
}
FIXED = [k for k, c in CASES.items() if c.iters is not None]
CONVERGED = [k for k, c in CASES.items() if c.iters is None]
F64_ITERS_CONVERGED = 40   # plain steps that take the float64 restatement below TOL on the converged cases


@functools.lru_cache(maxsize=None)
def case(name):
    """(Case, batches) by name, built once: low-rank signal + noise + a per-gene offset per batch; under cos_norm shifted
    away from the origin, as normalised expression is."""
    c = CASES[name]
    rng = np.random.default_rng([c.G, c.d, sum(c.sizes), c.seed])
    load = rng.standard_normal((c.G, c.rank)) * np.linspace(3.0, 1.0, c.rank)
    out = []
    for i, n in enumerate(c.sizes):
        x = load @ rng.standard_normal((c.rank, n)) + 0.3 * rng.standard_normal((c.G, n))
        x += 0.4 * i * rng.standard_normal((c.G, 1)) + (3.0 if c.cos_norm else 0.0)
        out.append(x)
    if c.zero is not None:
        out[c.zero[0]][:, c.zero[1]] = 0.0
    for m in out:
        m.setflags(write=False)
    return c, out


@functools.lru_cache(maxsize=None)
def reference(name):
    """(exact, allowances) of a case, built once and shared."""
    c, B = case(name)
    ex = exact(B, c.weights, c.cos_norm)
    return ex, allowances(ex)


@functools.lru_cache(maxsize=None)
def contract_case():
    """The input of test_gpu_pca.py::test_fit_contract_of_both_handles: 130 genes, batches of 257 and 300 cells of seeded
    normal noise -- a flat spectrum, so that one application of the operator is nowhere near TOL."""
    rng = np.random.default_rng(20260)
    out = [rng.standard_normal((130, n)) for n in (257, 300)]
    for m in out:
        m.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------- stand-alone projection
PROJECT_SHAPES = [   # (G, n, d, cos_norm): bx.project stages 64 genes x d and 16 cells a workgroup; d <= 256
    (1, 1, 1, False), (63, 15, 15, True), (64, 16, 16, False), (65, 17, 17, True), (200, 500, 120, True),
    (65, 17, 256, True), (200, 16, 256, False), (63, 500, 16, False), (64, 1, 120, True), (65, 15, 1, False),
]


@functools.lru_cache(maxsize=None)
def project_case(G, n, d, cos_norm):
    """(x, rotation, centers) for bx.project: any rotation will do, orthonormal or not.  Under cos_norm a middle cell is
    all zero."""
    rng = np.random.default_rng([G, n, d, int(cos_norm)])
    x = rng.standard_normal((G, n)) + (3.0 if cos_norm else 0.0)
    if cos_norm:
        x[:, n // 2] = 0.0
    rot = rng.standard_normal((G, d)) / np.sqrt(G)
    cen = rng.standard_normal(G) * 0.5 + (0.3 if cos_norm else 0.0)
    for m in (x, rot, cen):
        m.setflags(write=False)
    return x, rot, cen


def project_f64(x, rot, cen, cos_norm):
    s = scales(np.asarray(x, dtype=np.float64), cos_norm)
    return s[:, None] * (x.T @ rot) - (cen @ rot)[None, :]


def project_ratio(x, rot, cen, cos_norm, got):
    """error / allowance of a stand-alone projection, every element."""
    ex = exact([x], None, cos_norm)
    al = allowances(ex)
    assert got.shape == (x.shape[1], rot.shape[1]) and np.all(np.isfinite(got))
    return worst(np.asarray(got, dtype=LD) - ex.projection(0, rot, cen), al.projection(0, rot, cen))
