"""What multiBatchPCA's subset_row / get_all_genes / get_variance (csrc/pca.hip: PcaGenes, R/multiBatchPCA.R:401-432) are
held to in tests/test_cpu_pca_genes.py and tests/test_gpu_pca_genes.py.  A helper module (not a conftest); it imports
nothing from the package under test and builds on tests/pca_ref.py.  Batches are genes x cells; S = the subset rows (in
the caller's order, 0-based here), L = the other rows, ascending.

As in pca_ref, the checks are identities that hold for whatever `fit` returned, so they need no sign alignment and no
spectral gap.  With  y_gc = scale_c x_gc  (scale_c = 1 / max(1e-8, l2 of the cell over S ONLY), or 1),  coef_b = w_b / n_b,
and the fit's OWN pcs, d and centers:

  extension identity  U_L[g, j] = ( P - Q ) / d_j^2,   P = sum_b coef_b sum_c y_gc pcs_b[c, j],
                                                       Q = centers[g] * sum_b coef_b sum_c pcs_b[c, j]
  centres             mu_L[g]   = sum_b (w_b / W) mean_c y_gc                   (from the inputs alone)
  var_total           = sum_b coef_b sum_c sum_{g in S} (y_gc - centers[g])^2 / B
  var_explained       = d^2 / B  exactly (one division of the square the caller can form too)

The device forms the pcs of a block's cells itself with the kernel and operands of its projection, so they are bitwise
the fit's pcs; the identity is therefore evaluated from those.  The allowances follow pca_ref's rule, u = 2^-53: (number
of roundings on the way to the value) x u x (the same expression with every term replaced by its absolute value); a sum
of k terms is within k u sum|terms| in ANY order (MFMA order, cell splits, blocks of any size fed one after the other,
batches), and the device's own scale_c is within (|S| + 2) u of exact (|S| squares summed, a root, a reciprocal): `cos`.

  U_L[g, j]   ( (N + 8 + cos) u |P| + (N + 6) u |Q| ) / d_j^2,   |P|, |Q| with absolute values inside the sums, N = all cells
              P: N terms in any order; the products scale_c * pcs and x * that (2); coef_b = w_b / n_b and the product
              with it (2): N + 4 + cos.  Q: N terms of the column sums; coef_b and its product (2); the product with
              centers[g] (1): N + 3.  Then, on both: the subtraction, d_j * d_j and the division (3).
  mu_L[g]     pca_ref's centres formula  (n_max + 2 B + 6 + cos) u sum_b (w_b / W) mean_c |y_gc|  with cos counted on |S|
              genes: the scale comes from the subset rows whichever row it multiplies.
  var_total   K u sum_b coef_b sum_c sum_{g in S} (|y_gc| + |centers[g]|)^2 / B,   K = |S| + n_max + B + 8 [+ 2 (|S| + 2)]
              a term v^2, v = y - centers[g], a = |y| + |centers[g]|: the product scale * x and the subtraction put v
              within 2 u a (+ cos u a), the square is within 2 a (that) + u a^2: 5 u a^2 (+ 2 cos u a^2).  coef_b, the
              product with it and the division by B: 3.  That is the 8 (and the bracket).  The sum: |S| terms of a cell,
              n_b cells, B batches is the deepest any term can go through, |S| + n_max + B.  (The device's order is
              shallower: a lane adds ceil(n_b / nb / 4) ceil(|S| / 64) <= |S| / 4 + n_max / 64 + 17 terms, a wave 6 more, a
              workgroup 2, the host nb <= n_b / 64 + 1 parts and B batches.)
              The centers are the fit's own.  Their error does not enter to first order anyway: the derivative of the sum
              in centers[g] is  -2 sum_b w_b (mean_b - mu)[g] = 0  by the definition of mu.

The host path (multiBatchPCA_host) against the reference's own words (`literal`: numpy.linalg.svd of the scaled matrix,
left.scaled %*% v swept by d, sum(scaled^2) / nbatches, d^2 / nbatches) is compared column by column after sign
alignment, on inputs with a planted, well separated spectrum.  `literal_bounds` derives that bound.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import pca_ref

U = pca_ref.U
LD = pca_ref.LD


def split_rows(G_all, subset1):
    """(S 0-based in the caller's order, L ascending) for a 1-based subset."""
    sub = np.asarray(subset1, dtype=np.int64) - 1
    keep = np.ones(G_all, dtype=bool)
    keep[sub] = False
    return sub, np.flatnonzero(keep)


# ---------------------------------------------------------------------------------------------- exact side
class exact:
    """The inputs in longdouble, scaled by the subset rows' norms; `fit` is a multiBatchPCA record over all G_all rows."""

    def __init__(self, batches, subset1, weights, cos_norm):
        G_all = batches[0].shape[0]
        self.sub, self.left = split_rows(G_all, subset1)
        self.cos_norm = bool(cos_norm)
        x = [np.asarray(b, dtype=LD) for b in batches]
        self.n = [b.shape[1] for b in x]
        self.N, self.B, self.nmax, self.nS = sum(self.n), len(x), max(self.n), self.sub.size
        self.w = pca_ref.weight_vector(self.n, weights).astype(LD)
        self.coef = [w / LD(n) for w, n in zip(self.w, self.n)]
        self.scale = [pca_ref.scales(b[self.sub], cos_norm) for b in x]
        self.yS = [b[self.sub] * s[None, :] for b, s in zip(x, self.scale)]
        self.yL = [b[self.left] * s[None, :] for b, s in zip(x, self.scale)]
        self.cos = (self.nS + 2) if self.cos_norm else 0

    def centers_left(self):
        return sum((w / self.w.sum()) * y.mean(axis=1) for w, y in zip(self.w, self.yL))

    def _pq(self, fit, absolute):
        f = np.abs if absolute else (lambda a: a)
        pcs = [f(np.asarray(p, dtype=LD)) for p in fit["pcs"]]
        P = sum(c * (f(y) @ p) for c, y, p in zip(self.coef, self.yL, pcs))
        t = sum(c * p.sum(axis=0) for c, p in zip(self.coef, pcs))
        Q = np.outer(f(np.asarray(fit["centers"], dtype=LD)[self.left]), t)
        return P, Q

    def rotation_left(self, fit):
        P, Q = self._pq(fit, False)
        return (P - Q) / (np.asarray(fit["d"], dtype=LD) ** 2)[None, :]

    def rotation_left_allow(self, fit):
        P, Q = self._pq(fit, True)
        return ((self.N + 8 + self.cos) * U * P + (self.N + 6) * U * Q) / (np.asarray(fit["d"], dtype=LD) ** 2)[None, :]

    def centers_left_allow(self):
        mag = sum((w / self.w.sum()) * np.abs(y).mean(axis=1) for w, y in zip(self.w, self.yL))
        return (self.nmax + 2 * self.B + 6 + self.cos) * U * mag

    def var_total(self, fit):
        cen = np.asarray(fit["centers"], dtype=LD)[self.sub][:, None]
        return sum(c * ((y - cen) ** 2).sum() for c, y in zip(self.coef, self.yS)) / self.B

    def var_total_allow(self, fit):
        cen = np.abs(np.asarray(fit["centers"], dtype=LD)[self.sub])[:, None]
        K = self.nS + self.nmax + self.B + 8 + 2 * self.cos
        return K * U * sum(c * ((np.abs(y) + cen) ** 2).sum() for c, y in zip(self.coef, self.yS)) / self.B


def ratios(ex, fit):
    """error / allowance of a record {"rotation", "centers", "d", "pcs", "var_total", "var_explained"} over all rows: the
    extension identity, mu_L, var_total, and how far var_total is BELOW sum(var_explained) in allowances (the d wanted
    directions cannot explain more than everything).  Where the subset rows sit is assembly_ok's to check."""
    R, cen = np.asarray(fit["rotation"]), np.asarray(fit["centers"])
    assert R.shape == (ex.sub.size + ex.left.size, len(fit["d"])) and cen.shape == (R.shape[0],)
    assert np.all(np.isfinite(R)) and np.all(np.isfinite(cen))
    out = {"rotation_left": pca_ref.worst(np.asarray(R[ex.left], dtype=LD) - ex.rotation_left(fit), ex.rotation_left_allow(fit)),
           "centers_left": pca_ref.worst(np.asarray(cen[ex.left], dtype=LD) - ex.centers_left(), ex.centers_left_allow())}
    if "var_total" in fit:
        allow = ex.var_total_allow(fit)
        out["var_total"] = float(abs(LD(fit["var_total"]) - ex.var_total(fit)) / allow)
        out["explained_over_total"] = float(max(LD(0), LD(np.sum(fit["var_explained"])) - LD(fit["var_total"])) / allow)
    return out


# ---------------------------------------------------------------------------------------------- float64 restatement
FAULTS = ("scale_all_rows", "no_scale_left", "divide_by_s", "drop_last_cell", "drop_last_gene", "inv_offset",
          "no_centring_term", "n_minus_one", "sorted_subset")
NEEDS_COS = ("scale_all_rows", "no_scale_left", "inv_offset")
# no_centring_term leaves  - mu_L t_b^T  out of the LAST batch only.  Left out of every batch it is no fault, as in pca_ref:
# sum_b coef_b sum_c pcs_b[c, :] = (sum_b w_b (mean_b - mu))^T R = 0 by the definition of mu; what the term does is keep
# each batch's share small.  HARMLESS is that variant.
HARMLESS = "no_centring_term_all_batches"


def stream_f64(batches, subset1, fit_S, weights, cos_norm, block=None, fault=None):
    """The streaming pass in float64 numpy, as the device does it: for each batch, cells in blocks of `block` (None: the
    whole batch); the block's projections  Z = diag(scale) x_S^T R - 1 (mu_S^T R)  from the subset rows and the fit
    {"rotation", "centers", "d"} on them; A += coef x_L diag(scale) Z, t += coef 1^T Z, gene sums; at the end mu_L and
    (A - mu_L t^T) / d^2, assembled over all rows with the subset rows assigned by index.  Returns the full record with
    "pcs" and "var_total" / "var_explained".  `fault`: one of FAULTS or HARMLESS."""
    assert fault is None or fault in FAULTS or fault == HARMLESS
    x = [np.asarray(b, dtype=np.float64) for b in batches]
    G_all = x[0].shape[0]
    sub, left = split_rows(G_all, subset1)
    R, muS, s = fit_S["rotation"], fit_S["centers"], fit_S["d"]
    n = [b.shape[1] for b in x]
    w = pca_ref.weight_vector(n, weights)
    nl = left.size - 1 if fault == "drop_last_gene" else left.size
    A, t, muL = np.zeros((left.size, R.shape[1])), np.zeros(R.shape[1]), np.zeros(left.size)
    total, pcs = 0.0, []
    for i, b in enumerate(x):
        inv = pca_ref.scales(b if fault == "scale_all_rows" else b[sub], cos_norm)
        invS = pca_ref.scales(b[sub], cos_norm)
        coef = w[i] / (max(n[i] - 1, 1) if fault == "n_minus_one" else n[i])
        cells = n[i] - 1 if (fault == "drop_last_cell" and i == len(x) - 1) else n[i]
        gsum, tb, Zs = np.zeros(left.size), np.zeros(R.shape[1]), []
        step = cells if block is None else block
        for k, lo in enumerate(range(0, cells, max(1, step))):
            hi = min(cells, lo + step)
            Z = invS[lo:hi, None] * (b[sub][:, lo:hi].T @ R) - (muS @ R)[None, :]
            Zs.append(Z)
            off = 0 if (fault == "inv_offset" and k == 1) else lo
            f = np.ones(hi - lo) if fault == "no_scale_left" else inv[off:off + hi - lo]
            yl = b[left][:nl, lo:hi] * f[None, :]
            A[:nl] += coef * (yl @ Z)
            gsum[:nl] += yl.sum(axis=1)
            tb += coef * Z.sum(axis=0)
            v = b[sub][:, lo:hi] * invS[None, lo:hi] - muS[:, None]
            total += w[i] / n[i] * float((v * v).sum())
        muL += (w[i] / w.sum()) * (gsum / n[i])
        if not (fault == HARMLESS or (fault == "no_centring_term" and i == len(x) - 1)):
            t += tb
        full_Z = np.vstack(Zs)
        if full_Z.shape[0] < n[i]:   # (the dropped cell still has its projection in the fit's record)
            full_Z = np.vstack([full_Z, invS[-1:, None] * (b[sub][:, -1:].T @ R) - (muS @ R)[None, :]])
        pcs.append(full_Z)
    UL = (A - np.outer(muL, t)) / (s if fault == "divide_by_s" else s ** 2)[None, :]
    rotation, centers = np.zeros((G_all, R.shape[1])), np.zeros(G_all)
    where = np.sort(sub) if fault == "sorted_subset" else sub
    rotation[where], centers[where] = R, muS
    rotation[left], centers[left] = UL, muL
    return {"rotation": rotation, "centers": centers, "d": s, "pcs": pcs, "var_total": total / len(x),
            "var_explained": s ** 2 / len(x)}


def assembly_ok(subset1, fit, fit_S):
    """The subset rows of the full record are the fit's rows, by index and bit for bit (a row named twice: the later)."""
    sub = np.asarray(subset1, dtype=np.int64) - 1
    last = {g: i for i, g in enumerate(sub.tolist())}
    rows = np.array(sorted(last)), np.array([last[g] for g in sorted(last)])
    return bool(np.array_equal(fit["rotation"][rows[0]], fit_S["rotation"][rows[1]]) and
                np.array_equal(fit["centers"][rows[0]], fit_S["centers"][rows[1]]))


# ---------------------------------------------------------------------------------------------- cases
class Case:
    def __init__(self, G_all, nS, sizes, d, weights=None, cos_norm=False, iters=1, zero_subset=None, rank=12, seed=0):
        self.G_all, self.nS, self.sizes, self.d, self.weights, self.cos_norm, self.iters = G_all, nS, sizes, d, weights, cos_norm, iters
        self.zero_subset, self.rank, self.seed = zero_subset, rank, seed
        self.G = nS   # (what pca_ref's width / fixed_count_f64 see)

    def kwargs(self):
        return {"d": self.d, "weights": self.weights, "cos_norm": self.cos_norm}


# Leftover tiles are 64 genes, the cells of a block go 32 a step and split at 4096 cells a block; the subspace is 64
# columns a half.  zero_subset=(b, c): cell c of batch b is zero on the subset rows and not on the others (scale 1e8).
CASES = {
    "a": Case(130, 64, (70, 257, 300), 10, weights=(1.0, 3.0, 0.5), cos_norm=True, iters=2),   # one full tile + 2 genes
    "b": Case(65, 64, (1, 2, 63, 70), 10, iters=1),                       # one leftover gene; batches of 1 and 2 cells
    "c": Case(191, 128, (257, 513), 80, cos_norm=True, iters=2),          # 63 genes; 16 columns in the second half
    "d": Case(249, 128, (4100, 300), 120, weights=False, iters=1),        # two cell splits; 121 genes; 56 columns
    "e": Case(130, 64, (31, 33, 64, 65), 57, iters=1),                    # 64 subset rows < the block of 128: host path
    "f": Case(130, 64, (70, 257, 300), 10, weights=(1.0, 3.0, 0.5), cos_norm=True, iters=2, zero_subset=(1, 100)),
}
DEVICE = ["a", "b", "c", "d", "f"]


@functools.lru_cache(maxsize=None)
def case(name):
    """(Case, batches, subset1): the subset is a fixed scattered, UNSORTED choice of rows (1-based); its rows are drawn as
    pca_ref.case draws them (low-rank signal + noise + a per-gene offset per batch, shifted under cos_norm), the others
    are half that signal and more noise."""
    c = CASES[name]
    rng = np.random.default_rng([c.G_all, c.nS, c.d, sum(c.sizes), c.seed])
    subset1 = rng.permutation(c.G_all)[:c.nS] + 1
    assert np.any(np.diff(subset1) < 0)
    sub, left = split_rows(c.G_all, subset1)
    load = rng.standard_normal((c.G_all, c.rank)) * np.linspace(3.0, 1.0, c.rank)
    out = []
    for i, n in enumerate(c.sizes):
        sig = load @ rng.standard_normal((c.rank, n))
        x = sig + 0.3 * rng.standard_normal((c.G_all, n))
        x[left] = 0.5 * sig[left] + rng.standard_normal((left.size, n))
        x += 0.4 * i * rng.standard_normal((c.G_all, 1)) + (3.0 if c.cos_norm else 0.0)
        out.append(x)
    if c.zero_subset is not None:
        out[c.zero_subset[0]][sub, c.zero_subset[1]] = 0.0
    for m in out:
        m.setflags(write=False)
    subset1.setflags(write=False)
    return c, out, subset1


@functools.lru_cache(maxsize=None)
def reference(name):
    c, B, subset1 = case(name)
    return exact(B, subset1, c.weights, c.cos_norm)


# ---------------------------------------------------------------------------------------------- the host path, literally
def planted_case(seed=0, G_all=90, nS=40, sizes=(120, 150, 90), d=5):
    """Batches whose subset rows have d directions of strength 12, 10, 8, ... over noise of 0.05: the top d singular
    values of the scaled matrix are separated from each other and from the rest by a large fraction of themselves."""
    rng = np.random.default_rng([seed, G_all, nS])
    subset1 = rng.permutation(G_all)[:nS] + 1
    dirs = np.linalg.qr(rng.standard_normal((G_all, d)))[0]
    strength = 12.0 - 2.0 * np.arange(d)
    out = []
    for i, n in enumerate(sizes):
        f = rng.standard_normal((d, n)) * strength[:, None]
        out.append(dirs @ f + 0.05 * rng.standard_normal((G_all, n)) + 0.2 * i + 2.0)
    return out, subset1, d


def literal(batches, subset1, weights, cos_norm, d):
    """R/multiBatchPCA.R:211-258, 401-432 word for word in float64: scaled = centred / sqrt(n_b / w_b) side by side,
    svd, rotation[subset.row,] <- u, leftover.u = sweep(left.scaled %*% v, 2, d, "/"), var.explained = d^2 / nbatches,
    var.total = sum(scaled^2) / nbatches.  Also returns what literal_bounds needs."""
    x = [np.asarray(b, dtype=np.float64) for b in batches]
    sub, left = split_rows(x[0].shape[0], subset1)
    n = [b.shape[1] for b in x]
    w = pca_ref.weight_vector(n, weights)
    sc = [pca_ref.scales(b[sub], cos_norm) for b in x]

    def process(rows):
        y = [b[rows] * s[None, :] for b, s in zip(x, sc)]
        centers = sum(wb / w.sum() * yb.mean(axis=1) for wb, yb in zip(w, y))
        scaled = np.hstack([(yb - centers[:, None]) / np.sqrt(nb / wb) for yb, nb, wb in zip(y, n, w)])
        return centers, scaled

    cen, scaled = process(sub)
    u, sv, vt = np.linalg.svd(scaled, full_matrices=False)
    cenL, left_scaled = process(left)
    rotation, centers = np.zeros((x[0].shape[0], d)), np.zeros(x[0].shape[0])
    rotation[sub], centers[sub] = u[:, :d], cen
    rotation[left], centers[left] = (left_scaled @ vt[:d].T) / sv[None, :d], cenL
    return {"rotation": rotation, "centers": centers, "d": sv[:d], "var_explained": sv[:d] ** 2 / len(x),
            "var_total": float((scaled ** 2).sum()) / len(x), "scaled": scaled, "left_scaled": left_scaled, "all_d": sv}


def literal_bounds(lit, d):
    """2-norm bounds on  column_j(host U_L) -+ column_j(literal U_L),  |host d_j^2 - literal d_j^2| / B  and
    |host var_total - literal var_total|.

    Write A (|S| x N) for the scaled subset matrix, L for the scaled leftover matrix, (u_j, d_j, v_j) for A's exact
    triplets, gap_j for the distance of d_j to the nearest other singular value and gapl_j for that of d_j^2 among the
    squares.  Both sides evaluate  L v / d  for an approximate pair:
      literal  (v^, d^) from LAPACK's SVD, which is the exact SVD of A + E, |E|_2 <= p u |A|_2 (LAPACK Users' Guide 4.9,
               "Error bounds for the singular value decomposition"; p a modest function of the shape, max(|S|, N) here):
               |d^ - d_j| <= e_s = p u |A|_2,   |v^ - v_j|_2 <= sqrt(2) e_s / gap_j      (ibid.; the guide's angle bound)
      host     (A^T r / d~, d~), r an eigenvector of the Gram matrix formed in float64, G^ = A A^T + F with
               |F|_2 <= (N + 3) u |A|_F^2 (an N-term dot product and the coef product per element), solved by LAPACK's
               symmetric eigensolver with backward error |S| u |G|_2 (ibid. 4.7):  e_g = (N + 3 + |S|) u |A|_F^2,
               |d~^2 - d_j^2| <= e_g,   |r - u_j|_2 <= sqrt(2) e_g / gapl_j,
               |A^T r / d~ - v_j|_2 <= |A|_2 sqrt(2) e_g / (gapl_j d_j) + e_g / d_j^2   (to first order)
    so with  |L x / d - L v_j / d_j|_2 <= |L|_2 (|x - v_j|_2 / d_j + |d - d_j| / d_j^2):
      column bound = |L|_2 / d_j ( sqrt(2) e_s / gap_j + e_s / d_j  +  |A|_2 sqrt(2) e_g / (gapl_j d_j) + 2 e_g / d_j^2 )
                     + the two products' own roundings, (N + |S| + 8) u | |L| |A|^T |_F / d_j^2 + (N + 3) u |L|_F / d_j
    (the first: the host identity's allowance in norm, |P| <= |L| |A|^T |r| entrywise with |r|_2 = 1, Q = 0 exactly;
    the second: the literal's N-term product, the root of its scaling and the sweep).
      d_j^2 / B:  (2 d_j e_s + e_s^2 + e_g) / B.
      var_total:  both are sums of the same |S| N squares of values that agree to 4 u |.|: (|S| N + 8) u |A|_F^2 / B is
      each one's distance from exact in any order of summation; twice that."""
    A, L, sv = lit["scaled"], lit["left_scaled"], lit["all_d"]
    nS, N = A.shape
    nb = int(round(float(sv[0] ** 2 / lit["var_explained"][0])))
    A2, AF2, L2 = sv[0], float((A ** 2).sum()), np.linalg.norm(L, 2)
    e_s = max(nS, N) * U * A2
    e_g = (N + 3 + nS) * U * AF2
    cols = np.zeros(d)
    for j in range(d):
        others = np.delete(sv, j)
        gap = np.abs(others - sv[j]).min()
        gapl = np.abs(others ** 2 - sv[j] ** 2).min()
        dj = sv[j]
        cols[j] = L2 / dj * (np.sqrt(2) * e_s / gap + e_s / dj + A2 * np.sqrt(2) * e_g / (gapl * dj) + 2 * e_g / dj ** 2)
        cols[j] += (N + nS + 8) * U * np.linalg.norm(np.abs(L) @ np.abs(A).T) / dj ** 2 + (N + 3) * U * np.linalg.norm(L) / dj
    return {"columns": cols, "var_explained": (2 * sv[:d] * e_s + e_s ** 2 + e_g) / nb,
            "var_total": 2 * (nS * N + 8) * U * AF2 / nb}
