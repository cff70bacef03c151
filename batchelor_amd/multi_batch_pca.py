"""multiBatchPCA on the device (default) or on the host (BASELINE.json north_star: "multiBatchPCA stays on the
reference CPU path"; kept as `multiBatchPCA_host`), and the device cosineNorm / projection steps on either side of it.

multiBatchPCA follows R/multiBatchPCA.R:211-322: grand mean of the batch means (weighted), each centred batch scaled
by 1/sqrt(n_b / w_b), left singular vectors u of the scaled genes x cells matrix, projection of the UNSCALED centred
batches on u.  Instead of an SVD of the genes x N matrix this host implementation accumulates the genes x genes Gram
matrix batch by batch (N only enters through blocked GEMMs, so 10^5..10^6 cells never have to be held scaled) and
takes its top eigenvectors -- the same subspace and, up to sign, the same vectors.
"""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np
import scipy.sparse as sp

from . import _lib
from ._handle import ResidentHandle
from .inputs import all_sparse, canonical_csc, check_same_dim, check_same_rows, csc_block_width, subset_index, unpack_batches

# Sparse batches that the device path cannot take (multiBatchPCA's docstring) are made dense for the host path; beyond
# this many bytes of dense float64 over all batches the call is refused instead.
DENSIFY_CAP_BYTES = 8 << 30


def cosineNorm(x, mode="matrix", subset_row=None):
    """cosineNorm(x, mode=c("matrix", "all", "l2norm"), subset.row=NULL) (R/cosineNorm.R:53-82) on the GPU; x is genes x
    cells.  With subset_row (1-based integers or a logical mask; we have no row names) x is subset first (:54-56): the
    norms are over those rows and the matrix returned has only them.  A scipy.sparse x stays on the host (one pass over
    its stored entries, less work than their transfer): the matrix comes back as canonical CSC, a zero stays a zero."""
    if mode not in ("matrix", "all", "l2norm"):
        raise ValueError("'arg' should be one of 'matrix', 'all', 'l2norm'")
    if sp.issparse(x):
        return _cosine_norm_sparse(x, mode, subset_row)
    idx = subset_index(subset_row, np.asarray(x).shape[0])
    if idx is not None:
        x = np.asarray(x)[idx.astype(np.int64) - 1]
    _lib.require_gpu()
    x = _lib.as_f(x)
    G, n = x.shape
    l2 = np.zeros(n, dtype=np.float64)
    mat = None if mode == "l2norm" else np.zeros((G, n), dtype=np.float64, order="F")
    _lib.check(_lib.lib().bmx_cosine_norm(_lib.f64p(x), G, n, _lib.f64p(l2), None if mat is None else _lib.f64p(mat)))
    if mode == "l2norm":
        return l2
    return mat if mode == "matrix" else {"matrix": mat, "l2norm": l2}


def _cosine_norm_sparse(x, mode, subset_row):
    c = canonical_csc(x)[0]
    idx = subset_index(subset_row, c.shape[0])
    if idx is not None:
        c = canonical_csc(c[idx.astype(np.int64) - 1])[0]
    l2 = np.sqrt(np.asarray(c.multiply(c).sum(axis=0), dtype=np.float64).ravel())
    if mode == "l2norm":
        return l2
    scale = 1.0 / np.maximum(1e-8, l2)
    mat = sp.csc_matrix((c.data * np.repeat(scale, np.diff(c.indptr)), c.indices.copy(), c.indptr.copy()), shape=c.shape)
    return mat if mode == "matrix" else {"matrix": mat, "l2norm": l2}


def _list_weights(tree, current=1.0):
    out = []
    share = current / len(tree)
    for item in tree:
        if isinstance(item, (list, tuple)):
            out.extend(_list_weights(item, share))
        else:
            out.append((item, share))
    return out


def _weight_vector(ncells, weights):
    """.construct_weight_vector (R/multiBatchPCA.R:299-334)."""
    n = np.asarray(ncells, dtype=np.float64)
    if weights is None or weights is True:
        return np.ones_like(n)
    if weights is False:
        return n.copy()
    if isinstance(weights, (list, tuple)) and any(isinstance(w, (list, tuple)) for w in weights):
        pairs = _list_weights(weights)
        if sorted(int(i) for i, _ in pairs) != list(range(1, n.size + 1)):
            raise ValueError("invalid integer indices in tree-like 'weights'")
        out = np.zeros_like(n)
        for i, w in pairs:
            out[int(i) - 1] = w
        return out
    w = np.asarray(weights, dtype=np.float64)
    if w.size != n.size:
        raise ValueError("'length(weights)' should be the same as number of entries in '...'")
    return w


class _ResidentPCA(ResidentHandle):
    """What DevicePCA and DeviceSparsePCA share: fit() and project() on a handle whose PCA runs on _fit_rows rows."""

    def __init__(self, n_rows, device=0, *create_args):
        _lib.require_gpu()
        super().__init__(n_rows, device, *create_args)
        self.d = 0
        self.iters_used = 0
        self.residual = float("nan")

    @property
    def _fit_rows(self):
        return self.G

    def fit(self, d=50, tol=1e-9, max_iters=500, iters=None):
        """tol: relative Ritz residual at which the iteration stops (raises if max_iters applications of the operator do
        not reach it; the handle is fitted all the same).  iters=N: the fixed-count form of round 2 (N plain subspace
        iterations, no test).  A fit refused for another reason leaves the handle unfitted: project() raises."""
        centers = np.zeros(self._fit_rows)
        rotation = np.zeros((self._fit_rows, d), order="F")
        sdev = np.zeros(d)
        out = (_lib.f64p(centers), _lib.f64p(rotation), _lib.f64p(sdev))
        if iters is not None:
            rc = self._entry("fit")(self._h, int(d), int(iters), *out)
            self.iters_used, self.residual = int(iters), float("nan")
        else:
            used, res = ctypes.c_int32(0), ctypes.c_double(0.0)
            rc = self._entry("fit_tol")(self._h, int(d), ctypes.c_double(float(tol)), int(max_iters), *out,
                                        ctypes.byref(used), ctypes.byref(res))
            self.iters_used, self.residual = used.value, res.value
        self.d = int(d)   # before the status is looked at: a run that missed its tolerance has fitted the handle with d
        _lib.check(rc)
        return {"rotation": np.ascontiguousarray(rotation), "centers": centers, "d": sdev,
                "iters_used": self.iters_used, "residual": self.residual}

    def project(self, b):
        out = np.zeros((self.ncells[b], self.d), order="F")
        self._call("project", int(b), _lib.f64p(out))
        return np.ascontiguousarray(out)


class DevicePCA(_ResidentPCA):
    """bmx_pca_t: the batches (genes x cells) stay in HBM; fit() = multiBatchPCA (R/multiBatchPCA.R:211-322) by
    Chebyshev-filtered subspace iteration on the FP64 matrix cores, run until the Ritz residual is below `tol`;
    project(b) = crossprod(cosineNorm(x_b) - centers, rotation)."""
    PREFIX = "bmx_pca"

    def _check_rows(self, x):
        if x.ndim != 2 or x.shape[0] != self.G:
            raise ValueError("number of rows is not the same across batches")

    def add_batch(self, x, weight=1.0, cos_norm=False):
        x = _lib.as_f(x)
        self._check_rows(x)
        self._upload(x, None, ctypes.c_double(float(weight)), 1 if cos_norm else 0)

    def begin_batch(self, n, weight=1.0, cos_norm=False):
        """Announce a batch of n cells whose columns follow in blocks (add_block), so that it never has to exist on the
        host in one piece."""
        self._call("begin_batch", ctypes.c_int64(int(n)), ctypes.c_double(float(weight)), 1 if cos_norm else 0)
        self.ncells.append(int(n))

    def add_block(self, x_block):
        x_block = _lib.as_f(x_block)
        self._check_rows(x_block)
        self._call("add_block", _lib.f64p(x_block), ctypes.c_int64(x_block.shape[1]))

    def genes(self, n_left):
        """The streaming pass over the n_left genes outside subset.row, on this fitted PCA (DevicePCAGenes)."""
        return DevicePCAGenes(self, n_left)


class DevicePCAGenes:
    """bmx_pca_genes_t: multiBatchPCA's get.all.genes / get.variance (R/multiBatchPCA.R:401-432) for a DevicePCA that
    holds the subset.row rows and has been fitted.  The rows outside the subset go through in column blocks, batch by batch
    in the order the batches were added, and are not kept on the device; finish() returns their centres and rotation rows.
    The wrapper keeps its DevicePCA alive; a fit() or a new batch on it makes every later call here an error."""

    def __init__(self, pca, n_left):
        self.pca = pca
        self.n_left = int(n_left)
        self._h = ctypes.c_void_p()
        lib = _lib.lib()
        lib.bmx_pca_genes_destroy.argtypes = [ctypes.c_void_p]
        lib.bmx_pca_genes_destroy.restype = None
        _lib.check(lib.bmx_pca_genes_create(ctypes.c_int32(self.n_left), pca._h, ctypes.byref(self._h)))

    def begin_batch(self, b):
        _lib.check(_lib.lib().bmx_pca_genes_begin_batch(self._h, ctypes.c_int32(int(b))))

    def add_block(self, x_left_block):
        """The next cells of the batch begun last: n_left x cells."""
        x_left_block = _lib.as_f(x_left_block)
        if x_left_block.ndim != 2 or x_left_block.shape[0] != self.n_left:
            raise ValueError("number of rows is not the same across batches")
        _lib.check(_lib.lib().bmx_pca_genes_add_block(self._h, _lib.f64p(x_left_block),
                                                      ctypes.c_int64(x_left_block.shape[1])))

    def finish(self):
        """(centers [n_left], rotation [n_left x d]) of the leftover genes."""
        centers = np.zeros(self.n_left)
        rotation = np.zeros((self.n_left, self.pca.d), order="F")
        _lib.check(_lib.lib().bmx_pca_genes_finish(self._h, _lib.f64p(centers), _lib.f64p(rotation)))
        return centers, np.ascontiguousarray(rotation)

    def total_variance(self):
        """sum_b (w_b / n_b) |C_b|_F^2 over the rows the DevicePCA holds: var.total times the number of batches."""
        out = ctypes.c_double(0.0)
        _lib.check(_lib.lib().bmx_pca_genes_total_variance(self._h, ctypes.byref(out)))
        return out.value

    def close(self):
        if self._h:
            _lib.lib().bmx_pca_genes_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sparse_row_segment():
    """Stored entries of a gene row that one wave of the sparse PCA's by-gene pass adds (bmx_dev_get
    "pca_sparse_row_segment"; needs no device): a row with more entries is cut into segments of this length."""
    return _lib.dev_get("pca_sparse_row_segment")


class DeviceSparsePCA(_ResidentPCA):
    """bmx_pca_sparse_t: DevicePCA for batches kept in HBM as CSC.  The handle holds n_rows rows of every batch, of which
    the first n_rows_pca are the rows the PCA runs on (the subset in the caller's order) and the others the genes outside
    the subset, ascending; they stay resident, so genes() needs no second pass over the host's data."""
    PREFIX = "bmx_pca_sparse"
    BLOCK_BYTES = 1 << 28   # a batch goes to the device in column blocks of about this many bytes of stored entries

    def __init__(self, n_rows, n_rows_pca=None, device=0):
        self.n_pca = int(n_rows if n_rows_pca is None else n_rows_pca)
        super().__init__(n_rows, device, ctypes.c_int32(self.n_pca))

    @property
    def _fit_rows(self):
        return self.n_pca

    def add_batch(self, c, weight=1.0, cos_norm=False, block_cells=None):
        """c: canonical CSC (inputs.canonical_csc), n_rows x cells.  block_cells: cells per uploaded block (None: as many
        as hold about BLOCK_BYTES of stored entries, 12 bytes each); the results do not depend on it."""
        if c.ndim != 2 or c.shape[0] != self.G:
            raise ValueError("number of rows is not the same across batches")
        per = csc_block_width(c, self.BLOCK_BYTES) if block_cells is None else max(1, int(block_cells))
        self._upload_csc(c, per, ctypes.c_double(float(weight)), 1 if cos_norm else 0)

    def add_block(self, m, indptr, indices, data):
        """The next m cells of the batch begun last: indptr [m + 1] int64 relative to the block, int32 rows, float64."""
        self._add_csc_block(m, indptr, indices, data)

    def genes(self):
        """(centers [n_rows - n_rows_pca], rotation [n_rows - n_rows_pca x d]) of the rows outside the subset."""
        n_left = self.G - self.n_pca
        centers = np.zeros(n_left)
        rotation = np.zeros((n_left, self.d), order="F")
        self._call("genes", _lib.f64p(centers), _lib.f64p(rotation))
        return centers, np.ascontiguousarray(rotation)

    def total_variance(self):
        """sum_b (w_b / n_b) |C_b|_F^2 over the PCA rows: var.total times the number of batches."""
        out = ctypes.c_double(0.0)
        self._call("total_variance", ctypes.byref(out))
        return out.value


def device_pca_takes(n_rows, n_cells, d):
    """Whether the blocked subspace iteration takes a PCA of this shape: at least as many rows as its block of 64 / 128
    vectors, more cells than that (over all batches), d <= 120."""
    width = 64 if d <= 56 else 128
    return d <= 120 and n_rows >= width and n_cells > width


def _split_rows(subset_row, G):
    """(0-based subset rows in the caller's order, 0-based rows outside it ascending); (None, empty) without a subset."""
    idx = subset_index(subset_row, G)
    if idx is None:
        return None, np.zeros(0, dtype=np.int64)
    sub = idx.astype(np.int64) - 1
    keep = np.ones(G, dtype=bool)
    keep[sub] = False
    return sub, np.flatnonzero(keep)


def _all_genes(rec, G, sub, left, centers_left, rotation_left):
    """rotation / centers over all G rows (R/multiBatchPCA.R:408-414): the subset rows assigned by index -- a row named
    twice takes the later one, as R's `rotation[subset.row,] <- u` does -- and the others from the leftover pass."""
    rotation = np.zeros((G, rec["rotation"].shape[1]))
    centers = np.zeros(G)
    rotation[sub] = rec["rotation"]
    centers[sub] = rec["centers"]
    rotation[left] = rotation_left
    centers[left] = centers_left
    rec["rotation"], rec["centers"] = rotation, centers


_UPLOAD_BYTES = 1 << 28   # a column block of gathered rows on its way to the device


def multiBatchPCA(*batches, d=50, weights=None, cos_norm=False, tol=1e-9, max_iters=500, iters=None, device=0,
                  return_pcs=True, l2=None, block=65536, subset_row=None, get_all_genes=False, get_variance=False):
    """multiBatchPCA(..., d=, weights=, subset.row=, get.all.genes=, get.variance=) (R/multiBatchPCA.R:140-258) on the
    device.  Batches are genes x cells; with cos_norm the cosine normalisation of fastMNN (R/fastMNN.R:348-351) is applied
    on the fly.
    Returns {"rotation", "centers", "d", "weights", "iters_used", "residual", "path"} plus "pcs": the list of cells x d
    projections.

    subset_row (1-based integers or a logical mask): the PCA runs on those rows, gathered on the host block by block --
    the call is the call on x[subset_row], cosine norms included (they are taken over the subset, R/fastMNN.R:348-351).
    get_all_genes: "rotation" and "centers" cover every row of the input; the rows outside the subset are streamed through
    the device once (DevicePCAGenes) and never gathered whole (R/multiBatchPCA.R:401-414).  Without a subset, or with one
    that leaves no row out, it changes nothing.  get_variance: "var_explained" = d^2 / nbatches and "var_total"
    (:422-432).  Not taken: d=NA, preserve.single, a character subset.row (there are no row names), deferred, BSPARAM.

    The device path iterates until the relative Ritz residual is <= tol (the reference's irlba stops at 1e-5 on the
    singular triplets, R/multiBatchPCA.R:386-393) and raises when max_iters passes do not get there.  Inputs the blocked
    iteration cannot take -- fewer genes or cells than its block of 64 / 128 vectors, d > 120, data of rank below the
    block -- go to multiBatchPCA_host (north_star keeps multiBatchPCA on the host path anyway), as does a call in
    round 1's form with per-cell norms `l2=` (and its `block=`).

    Batches that are all scipy.sparse objects (a mixture with dense ones is a TypeError) go up as canonical CSC and stay
    sparse in HBM (DeviceSparsePCA, "path": "device-sparse"): every batch as [x[subset_row]; the other rows, ascending] by
    one sparse row-indexing, so the leftover rows of get_all_genes are resident too and nothing is streamed; all the
    arguments above work as for dense batches.  Under the fallback conditions above the sparse batches are made dense
    for the host path; that is refused with a ValueError above DENSIFY_CAP_BYTES (8 GiB of float64 over all batches)."""
    batches = unpack_batches(batches)
    if len(batches) == 0:
        raise ValueError("at least one batch must be specified")
    sparse = all_sparse(batches, "multiBatchPCA")
    G_all = check_same_rows(batches) if sparse else check_same_dim(batches, byrow=False)
    sub, left = _split_rows(subset_row, G_all)
    G = G_all if sub is None else sub.size
    if not get_all_genes:
        left = left[:0]
    ncells = [(m if sparse else np.asarray(m)).shape[1] for m in batches]
    w = _weight_vector(ncells, weights)

    def host(reason):
        return _host_route(densify(batches, "multiBatchPCA") if sparse else batches, reason, d, weights, cos_norm, l2,
                           block, subset_row, sub, get_all_genes, get_variance, return_pcs)

    if l2 is not None:
        return host("per-cell norms given (round-1 signature)")
    if not device_pca_takes(G, sum(ncells), d):
        return host("fewer genes / cells than the device block, or d > 120")
    # what differs between the two device routes: the handle and how it is filled, and where the leftover rows come from
    if sparse:
        fill, leftovers, path = _fill_sparse, _resident_leftovers, "device-sparse"
        pca = DeviceSparsePCA(G + left.size, G, device)
    else:
        fill, leftovers, path = _fill_dense, _streamed_leftovers, "device"
        pca = DevicePCA(G, device)
    try:
        fill(pca, batches, w, ncells, sub, left, cos_norm)
        try:
            out = pca.fit(d=d, tol=tol, max_iters=max_iters, iters=iters)
        except _lib.BatchelorMI355XError as exc:
            if "rank below the subspace width" in str(exc):
                pca.close()
                return host("data of rank below the device block")
            raise
        out["weights"] = w
        out["path"] = path
        if return_pcs:
            out["pcs"] = [pca.project(b) for b in range(len(batches))]
        if left.size or get_variance:
            with leftovers(pca, batches, ncells, left) as (finish, total_variance):
                if left.size:
                    _all_genes(out, G_all, sub, left, *finish())
                if get_variance:
                    out["var_explained"] = out["d"] ** 2 / len(batches)
                    out["var_total"] = total_variance() / len(batches)
    finally:
        pca.close()
    return out


def _rows(m, which, lo, hi):
    """Columns [lo, hi) of the rows `which` (None: all) of a dense batch."""
    blk = np.asarray(m)[:, lo:hi]
    return blk if which is None else blk[which]


def _fill_dense(pca, batches, w, ncells, sub, left, cos_norm):
    """The subset rows of every batch into a DevicePCA, gathered on the host block by block."""
    for m, wi, n in zip(batches, w, ncells):
        if sub is None:
            pca.add_batch(m, weight=wi, cos_norm=cos_norm)
            continue
        pca.begin_batch(n, weight=wi, cos_norm=cos_norm)
        per = max(1, _UPLOAD_BYTES // (8 * pca.G))
        for lo in range(0, n, per):
            pca.add_block(_rows(m, sub, lo, lo + per))


def _fill_sparse(pca, batches, w, ncells, sub, left, cos_norm):
    """Every batch as [x[subset_row]; the other rows, ascending] into a DeviceSparsePCA."""
    order = None if sub is None else np.concatenate([sub, left])
    for m, wi in zip(batches, w):
        pca.add_batch(_csc_rows(m, order), weight=wi, cos_norm=cos_norm)


@contextlib.contextmanager
def _streamed_leftovers(pca, batches, ncells, left):
    """(finish, total_variance) of a DevicePCAGenes that the rows `left` of the dense batches have streamed through."""
    genes = pca.genes(left.size)
    try:
        if left.size:
            per = max(1, _UPLOAD_BYTES // (8 * left.size))
            for b, (m, n) in enumerate(zip(batches, ncells)):
                genes.begin_batch(b)
                for lo in range(0, n, per):
                    genes.add_block(_rows(m, left, lo, lo + per))
        yield genes.finish, genes.total_variance
    finally:
        genes.close()


@contextlib.contextmanager
def _resident_leftovers(pca, batches, ncells, left):
    """(finish, total_variance) of a DeviceSparsePCA: the leftover rows are resident."""
    yield pca.genes, pca.total_variance


def _host_route(batches, reason, d, weights, cos_norm, l2, block, subset_row, sub, get_all_genes, get_variance, return_pcs):
    """multiBatchPCA's record from the host path (dense batches), with the device's projection."""
    if l2 is not None:
        norms = l2
    else:
        norms = [cosineNorm(m, mode="l2norm", subset_row=subset_row) for m in batches] if cos_norm else None
    out, rot, cen = _multi_batch_pca_host(batches, d, weights, norms, block, subset_row, get_all_genes, get_variance)
    out.update(iters_used=0, residual=0.0, path="host: " + reason)
    if return_pcs:
        out["pcs"] = [project(np.asarray(m) if sub is None else np.asarray(m)[sub], rot, cen, cos_norm=norms is not None)
                      for m in batches]
    return out


def densify(batches, who):
    """scipy.sparse batches as dense float64 for a host path; refused above DENSIFY_CAP_BYTES over all batches."""
    need = sum(8 * int(m.shape[0]) * int(m.shape[1]) for m in batches)
    if need > DENSIFY_CAP_BYTES:
        raise ValueError(f"{who}: the host path needs the sparse batches dense, {need} bytes of float64; more than "
                         f"{DENSIFY_CAP_BYTES} bytes are not densified")
    return [np.asarray(m.toarray(), dtype=np.float64) for m in batches]


def _csc_rows(m, rows):
    """Batch m as canonical CSC with the rows `rows` (0-based, in that order, repeats allowed; None: all)."""
    c = canonical_csc(m)[0]
    return c if rows is None else canonical_csc(c[rows])[0]


def multiBatchPCA_host(*batches, d=50, weights=None, l2=None, block=65536, subset_row=None, get_all_genes=False,
                       get_variance=False):
    """Host PCA across batches (genes x cells each).  `l2` (optional list of per-cell norms) applies the cosine
    normalisation on the fly, so the normalised matrices are never materialised.

    Returns {"rotation": [G x d], "centers": [G], "d": singular values, "weights": w}.  Project with `project()`.

    subset_row, get_all_genes, get_variance: as multiBatchPCA (R/multiBatchPCA.R:401-432), in float64 numpy; `l2` then
    holds the norms over the subset rows (cosineNorm(x, "l2norm", subset_row=)) and scales every row.
    """
    return _multi_batch_pca_host(unpack_batches(batches), d, weights, l2, block, subset_row, get_all_genes, get_variance)[0]


def _multi_batch_pca_host(batches, d, weights, l2, block, subset_row, get_all_genes, get_variance):
    """multiBatchPCA_host's record, and the rotation and centres of the rows the PCA ran on (what projects them)."""
    if len(batches) == 0:
        raise ValueError("at least one batch must be specified")
    full = [np.asarray(b, dtype=np.float64) for b in batches]
    G_all = check_same_dim(full, byrow=False)
    sub, left = _split_rows(subset_row, G_all)
    mats = full if sub is None else [m[sub] for m in full]
    rec = _host_pca(mats, d, weights, l2, block)
    rot, cen = rec["rotation"], rec["centers"]
    w, nb = rec["weights"], len(mats)
    inv = [None if l2 is None else 1.0 / np.maximum(1e-8, np.asarray(l2[i], dtype=np.float64)) for i in range(nb)]
    if get_variance:
        total = 0.0
        for i, m in enumerate(mats):
            for lo in range(0, m.shape[1], block):
                c = m[:, lo:lo + block]
                c = (c if inv[i] is None else c * inv[i][None, lo:lo + block]) - cen[:, None]
                total += (w[i] / m.shape[1]) * float((c * c).sum())
        rec["var_explained"] = rec["d"] ** 2 / nb
        rec["var_total"] = total / nb
    if get_all_genes and left.size:
        # left.scaled %*% v swept by d, v = S_scaled^T u / d (R/multiBatchPCA.R:404-406): with Z_b = C_b^T u,
        # ( sum_b coef_b L_b diag(scale_b) Z_b  -  mu_L sum_b coef_b 1^T Z_b ) / d^2
        acc = np.zeros((left.size, rot.shape[1]))
        zsum = np.zeros(rot.shape[1])
        mu_left = np.zeros(left.size)
        for i, (m, f) in enumerate(zip(mats, full)):
            coef = w[i] / m.shape[1]
            gsum = np.zeros(left.size)
            for lo in range(0, m.shape[1], block):
                sc = 1.0 if inv[i] is None else inv[i][None, lo:lo + block]
                z = (m[:, lo:lo + block] * sc - cen[:, None]).T @ rot
                lb = f[:, lo:lo + block][left] * sc
                acc += coef * (lb @ z)
                zsum += coef * z.sum(axis=0)
                gsum += lb.sum(axis=1)
            mu_left += (gsum / m.shape[1]) * w[i]
        mu_left /= w.sum()
        _all_genes(rec, G_all, sub, left, mu_left, (acc - np.outer(mu_left, zsum)) / rec["d"] ** 2)
    return rec, rot, cen


def _host_pca(mats, d, weights, l2, block):
    """The PCA itself on float64 batches that all have the rows it runs on."""
    G = mats[0].shape[0]
    w = _weight_vector([m.shape[1] for m in mats], weights)
    inv = [None if l2 is None else 1.0 / np.maximum(1e-8, np.asarray(l2[i], dtype=np.float64)) for i in range(len(mats))]

    def cols(i, lo, hi):
        blk = mats[i][:, lo:hi]
        return blk if inv[i] is None else blk * inv[i][None, lo:hi]

    # pass 1: grand centre = weighted mean of the batch means (R/multiBatchPCA.R:268-281)
    grand = np.zeros(G)
    for i, m in enumerate(mats):
        s = np.zeros(G)
        for lo in range(0, m.shape[1], block):
            s += cols(i, lo, min(m.shape[1], lo + block)).sum(axis=1)
        grand += (s / m.shape[1]) * w[i]
    grand /= w.sum()
    if G > 4096:
        return _host_pca_lanczos(mats, inv, grand, w, d, block)
    # pass 2: Gram matrix of the scaled, centred data: sum_b (w_b / n_b) C_b C_b^T   (scaled = C_b / sqrt(n_b / w_b))
    gram = np.zeros((G, G))
    for i, m in enumerate(mats):
        for lo in range(0, m.shape[1], block):
            c = cols(i, lo, min(m.shape[1], lo + block)) - grand[:, None]
            gram += (w[i] / m.shape[1]) * (c @ c.T)
    evals, evecs = np.linalg.eigh(gram)
    order = np.argsort(evals)[::-1][:d]
    return {"rotation": np.ascontiguousarray(evecs[:, order]), "centers": grand,
            "d": np.sqrt(np.maximum(evals[order], 0.0)), "weights": w}


def _host_pca_lanczos(mats, inv, grand, w, d, block):
    """Many genes: the genes x genes Gram matrix is not formed (20 000 genes: 3.2 GB and a dense eigensolver of 1e13
    flops); its top d eigenpairs come from implicitly restarted Lanczos on the operator v -> sum_b (w_b/n_b) C_b (C_b^T v),
    run to machine precision -- the host analogue of the reference's default BSPARAM=IrlbaParam() (R/fastMNN.R:287).
    C_b = X_b diag(inv_b) - grand 1^T is never formed: the per-cell factors and the centring are applied to the vectors."""
    from scipy.sparse.linalg import LinearOperator, eigsh
    G = mats[0].shape[0]

    def matvec(v):
        v = np.asarray(v, dtype=np.float64).reshape(G)
        out = np.zeros(G)
        gv = float(grand @ v)
        for i, m in enumerate(mats):
            acc = np.zeros(G)
            zsum = 0.0
            for lo in range(0, m.shape[1], block):
                hi = min(m.shape[1], lo + block)
                blk = m[:, lo:hi]
                z = blk.T @ v                 # C_b^T v for these cells ...
                if inv[i] is not None:
                    z *= inv[i][lo:hi]
                z -= gv
                zsum += float(z.sum())
                acc += blk @ (z if inv[i] is None else z * inv[i][lo:hi])
            out += (w[i] / m.shape[1]) * (acc - grand * zsum)
        return out

    op = LinearOperator((G, G), matvec=matvec, dtype=np.float64)
    k = min(d, G - 1)
    evals, evecs = eigsh(op, k=k, which="LA", tol=0, ncv=min(G, max(3 * k, k + 32)),
                         v0=np.random.default_rng(0).standard_normal(G))
    order = np.argsort(evals)[::-1]
    return {"rotation": np.ascontiguousarray(evecs[:, order]), "centers": grand,
            "d": np.sqrt(np.maximum(evals[order], 0.0)), "weights": w}


def project(x, rotation, centers, cos_norm=True):
    """crossprod(cosineNorm(x) - centers, rotation) in one GPU pass over x (R/fastMNN.R:348-354 +
    R/multiBatchPCA.R:236-239).  x: genes x cells; returns cells x d."""
    _lib.require_gpu()
    x = _lib.as_f(x)
    rot = _lib.as_f(rotation)
    cen = np.ascontiguousarray(centers, dtype=np.float64)
    G, n = x.shape
    if rot.shape[0] != G or cen.size != G:
        raise ValueError("number of rows is not the same across batches")
    d = rot.shape[1]
    out = np.zeros((n, d), dtype=np.float64, order="F")
    _lib.check(_lib.lib().bmx_cosnorm_project(_lib.f64p(x), G, n, _lib.f64p(rot), d, _lib.f64p(cen),
                                              ctypes.c_int32(1 if cos_norm else 0), _lib.f64p(out)))
    return np.ascontiguousarray(out)
