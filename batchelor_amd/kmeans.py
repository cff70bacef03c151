"""kmeans(): R's kmeans(x, centers, iter.max, nstart, algorithm="Lloyd") on the device (csrc/kmeans.hip), and KmeansParam,
what bluster::KmeansParam stands for in clusterMNN(clusters=<BlusterParam>) (R/clusterMNN.R:199-221).

The observations go to the device once (bmx_kmeans_t) and stay there for every start and every iteration.  Random starts
are drawn on the host: np.random.default_rng(seed), one choice(n, K, replace=False) per start, in order.

Out of scope: Hartigan-Wong and MacQueen, k-means++, every other bluster method.
"""
from __future__ import annotations

import ctypes
import warnings
from dataclasses import dataclass
from typing import Callable, Optional, Union

import numpy as np

from . import _lib
from ._handle import ResidentHandle

MAX_CENTERS = 1024      # BMX_KMEANS_MAX_CENTERS
BLOCK_BYTES = 1 << 28   # observations above this size go to the device in blocks of about this many bytes


@dataclass
class KmeansResult:
    """What kmeans() returns, the fields named as in R."""
    cluster: np.ndarray        # 1-based int32 label per observation
    centers: np.ndarray        # K x d: the means of the returned labels
    withinss: np.ndarray       # per cluster: sum (x - c)^2
    tot_withinss: float
    size: np.ndarray           # members per cluster
    iter: int                  # assignments made
    converged: bool            # the last assignment changed no label
    stats: Optional[dict] = None   # "stage_ms": upload, assign, update, withinss, download; "start": the start kept (0-based)


@dataclass
class KmeansParam:
    """bluster::KmeansParam(centers, iter.max, nstart): `centers` is the number of clusters or a function of the number of
    observations that gives it; `seed` seeds the starts (R draws them from its global generator)."""
    centers: Union[int, Callable[[int], int]]
    iter_max: int = 10
    nstart: int = 1
    seed: int = 0

    def n_centers(self, n):
        k = self.centers(int(n)) if callable(self.centers) else self.centers
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
            raise ValueError("'centers' of a KmeansParam must be an integer or a function that returns one")
        return int(k)


class _KmeansHandle(ResidentHandle):
    """bmx_kmeans_t: the observations stay in HBM between the starts."""
    PREFIX = "bmx_kmeans"
    STAGES = ("upload", "assign", "update", "withinss", "download")

    def __init__(self, x, device, block_bytes=BLOCK_BYTES):
        """x: observations x dimensions, C-contiguous float64."""
        super().__init__(x.shape[1], device)
        n = int(x.shape[0])
        self.n = n
        block = n if block_bytes is None else max(1, int(block_bytes) // (8 * self.G))
        self._call("begin", ctypes.c_int64(n))
        for a in range(0, n, block):
            xb = x[a:a + block]
            self._call("add_block", _lib.f64p(xb), ctypes.c_int64(xb.shape[0]))

    def run(self, centers, iter_max):
        centers = np.ascontiguousarray(centers, dtype=np.float64)
        K = int(centers.shape[0])
        cluster = np.empty(self.n, dtype=np.int32)
        cen = np.empty((K, self.G), dtype=np.float64)
        size = np.empty(K, dtype=np.int32)
        wss = np.empty(K, dtype=np.float64)
        tot, it, conv = ctypes.c_double(0.0), ctypes.c_int32(0), ctypes.c_int32(0)
        self._call("run", _lib.f64p(centers), ctypes.c_int32(K), ctypes.c_int32(int(iter_max)), _lib.i32p(cluster),
                   _lib.f64p(cen), _lib.i32p(size), _lib.f64p(wss), ctypes.byref(tot), ctypes.byref(it), ctypes.byref(conv))
        return KmeansResult(cluster=cluster, centers=cen, withinss=wss, tot_withinss=float(tot.value), size=size,
                            iter=int(it.value), converged=bool(conv.value))


def _check_args(x, centers, iter_max, nstart):
    """The argument errors of kmeans() that need no device; returns (x, the matrix of centres or None, K)."""
    x = np.asarray(x)
    if x.ndim != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("'x' must be a matrix of observations x dimensions with at least one of each")
    if x.dtype.kind not in "fiub":
        raise ValueError("'x' must be numeric")
    if isinstance(iter_max, (bool, np.bool_)) or int(iter_max) != iter_max or iter_max < 1:
        raise ValueError("'iter_max' must be positive")
    if isinstance(nstart, (bool, np.bool_)) or int(nstart) != nstart or nstart < 1:
        raise ValueError("'nstart' must be a positive integer")
    n = x.shape[0]
    if isinstance(centers, (int, np.integer)) and not isinstance(centers, (bool, np.bool_)):
        K, init = int(centers), None
    else:
        init = np.asarray(centers, dtype=np.float64)
        if init.ndim != 2 or init.shape[1] != x.shape[1]:
            raise ValueError("must have same number of columns in 'x' and 'centers'")
        if nstart != 1:
            raise ValueError("'nstart' must be 1 when 'centers' is a matrix")
        K = init.shape[0]
    if K < 1:
        raise ValueError("number of cluster centres must be positive")
    if K > n:
        raise ValueError("more cluster centers than observations")
    if K > MAX_CENTERS:
        raise ValueError(f"kmeans takes at most {MAX_CENTERS} centers")
    return np.ascontiguousarray(x, dtype=np.float64), init, K


def start_indices(n, K, nstart=1, seed=0):
    """The rows (0-based) every start takes as its centres: default_rng(seed), one choice(n, K, replace=False) per start."""
    rng = np.random.default_rng(seed)
    return [rng.choice(int(n), int(K), replace=False) for _ in range(int(nstart))]


def kmeans(x, centers, iter_max=10, nstart=1, seed=0, device=0) -> KmeansResult:
    """kmeans(x, centers, iter.max, nstart, algorithm="Lloyd").  `x` is observations x dimensions; `centers` a K x d matrix
    of initial centres (nstart must then be 1) or the number K of rows of x drawn as centres for every start (see
    start_indices).  The start with the smallest tot_withinss is kept, the earliest on a tie.  Initial centres that are not
    distinct and a cluster left empty are errors; a run that has not converged after iter_max assignments is a warning."""
    x, init, K = _check_args(x, centers, iter_max, nstart)
    _lib.require_gpu()
    h = _KmeansHandle(x, device)
    try:
        if init is not None:
            best, kept = h.run(init, iter_max), 0
        else:
            best, kept = None, 0
            for s, idx in enumerate(start_indices(x.shape[0], K, nstart, seed)):
                res = h.run(x[idx], iter_max)
                if best is None or res.tot_withinss < best.tot_withinss:
                    best, kept = res, s
        stage_ms = h.stage_ms()
    finally:
        h.close()
    best.stats = {"stage_ms": stage_ms, "start": kept}
    if not best.converged:
        warnings.warn(f"did not converge in {int(iter_max)} iterations", stacklevel=2)
    return best
