"""The gene-variance handles (bmx_genevar_*, bmx_genevar_sparse_*) at a user's size: one batch of 20 000 genes x 200 000
cells by default (32 GB of FP64 dense; about 5 % of it stored as CSC), streamed through the handle in blocks.  A batch never
has to exist on the host either: a tile of cells is drawn once and sent again and again with the block width the Python
layer would choose, which moves the same bytes.  One warm-up run, then the median of the timed runs, as one JSON line:
the handle's stage_ms (upload wall, kernels by HIP events, run wall), the host-to-host wall time, and the rates
    kernel_read_once_GBps   the block buffers' bytes / kernel time (each sweep of the two reads them once)
    kernel_two_sweeps_GBps  twice that: what the kernels load, wherever the second sweep is served from
    host_to_host_GBps       the bytes sent / wall time, to hold against the host link

    python scripts/gene_var_time.py [--genes G] [--cells N] [--density D] [--runs R] [--form dense|csc|both]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from batchelor_amd import _lib  # noqa: E402
from batchelor_amd import model_gene_var as mgv  # noqa: E402


def stream_dense(G, N, tile):
    w = tile.shape[1]
    h = mgv._GeneVarHandle(G, 0)
    try:
        t0 = time.perf_counter()
        h._call("begin_batch", ctypes.c_int64(N))
        for a in range(0, N, w):
            m = min(w, N - a)
            h._call("add_block", _lib.f64p(tile), ctypes.c_int64(m))
        h.ncells.append(N)
        mean, total = h.run()
        wall = (time.perf_counter() - t0) * 1e3
        return wall, h.stage_ms(), float(total[:, 0].mean())
    finally:
        h.close()


def stream_csc(G, N, tile):
    w = tile.shape[1]
    nblocks, last = divmod(N, w)
    tail = tile[:, :last].tocsc() if last else None
    nnz = nblocks * tile.nnz + (tail.nnz if last else 0)
    h = mgv._SparseGeneVarHandle(G, 0)
    try:
        t0 = time.perf_counter()
        h._call("begin_batch", ctypes.c_int64(N), ctypes.c_int64(nnz))
        ip = tile.indptr.astype(np.int64)
        for _ in range(nblocks):
            h._add_csc_block(w, ip, tile.indices, tile.data)
        if last:
            h._add_csc_block(last, tail.indptr.astype(np.int64), tail.indices, tail.data)
        h.ncells.append(N)
        mean, total = h.run()
        wall = (time.perf_counter() - t0) * 1e3
        return wall, h.stage_ms(), float(total[:, 0].mean()), nnz
    finally:
        h.close()


def median_of(runs, fn):
    fn()  # warm-up: code objects, the pinned rings, the block buffers' first allocation
    got = [fn() for _ in range(runs)]
    walls = [g[0] for g in got]
    stages = {k: float(np.median([g[1][k] for g in got])) for k in got[0][1]}
    return float(np.median(walls)), float(min(walls)), float(max(walls)), stages, got[0]


def rates(nbytes, wall_ms, stages):
    return {"kernel_read_once_GBps": nbytes / stages["kernels"] / 1e6,
            "kernel_two_sweeps_GBps": 2 * nbytes / stages["kernels"] / 1e6,
            "host_to_host_GBps": nbytes / wall_ms / 1e6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=20000)
    ap.add_argument("--cells", type=int, default=200000)
    ap.add_argument("--density", type=float, default=0.05)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--form", default="both", choices=("dense", "csc", "both"))
    a = ap.parse_args()
    _lib.require_gpu()
    G, N = a.genes, a.cells
    rng = np.random.default_rng(1)
    out = {"genes": G, "cells": N, "runs": a.runs}
    if a.form in ("dense", "both"):
        w = max(mgv.CHUNK, mgv.BLOCK_BYTES // (8 * G) // mgv.CHUNK * mgv.CHUNK)
        tile = np.asfortranarray(5.0 + rng.standard_normal((G, min(w, N))))
        wall, lo, hi, stages, _ = median_of(a.runs, lambda: stream_dense(G, N, tile))
        nbytes = 8 * G * N
        out["dense"] = {"block_cells": int(tile.shape[1]), "bytes": nbytes, "wall_ms": wall, "wall_ms_min_max": [lo, hi],
                        "stage_ms": stages, **rates(nbytes, wall, stages)}
    if a.form in ("csc", "both"):
        per_cell = max(1, int(12 * a.density * G))
        w = max(mgv.CHUNK, mgv.BLOCK_BYTES // per_cell // mgv.CHUNK * mgv.CHUNK)
        w = min(w, N)
        dense_tile = np.where(rng.random((G, min(w, 4096))) < a.density, 5.0 + rng.standard_normal((G, min(w, 4096))), 0.0)
        small = sp.csc_matrix(dense_tile)
        tile = sp.hstack([small] * -(-w // small.shape[1]), format="csc")[:, :w].tocsc()
        tile.sort_indices()
        tile = sp.csc_matrix((tile.data.astype(np.float64), tile.indices.astype(np.int32), tile.indptr), shape=tile.shape)
        wall, lo, hi, stages, first = median_of(a.runs, lambda: stream_csc(G, N, tile))
        nnz = first[3]
        nbytes = 12 * nnz + 8 * (N + 1)
        out["csc"] = {"block_cells": int(w), "nnz": int(nnz), "density": nnz / (G * N), "bytes": nbytes, "wall_ms": wall,
                      "wall_ms_min_max": [lo, hi], "stage_ms": stages, **rates(nbytes, wall, stages)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
