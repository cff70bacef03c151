"""Developer helper: multiBatchPCA on scipy.sparse batches kept sparse on the device against what the same data costs
when it has to be made dense first.  One shape per run, host to host:

    (a) multiBatchPCA(csc, csc, ...)                      the sparse path (DeviceSparsePCA)
    (b) toarray() on the host, then multiBatchPCA(dense)  what a caller had to do before; reported with and without
                                                          the time of the toarray()

and the time of one application of the operator on either handle, from fixed-count fits of 2 and 6 steps on batches that
are already resident ((t6 - t2) / 4: one operator application and the Cholesky QR 2 on the G x L block that follows it,
the latter the same kernels on both handles).

    python scripts/pca_sparse_bench.py --cells 50000 --genes 5000 --density 0.1 --d 10 --batches 2

Values are log-count-like and non-negative: log2(1 + a low-rank non-negative signal) at the stored entries.  One warm-up
call of each path, then --repeats timed calls; the median and the spread are printed as one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import batchelor_amd as bx  # noqa: E402
from batchelor_amd.inputs import canonical_csc  # noqa: E402


def synth(cells, genes, density, batches, rank=6, seed=0):
    """CSC batches with a rank-`rank` non-negative structure under the log, an entry stored where a uniform draw of
    (gene, cell) pairs lands (about cells * genes * density of them a batch)."""
    rng = np.random.default_rng(seed)
    load = np.abs(rng.standard_normal((genes, rank))) * np.linspace(3.0, 1.0, rank)
    out = []
    for b in range(batches):
        nnz = int(cells * genes * density)
        rows = rng.integers(0, genes, nnz, dtype=np.int32)
        cols = rng.integers(0, cells, nnz, dtype=np.int32)
        f = np.abs(rng.standard_normal((rank, cells)))
        acc = np.full(nnz, 0.2 * b)
        for k in range(rank):
            acc += load[rows, k] * f[k, cols]
        acc *= np.exp(0.5 * rng.standard_normal(nnz))     # per-entry noise: keeps the spectrum's tail off zero
        m = sp.coo_matrix((np.log2(1.0 + acc), (rows, cols)), shape=(genes, cells)).tocsc()
        m.sum_duplicates()
        out.append(m)
    return out


def timed(fn, repeats):
    fn()                                      # warm-up: allocations, first launches
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts)}


def per_application(make, d, repeats):
    """Seconds per application of the operator (+ one orthonormalisation) on a handle whose batches are resident."""
    h = make()
    try:
        t = {}
        for iters in (2, 6):
            t[iters] = timed(lambda: h.fit(d=d, iters=iters), repeats)["median_s"]
        return (t[6] - t[2]) / 4
    finally:
        h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--genes", type=int, default=5000)
    ap.add_argument("--density", type=float, default=0.1)
    ap.add_argument("--d", type=int, default=10)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1e-9)
    ap.add_argument("--iters", type=int, default=None, help="a fixed count of plain subspace steps in place of --tol")
    ap.add_argument("--cos-norm", action="store_true")
    ap.add_argument("--sparse-only", action="store_true", help="one warm-up and one sparse call, for a kernel trace")
    a = ap.parse_args()
    B = synth(a.cells, a.genes, a.density, a.batches)
    kw = dict(d=a.d, cos_norm=a.cos_norm, tol=a.tol, iters=a.iters)
    res = {"cells": a.cells, "genes": a.genes, "density": a.density, "d": a.d, "batches": a.batches,
           "stored_entries": [int(m.nnz) for m in B]}

    last = {}

    def sparse_call():
        last["sparse"] = bx.multiBatchPCA(*B, **kw)

    def dense_call_with_densify():
        last["dense"] = bx.multiBatchPCA(*[m.toarray() for m in B], **kw)

    if a.sparse_only:
        res["a_sparse"] = timed(sparse_call, 1)
        res["applications"] = [int(last["sparse"]["iters_used"])]
        print(json.dumps(res))
        return
    res["a_sparse"] = timed(sparse_call, a.repeats)
    res["b_densify_then_dense"] = timed(dense_call_with_densify, a.repeats)
    D = [np.asfortranarray(m.toarray()) for m in B]
    res["b_dense_only"] = timed(lambda: bx.multiBatchPCA(*D, **kw), a.repeats)
    res["paths"] = [last["sparse"]["path"], last["dense"]["path"]]
    res["applications"] = [int(last["sparse"]["iters_used"]), int(last["dense"]["iters_used"])]
    res["d_rel_diff"] = float(np.abs(last["sparse"]["d"] - last["dense"]["d"]).max() / last["dense"]["d"][0])

    def make_sparse():
        h = bx.DeviceSparsePCA(a.genes)
        for m in B:
            h.add_batch(canonical_csc(m)[0], cos_norm=a.cos_norm)
        return h

    def make_dense():
        h = bx.DevicePCA(a.genes)
        for m in D:
            h.add_batch(m, cos_norm=a.cos_norm)
        return h

    res["per_application_sparse_s"] = per_application(make_sparse, a.d, a.repeats)
    res["per_application_dense_s"] = per_application(make_dense, a.d, a.repeats)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
