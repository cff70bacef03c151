"""regressBatches(d=) at size, today's route against deferred=True, residuals=False: host-to-host time and peak host
memory of one call, in a process of its own per route (the peak is the process's).  Default: 2 batches of 5 000 genes x
100 000 cells, d = 50.

    python scripts/residual_pca_time.py --route today|deferred|operator [--genes G] [--cells N] [--batches B] [--d D]
                                        [--design P]

--design P: a design of an intercept and P - 1 random columns, all regressed out (P + 1 columns of the low-rank term);
without it the default design (rank one per batch).

--route operator: the time of one application of the operator, deferred (bmx_residual_pca_fit with a fixed count of
plain steps, the coefficient fit timed apart and taken off) against Pca::apply_operator on the same shape (bmx_pca_fit
with the same count on the downloaded residuals): (time of 9 steps - time of 1 step) / 8 for both.
Prints one JSON line.
"""
import argparse
import json
import os
import resource
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import batchelor_amd as bx  # noqa: E402
from batchelor_amd.multi_batch_pca import DevicePCA  # noqa: E402


def make_batches(G, N, B, seed=1):
    """Low-rank signal + noise + a per-batch offset; the noise is a tile repeated along the cells with a per-cell factor,
    so that 1e9 values do not take a minute to draw."""
    rng = np.random.default_rng(seed)
    load = rng.standard_normal((G, 60)) * np.linspace(3.0, 0.5, 60)
    tile = 0.3 * rng.standard_normal((G, 512))
    out = []
    for b in range(B):
        x = np.empty((G, N), dtype=np.float64, order="F")
        for a in range(0, N, 8192):
            w = min(8192, N - a)
            x[:, a:a + w] = load @ rng.standard_normal((60, w))
            x[:, a:a + w] += np.tile(tile, (1, w // 512 + 1))[:, :w] * rng.uniform(0.5, 1.5, w)
        x += 2.0 * rng.standard_normal((G, 1))
        out.append(x)
    return out


def rss_gb():
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1048576.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=("today", "deferred", "operator"), required=True)
    ap.add_argument("--genes", type=int, default=5000)
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--d", type=int, default=50)
    ap.add_argument("--design", type=int, default=0)
    a = ap.parse_args()
    X = make_batches(a.genes, a.cells, a.batches)
    N = a.cells * a.batches
    design = None
    if a.design:
        design = np.column_stack([np.ones(N), np.random.default_rng(2).standard_normal((N, a.design - 1))])
    bx.regressBatches(*[x[:256, :512] for x in X], d=5)   # warm-up: the library, the pinned rings
    rec = {"route": a.route, "genes": a.genes, "cells": a.cells, "batches": a.batches, "d": a.d, "design": a.design,
           "input_gb": sum(x.nbytes for x in X) / 2 ** 30, "rss_before_gb": rss_gb()}
    if a.route == "operator":
        def deferred(iters):
            return bx.regressBatches(*X, design=design, d=a.d, deferred=True, residuals=False, pca_iters=iters).stats["pca_fit_ms"]
        d1, d9 = deferred(1), deferred(9)
        res = bx.regressBatches(*X, design=design)
        sizes = np.cumsum([x.shape[1] for x in X])[:-1]
        pca = DevicePCA(a.genes)
        for part in np.split(res.corrected, sizes, axis=1):
            pca.add_batch(part)
        del res

        def plain(iters):
            t0 = time.perf_counter()
            pca.fit(d=a.d, iters=iters)
            return (time.perf_counter() - t0) * 1e3
        p1, p9 = plain(1), plain(9)
        pca.close()
        rec.update(deferred_fit_ms=[d1, d9], pca_fit_ms=[p1, p9], deferred_ms_per_application=(d9 - d1) / 8,
                   pca_ms_per_application=(p9 - p1) / 8)
    else:
        t0 = time.perf_counter()
        if a.route == "today":
            res = bx.regressBatches(*X, design=design, d=a.d)
        else:
            res = bx.regressBatches(*X, design=design, d=a.d, deferred=True, residuals=False)
        rec.update(seconds=time.perf_counter() - t0, peak_rss_gb=rss_gb(), pcs_shape=list(res.pcs.shape),
                   stage_ms=res.stats["stage_ms"], pca=None if res.pca is None else
                   {k: res.pca[k] for k in ("iters_used", "residual", "path")}, pca_fit_ms=res.stats.get("pca_fit_ms"))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
