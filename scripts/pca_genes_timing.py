#!/usr/bin/env python
"""Developer helper (not bench.py): what the streaming pass over the genes outside subset.row costs at full size.

Default shape: 4 batches x 50 000 cells x 20 000 genes, 2 000 of them in the subset, d = 50.  The subset rows are made
resident and fitted (two fixed steps: the pass does not care how converged the rotation is); the 18 000 leftover rows
of every batch then go through DevicePCAGenes in column blocks.  The full leftover matrix (29 GB) is never built: one
block of random numbers is fed again and again, which costs the link, the staging ring and the kernels what real data
would.  Timed: the pass end to end (first add_block to finish), and the host's share of the same work -- the products
of multiBatchPCA_host's leftover loop (scale, L Z, gene sums) in numpy on the same blocks with the threads the process is
given.  The kernels' own time comes from a kernel trace of this script (run it under the profiler with --skip-host);
the pass minus the kernels is the time spent on the copy.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import batchelor_amd as bx  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--genes", type=int, default=20000)
    ap.add_argument("--subset", type=int, default=2000)
    ap.add_argument("--d", type=int, default=50)
    ap.add_argument("--block-mb", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    n_left = a.genes - a.subset
    per = max(1, (a.block_mb << 20) // (8 * n_left))
    block = np.asfortranarray(rng.standard_normal((n_left, min(per, a.cells))))
    load = rng.standard_normal((a.subset, 20))
    pca = bx.DevicePCA(a.subset)
    try:
        for _ in range(a.batches):
            pca.add_batch(np.asfortranarray(load @ rng.standard_normal((20, a.cells)) + rng.standard_normal((a.subset, a.cells)) + 3.0),
                          cos_norm=True)
        t0 = time.perf_counter()
        fit = pca.fit(d=a.d, iters=2)
        fit_s = time.perf_counter() - t0
        spans = [(lo, min(a.cells, lo + per)) for lo in range(0, a.cells, per)]

        def run():
            genes = pca.genes(n_left)
            try:
                t0 = time.perf_counter()
                for b in range(a.batches):
                    genes.begin_batch(b)
                    for lo, hi in spans:
                        genes.add_block(block[:, :hi - lo])
                fed = time.perf_counter() - t0
                genes.finish()
                return time.perf_counter() - t0, fed
            finally:
                genes.close()

        runs = [run() for _ in range(1 + a.repeats)][1:]     # the first allocates the buffers and the pinned ring
        pass_s = float(np.median([r[0] for r in runs]))
        out = {"batches": a.batches, "cells": a.cells, "genes": a.genes, "subset": a.subset, "d": a.d,
               "block_cells": per, "blocks": len(spans) * a.batches, "fit_2_steps_s": fit_s,
               "pass_s": pass_s, "pass_all_s": [r[0] for r in runs], "add_block_calls_s": float(np.median([r[1] for r in runs])),
               "leftover_gb": 8e-9 * n_left * a.cells * a.batches, "gb_per_s": 8e-9 * n_left * a.cells * a.batches / pass_s,
               "product_gflop": 2e-9 * n_left * a.cells * a.batches * a.d}
        if not a.skip_host:
            z = rng.standard_normal((block.shape[1], a.d))
            inv = rng.random(block.shape[1]) + 0.5
            acc, gsum = np.zeros((n_left, a.d)), np.zeros(n_left)
            t0 = time.perf_counter()
            for b in range(a.batches):
                for lo, hi in spans:
                    lb = block[:, :hi - lo] * inv[None, :hi - lo]
                    acc += 0.5 * (lb @ z[:hi - lo])
                    gsum += lb.sum(axis=1)
            out["host_product_s"] = time.perf_counter() - t0
            out["host_threads"] = os.environ.get("OMP_NUM_THREADS")
        print(json.dumps(out))
        assert np.all(np.isfinite(fit["d"]))
    finally:
        pca.close()


if __name__ == "__main__":
    main()
