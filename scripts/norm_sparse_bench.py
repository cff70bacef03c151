"""multiBatchNorm() host to host on the same synthetic counts, once dense and once sparse (CSC): 4 batches of 20 000
genes x 25 000 cells at about 5 % density by default (16 GB dense).  Warm-up runs first, then the median wall time of the
timed runs and the median stage_ms of each form, as one JSON line.

    python scripts/norm_sparse_bench.py [--genes G] [--cells N] [--batches B] [--density D] [--runs R] [--warmup W]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import batchelor_amd as bx  # noqa: E402


def make_batches(G, N, B, density, seed=1):
    """Per batch a CSC matrix of integer counts: a tile of 512 cells drawn at the density asked for (every cell with a
    count in row 0) and repeated along the cells with a multiplier per repeat, so that 2e9 values take no minutes to draw."""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(B):
        w = min(N, 512)
        tile = (rng.random((G, w)) < density) * rng.geometric(0.4 / (1 + 0.5 * b), (G, w)).astype(np.float64)
        tile[0] += 1
        tile = sp.csc_matrix(tile)
        reps = [tile[:, :min(w, N - a)] * float(1 + (a // w) % 3) for a in range(0, N, w)]
        out.append(sp.hstack(reps, format="csc"))
    return out


def timed(batches, runs, warmup):
    walls, stages = [], []
    for i in range(warmup + runs):
        t0 = time.perf_counter()
        res = bx.multiBatchNorm(*batches)
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            walls.append(dt)
            stages.append(res.stats["stage_ms"])
        del res
    return float(np.median(walls)), {k: float(np.median([s[k] for s in stages])) for k in stages[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=20000)
    ap.add_argument("--cells", type=int, default=25000)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--density", type=float, default=0.05)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    S = make_batches(a.genes, a.cells, a.batches, a.density)
    nnz = int(sum(m.nnz for m in S))
    sparse_ms, sparse_stages = timed(S, a.runs, a.warmup)
    D = [np.asfortranarray(m.toarray()) for m in S]
    dense_ms, dense_stages = timed(D, a.runs, a.warmup)
    print(json.dumps({"genes": a.genes, "cells": a.cells, "batches": a.batches, "nnz": nnz,
                      "density": nnz / (a.genes * a.cells * a.batches), "dense_bytes": int(sum(x.nbytes for x in D)),
                      "sparse_bytes": 12 * nnz + 8 * a.batches * (a.cells + 1), "runs": a.runs, "warmup": a.warmup,
                      "dense_ms": dense_ms, "sparse_ms": sparse_ms, "dense_stage_ms": dense_stages,
                      "sparse_stage_ms": sparse_stages}))


if __name__ == "__main__":
    main()
