"""multiBatchNorm() at size: 4 batches of 20 000 genes x 50 000 cells by default, the median of 5 runs after a warm-up.

Prints stage_ms, the bytes each kernel stage moves over its time, the host-to-host time, the transfer floor that
bmx_linear_fetch measures for the same bytes (upload + plain download, no kernel) and the time of the numpy
restatement.  The achieved bandwidths stand beside the measured HBM rate of an MI355X (6.29 TB/s, float4 copy).

    python scripts/multi_batch_norm_time.py [--genes G] [--cells N] [--batches B] [--runs R] [--no-numpy]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import batchelor_amd as bx  # noqa: E402
from batchelor_amd.linear_correct import _LinearHandle  # noqa: E402
from tests import multi_batch_norm_ref as ref  # noqa: E402

HBM_TBS = 6.29


def make_batches(G, N, B, seed=1):
    """Counts with a depth factor per batch: a tile of negative-binomial draws repeated along the cells with a per-cell
    multiplier, so that 4e9 values do not take minutes to draw."""
    rng = np.random.default_rng(seed)
    mu = 2.0 ** rng.uniform(-2, 7, G)
    out = []
    for b in range(B):
        tile = rng.negative_binomial(4, 4 / (4 + (1 + 0.5 * b) * mu[:, None]), (G, min(N, 512))).astype(np.float64)
        tile[0] += 1
        x = np.empty((G, N), dtype=np.float64, order="F")
        for a in range(0, N, tile.shape[1]):
            w = min(tile.shape[1], N - a)
            x[:, a:a + w] = tile[:, :w] * float(1 + (a // tile.shape[1]) % 3)
        out.append(x)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=20000)
    ap.add_argument("--cells", type=int, default=50000)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    X = make_batches(a.genes, a.cells, a.batches)
    nbytes = sum(x.nbytes for x in X)

    walls, stages = [], []
    for i in range(a.runs + 1):
        t0 = time.perf_counter()
        res = bx.multiBatchNorm(*X)
        dt = (time.perf_counter() - t0) * 1e3
        if i:  # the first run warms the pinned rings and the block cache
            walls.append(dt)
            stages.append(res.stats["stage_ms"])
        del res
    stage_ms = {k: float(np.median([s[k] for s in stages])) for k in stages[0]}

    floors = []
    for i in range(3):
        t0 = time.perf_counter()
        h = _LinearHandle(a.genes, 0)
        try:
            for x in X:
                h.add_batch(x, None)
            h.fetch()
        finally:
            h.close()
        if i:
            floors.append((time.perf_counter() - t0) * 1e3)

    # the statistics passes read every count twice (column sums, per-gene sums); the output pass reads and writes it once
    moved = {"statistics": 2 * nbytes, "output_kernels": 2 * nbytes}
    out = {"genes": a.genes, "cells": a.cells, "batches": a.batches, "count_bytes": nbytes, "stage_ms": stage_ms,
           "host_to_host_ms": float(np.median(walls)), "transfer_floor_ms": float(np.median(floors)),
           "hbm_roof_TBs": HBM_TBS,
           "achieved_TBs": {k: moved[k] / (stage_ms[k] * 1e-3) / 1e12 for k in moved}}
    if not a.no_numpy:
        t0 = time.perf_counter()
        ref.multi_batch_norm(*X)
        out["numpy_ms"] = (time.perf_counter() - t0) * 1e3
    print(json.dumps(out))


if __name__ == "__main__":
    main()
