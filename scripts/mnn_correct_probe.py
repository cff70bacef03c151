"""Per-stage device time of one mnnCorrect(var.adj=TRUE) run in gene space (default: 4 batches x 20 000 cells x 2 000
genes), and the CPU restatement's adjust_shift_variance time on a sample of the last merge's cells, scaled up.

    python scripts/mnn_correct_probe.py [--cells 20000] [--batches 4] [--genes 2000] [--sample 16]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import batchelor_amd as bx  # noqa: E402
from oracle import fastmnn_oracle as orc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=20000)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--sample", type=int, default=16)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    G, n, B = a.genes, a.cells, a.batches
    base = rng.normal(size=(G, 8))
    batches = [np.asfortranarray(np.abs(base @ rng.normal(size=(8, n)) + rng.normal(scale=0.3, size=(G, n))
                                        + 0.5 * i * rng.normal(size=(G, 1)))) for i in range(B)]
    t0 = time.perf_counter()
    out = bx.mnnCorrect(*batches)
    wall = time.perf_counter() - t0
    st = out.stage_ms
    print(f"mnnCorrect {B} x {n} cells x {G} genes, var.adj: wall {wall * 1e3:.0f} ms")
    for k, v in st.items():
        print(f"  {k:10s} {v:10.1f} ms")
    # asv pair stage: ~10 FP64 operations per (cell, streamed cell, gene), summed over the merges
    flops = sum(10.0 * n * (n * (m + 1) + n) * G for m in range(B - 1))
    print(f"  asv pair-stage work {flops:.2e} FP64 ops -> {flops / (st['asv'] * 1e-3) / 1e12:.1f} TFLOP/s over the asv stage")
    # the restatement's adjust_shift_variance on a sample of the last merge's right cells (its loop is per cell), scaled up
    left = np.asfortranarray(np.hstack([b for b in batches[:-1]]))
    right = batches[-1]
    vect = np.asfortranarray(rng.normal(size=(n, G)))
    cells = np.sort(rng.choice(n, a.sample, replace=False)).astype(np.int32)
    t0 = time.perf_counter()
    orc.adjust_shift_variance(left, right, vect, 0.1, np.arange(left.shape[1], dtype=np.int32),
                              np.arange(n, dtype=np.int32), cells=cells)
    t = time.perf_counter() - t0
    print(f"restatement asv, last merge: {t / a.sample * 1e3:.1f} ms a cell -> {t / a.sample * n:.1f} s for its {n} cells")


if __name__ == "__main__":
    main()
