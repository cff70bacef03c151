"""Per-stage device time of one mnnCorrect(var.adj=TRUE) run in gene space (default: 4 batches x 20 000 cells x 2 000
genes), and the CPU restatement's adjust_shift_variance time on a sample of the last merge's cells, scaled up.

    python scripts/mnn_correct_probe.py [--cells 20000] [--batches 4] [--genes 2000] [--sample 16]

With --sparse DENSITY the same matrices, every value kept with that probability, go through the dense call and through
the sparse call (scipy CSC in, expanded on the device), alternated in one process: one warm-up each, then --repeats timed
calls each, wall clock around the whole call, host to host.  --subset N restricts the correction to N rows
(correct_all=False).  The dense call is left out where its matrices would not fit into the host's free memory.

    python scripts/mnn_correct_probe.py --sparse 0.1
    python scripts/mnn_correct_probe.py --genes 20000 --subset 2000 --sparse 0.05 --repeats 1
"""
import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import batchelor_amd as bx  # noqa: E402
from oracle import fastmnn_oracle as orc  # noqa: E402


def _free_host_bytes():
    try:
        for line in open("/proc/meminfo"):
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) * 1024
    except OSError:
        pass
    return None


def sparse_against_dense(a):
    """--sparse: host-to-host wall time of the dense call and of the sparse call over the same matrices."""
    rng = np.random.default_rng(0)
    G, n, B = a.genes, a.cells, a.batches
    base = rng.normal(size=(G, 8))
    S = []
    for i in range(B):   # one dense batch at a time: only the CSC is kept
        x = np.abs(base @ rng.normal(size=(8, n)) + rng.normal(scale=0.3, size=(G, n)) + 0.5 * i * rng.normal(size=(G, 1)))
        x *= rng.random((G, n)) < a.sparse
        S.append(sp.csc_matrix(x))
        del x
    kw = {}
    if a.subset:
        kw = dict(subset_row=np.sort(rng.choice(G, a.subset, replace=False)) + 1, correct_all=False)
    dense_bytes = 8 * G * n * B
    sparse_bytes = sum(12 * m.nnz + 8 * (m.shape[1] + 1) for m in S)
    print(f"mnnCorrect {B} x {n} cells x {G} genes at density {a.sparse}"
          + (f", {a.subset} subset rows, correct_all=False" if a.subset else "") + f", {a.repeats} timed calls each after a warm-up")
    print(f"  upload: dense {dense_bytes / 1e6:.1f} MB, sparse {sparse_bytes / 1e6:.1f} MB")
    free = _free_host_bytes()
    D = None
    if free is not None and 2.5 * dense_bytes > free:
        print(f"  dense call: not measured, its matrices take {dense_bytes / 1e9:.1f} GB of the host's {free / 1e9:.1f} GB free")
    else:
        D = [np.asfortranarray(m.toarray()) for m in S]
    calls = {"sparse": lambda: bx.mnnCorrect(*S, **kw)}
    if D is not None:
        calls["dense"] = lambda: bx.mnnCorrect(*D, **kw)
    times = {k: [] for k in calls}
    for fn in calls.values():
        fn()  # warm-up
    for _ in range(a.repeats):   # alternated
        for name, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    for name, t in times.items():
        print(f"  {name:6s} median {np.median(t):9.1f} ms, spread (max - min) {max(t) - min(t):8.1f} ms, "
              f"calls {' '.join(f'{v:.1f}' for v in t)}")
    if D is not None:
        over = np.median(times["sparse"]) - np.median(times["dense"])
        spread = max(times["dense"]) - min(times["dense"])
        print(f"  sparse median - dense median {over:+.1f} ms; the dense call's spread {spread:.1f} ms: "
              + ("within" if over <= spread else "NOT within") + " the bound")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=20000)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--sample", type=int, default=16)
    ap.add_argument("--sparse", type=float, default=None, metavar="DENSITY")
    ap.add_argument("--subset", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if a.sparse is not None:
        return sparse_against_dense(a)
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
