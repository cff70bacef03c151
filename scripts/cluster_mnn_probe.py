"""Stage times of one clusterMNN() run (default: 4 batches x 200 000 cells x 2 000 genes, 30 clusters a batch), the bytes
per second of its two streaming passes against the HBM peak bench.py's roofline uses, and (--ref) the wall time of the
numpy restatement (tests/cluster_mnn_ref.py) on the same input.

    python scripts/cluster_mnn_probe.py [--cells 200000] [--batches 4] [--genes 2000] [--clusters 30] [--reps 3] [--ref]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import batchelor_amd as bx  # noqa: E402

HBM_PEAK = 8e12  # bytes / s, as in bench.py's streaming roofline


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=200000)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--clusters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    G, n, B, K = a.genes, a.cells, a.batches, a.clusters
    means = rng.normal(size=(G, K))
    batches, clusters = [], []
    for b in range(B):
        lab = rng.integers(0, K, n)
        lab[:K] = np.arange(K)
        x = np.asfortranarray(means[:, lab])
        x += rng.normal(size=(n, G)).T
        x += (b > 0) * rng.normal(size=(G, 1))
        batches.append(x)
        clusters.append(lab)
    nbytes = 8.0 * G * n * B
    print(f"clusterMNN {B} x {n} cells x {G} genes, {K} clusters a batch ({nbytes / 1e9:.2f} GB)")
    for rep in range(a.reps):  # the first run warms up (code objects, staging ring, allocations)
        t0 = time.perf_counter()
        out = bx.clusterMNN(*batches, clusters=clusters)
        wall = time.perf_counter() - t0
        st = out.stats["stage_ms"]
        print(f"run {rep}: wall {wall * 1e3:.0f} ms; " + ", ".join(f"{k} {v:.2f} ms" for k, v in st.items()))
    for name in ("centroids", "projection"):
        rate = nbytes / (st[name] * 1e-3)
        print(f"  {name}: {rate / 1e12:.2f} TB/s read = {rate / HBM_PEAK:.1%} of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak")
    if a.ref:
        from tests import cluster_mnn_ref as ref
        t0 = time.perf_counter()
        want = ref.cluster_mnn(*batches, clusters=clusters)
        t = time.perf_counter() - t0
        p, q = out.corrected @ out.rotation.T, want.corrected @ want.rotation.T
        print(f"restatement (numpy, CPU): wall {t:.1f} s; corrected @ rotation.T max rel diff "
              f"{np.abs(p - q).max() / np.abs(q).max():.2e}")


if __name__ == "__main__":
    main()
