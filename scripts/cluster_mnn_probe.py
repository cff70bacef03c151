"""Stage times of one clusterMNN() run (default: 4 batches x 200 000 cells x 2 000 genes, 30 clusters a batch), the bytes
per second of its two streaming passes against the HBM peak bench.py's roofline uses, and (--ref) the wall time of the
numpy restatement (tests/cluster_mnn_ref.py) on the same input.

    python scripts/cluster_mnn_probe.py [--cells 200000] [--batches 4] [--genes 2000] [--clusters 30] [--reps 3] [--ref]

--density D builds the batches with about that share of their entries stored and runs the call with both forms of the same
matrices, scipy.sparse CSC and the densified arrays, alternating; after a warm-up of each it prints every run and the
median of each form's wall time and upload / centroids / projection stage times.

    python scripts/cluster_mnn_probe.py --density 0.05 --cells 100000 --batches 2 --genes 20000 --clusters 100
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import batchelor_amd as bx  # noqa: E402

HBM_PEAK = 8e12  # bytes / s, as in bench.py's streaming roofline


def sparse_batch(rng, means, lab, density, shift):
    """A genes x cells CSC batch: per cell about density * genes stored rows (drawn with replacement, repeats dropped), the
    values |cluster mean + noise (+ the batch's per-gene shift)| + 0.1."""
    import scipy.sparse as sp
    G, n = means.shape[0], lab.size
    per = max(1, int(round(density * G)))
    rows = np.sort(rng.integers(0, G, size=(n, per), dtype=np.int32), axis=1)
    keep = np.ones(rows.shape, dtype=bool)
    keep[:, 1:] = rows[:, 1:] != rows[:, :-1]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(keep.sum(axis=1), out=indptr[1:])
    cols = np.repeat(np.arange(n), per).reshape(n, per)[keep]
    indices = rows[keep]
    data = np.abs(means[indices, lab[cols]] + rng.normal(size=indices.size) + shift[indices]) + 0.1
    return sp.csc_matrix((data, indices, indptr), shape=(G, n))


def sparse_and_dense(a):
    rng = np.random.default_rng(0)
    G, n, B, K = a.genes, a.cells, a.batches, a.clusters
    means = rng.normal(size=(G, K))
    sparse, clusters = [], []
    for b in range(B):
        lab = rng.integers(0, K, n)
        lab[:K] = np.arange(K)
        sparse.append(sparse_batch(rng, means, lab, a.density, (b > 0) * rng.normal(size=G)))
        clusters.append(lab)
    dense = [np.asfortranarray(c.toarray(order="F")) for c in sparse]
    stored = sum(c.nnz for c in sparse)
    print(f"clusterMNN {B} x {n} cells x {G} genes, {K} clusters a batch, density {stored / (G * n * B):.4f}: "
          f"{12.0 * stored / 1e9:.2f} GB as CSC, {8.0 * G * n * B / 1e9:.2f} GB dense")
    forms = {"sparse": sparse, "dense": dense}
    runs = {k: [] for k in forms}
    out = {}
    for rep in range(a.reps + 1):  # the first run of each form warms up (code objects, staging ring, allocations)
        for name, mats in forms.items():
            t0 = time.perf_counter()
            out[name] = bx.clusterMNN(*mats, clusters=clusters)
            wall = (time.perf_counter() - t0) * 1e3
            st = out[name].stats["stage_ms"]
            print(f"{name} run {rep}{' (warm-up)' if rep == 0 else ''}: wall {wall:.0f} ms; "
                  + ", ".join(f"{k} {v:.2f} ms" for k, v in st.items()))
            if rep:
                runs[name].append([wall, st["upload"], st["centroids"], st["projection"]])
    for name, r in runs.items():
        wall, up, cen, proj = np.median(np.asarray(r), axis=0)
        print(f"{name}: median of {len(r)}: wall {wall:.0f} ms, upload {up:.1f} ms, centroids {cen:.2f} ms, "
              f"projection {proj:.2f} ms")
    p, q = (o.corrected @ o.rotation.T for o in (out["sparse"], out["dense"]))
    print(f"sparse against dense: corrected @ rotation.T max rel diff {np.abs(p - q).max() / np.abs(q).max():.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=200000)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--clusters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref", action="store_true")
    ap.add_argument("--density", type=float, default=None)
    a = ap.parse_args()
    if a.density is not None:
        if not 0.0 < a.density <= 1.0:
            ap.error("--density takes a value in (0, 1]")
        return sparse_and_dense(a)
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
