"""make_snn_graph() host to host on 100 000 x 50 (synthetic Gaussian, decaying scales) at k = 10 and k = 20, type "rank": the whole
call, its graph kernels alone (HIP events around them, the library's "snn_graph_us"), find_knn alone on the same input, and as
the CPU comparator scipy.sparse's A @ A.T of the (n x n, k + 1 per row) membership matrix -- the "number" weights -- on at most
16 CPUs.  One step at a time, every step a child process of its own under its own time limit; the first step that fails or runs
out of time ends the run.  One JSON line per step, one for the run.

    python scripts/snn_bench.py [--n N] [--d D] [--runs R] [--warmup W] [--cpus C]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

CPUS = 16
for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = str(min(CPUS, int(os.environ.get(_v, CPUS))))

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_LIMIT_S = {"graph": 240, "knn": 240, "cpu": 420}


def data(n, d):
    rng = np.random.Generator(np.random.PCG64(20250314))
    return np.asfortranarray(rng.standard_normal((n, d)) / np.sqrt(1.0 + np.arange(d) / 5.0))


def spread(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def step_graph(a):
    import batchelor_amd as bx
    from batchelor_amd import _lib
    X = data(a.n, a.d)
    walls, kernels = [], []
    for i in range(a.warmup + a.runs):
        t0 = time.perf_counter()
        g = bx.make_snn_graph(X, a.k, type="rank")      # returns with the result on the host: the device is idle
        dt = (time.perf_counter() - t0) * 1e3
        if i >= a.warmup:
            walls.append(dt)
            kernels.append(_lib.dev_get("snn_graph_us") * 1e-3)
    return {"make_snn_graph": spread(walls), "graph_kernels": spread(kernels), "edges": int(g.first.size),
            "edges_per_cell": g.first.size / a.n, "most_edges_of_one_cell": int(np.bincount(g.first).max()),
            "spilled_cells": _lib.dev_get("snn_spilled_cells")}


def step_knn(a):
    import batchelor_amd as bx
    X = data(a.n, a.d)
    walls = []
    for i in range(a.warmup + a.runs):
        t0 = time.perf_counter()
        index, _ = bx.find_knn(X, a.k)
        dt = (time.perf_counter() - t0) * 1e3
        if i >= a.warmup:
            walls.append(dt)
    np.save(a.index_file, index)
    return {"find_knn": spread(walls)}


_A = _At = None      # the membership matrix and its transpose: set before the pool forks, so the workers inherit them


def _block_product(rows):
    r0, r1 = rows
    P = _A[r0:r1] @ _At
    return int(P.nnz), float(P.data.sum())


def step_cpu(a):
    """No device: the index is find_knn's of the step before."""
    import multiprocessing as mp
    import scipy.sparse as sp
    index = np.load(a.index_file)
    n, k = index.shape
    members = np.concatenate([np.arange(n)[:, None], index.astype(np.int64) - 1], axis=1)
    global _A, _At
    _A = sp.csr_matrix((np.ones(members.size), (np.repeat(np.arange(n), k + 1), members.ravel())), shape=(n, n))
    _At = _A.T.tocsr()
    cpus = min(a.cpus, CPUS)
    bounds = np.linspace(0, n, 4 * cpus + 1).astype(int)
    jobs = [(int(bounds[i]), int(bounds[i + 1])) for i in range(4 * cpus)]
    walls = []
    with mp.get_context("fork").Pool(cpus) as pool:
        for i in range(1 + a.runs):
            t0 = time.perf_counter()
            parts = pool.map(_block_product, jobs)
            dt = (time.perf_counter() - t0) * 1e3
            if i >= 1:
                walls.append(dt)
    nnz = sum(p[0] for p in parts)
    return {"scipy_A_At": spread(walls), "cpus": cpus, "edges": (nnz - n) // 2}


STEPS = {"graph": step_graph, "knn": step_knn, "cpu": step_cpu}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--d", type=int, default=50)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpus", type=int, default=CPUS)
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--k", type=int)
    ap.add_argument("--index-file")
    a = ap.parse_args()
    if a.step:
        out = STEPS[a.step](a)
        out.update({"step": a.step, "n": a.n, "d": a.d, "k": a.k, "runs": a.runs, "warmup": a.warmup})
        print(json.dumps(out))
        return 0
    results = []
    with tempfile.TemporaryDirectory() as tmp:
        for k in (10, 20):
            index_file = os.path.join(tmp, "index_k%d.npy" % k)
            for step in ("graph", "knn", "cpu"):
                cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--k", str(k), "--n", str(a.n), "--d", str(a.d),
                       "--runs", str(a.runs), "--warmup", str(a.warmup), "--cpus", str(a.cpus), "--index-file", index_file]
                try:
                    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=STEP_LIMIT_S[step])
                except subprocess.TimeoutExpired:
                    print(json.dumps({"step": step, "k": k, "error": "time limit of %d s" % STEP_LIMIT_S[step]}), flush=True)
                    return 1
                if p.returncode != 0:
                    print(json.dumps({"step": step, "k": k, "error": "exit status %d" % p.returncode}), flush=True)
                    return 1
                line = p.stdout.strip().splitlines()[-1]
                print(line, flush=True)
                results.append(json.loads(line))
    print(json.dumps({"snn_bench": results}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
