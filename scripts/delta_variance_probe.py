"""mnnDeltaVariance() at a user's size (default: 4 batches x 100 000 cells x 2 000 genes, 6.4 GB), with the pairs of the
three merge steps taken from fastMNN() on the same data: the HIP-event time of the two pair passes (the gather), the bytes
they must move (2 P G 8 per pass and step), what share of the HBM rate that is, the host-to-host time of the call, and
(--ref) the numpy restatement (tests/delta_variance_ref.py) on the same input, gene block by gene block as the reference
walks its rowAutoGrid, on --threads host threads.

--sparse DENSITY [DENSITY ...]: the same workload and pairs with every entry kept with that probability, through three
paths that alternate after a warm-up of each, in this process: (a) the batches as scipy.sparse CSC through the sparse
handle; (b) the same CSC batches densified on the host (`.toarray()`) and given to the dense handle -- the only route for
such data before the sparse handle existed; (c) the dense handle on batches that are dense already.  Per path the
host-to-host times and the HIP-event time of the pair passes; for (a) the bytes its passes must move, counted from the
pairs' column lengths at 12 bytes per stored entry and pass.

    python scripts/delta_variance_probe.py [--cells 100000] [--batches 4] [--genes 2000] [--reps 4] [--cos-norm] [--ref]
                                           [--threads 16] [--sparse 0.05 0.2]
"""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import batchelor_amd as bx  # noqa: E402
from batchelor_amd import _lib  # noqa: E402

COPY_BW = 6.29e12  # bytes / s a plain copy reaches on this part
HBM_SPEC = 8.0e12  # bytes / s, data sheet


def make(G, n, B, seed=0):
    """Four latent populations, noise and a per-batch shift: batches that share populations, so that MNN pairs exist."""
    rng = np.random.default_rng(seed)
    base = rng.normal(size=(G, 4))
    out = []
    for b in range(B):
        x = np.empty((G, n), order="F")
        shift = b * rng.normal(size=(G, 1))
        for a in range(0, n, 20000):
            m = min(20000, n - a)
            x[:, a:a + m] = np.abs(base @ rng.normal(size=(4, m)) + rng.normal(scale=0.3, size=(G, m)) + shift)
        out.append(x)
    return out


def restatement_by_gene_block(batches, pairs, threads, block=50):
    """.compute_mnn_variance over row blocks (blockApply(x, ..., grid=rowAutoGrid(x)), :145), `threads` blocks at a time."""
    from tests import delta_variance_ref as ref
    G = batches[0].shape[0]

    def one(g0):
        rows = slice(g0, min(G, g0 + block))
        x = np.concatenate([b[rows] for b in batches], axis=1)
        return g0, ref.compute_mnn_variance(x, pairs)

    mean = np.empty((G, len(pairs)))
    total = np.empty((G, len(pairs)))
    with ThreadPoolExecutor(threads) as pool:
        for g0, (xvar, xmean) in pool.map(one, range(0, G, block)):
            for s in range(len(pairs)):
                mean[g0:g0 + block, s] = xmean[s]
                total[g0:g0 + block, s] = xvar[s]
    return mean, total


def sparse_paths(batches, pairs, density, reps, seed=1):
    """The three paths at one density; prints what the module docstring lists."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    t0 = time.perf_counter()
    csc, nnz_col = [], []
    for x in batches:
        c = sp.csc_matrix(np.where(rng.random(x.shape) < density, x, 0.0))
        csc.append(c)
        nnz_col.append(np.diff(c.indptr))
    kept = [c.toarray(order="F") for c in csc]                       # path (c)'s input: dense already
    nnz_col = np.concatenate(nnz_col).astype(np.int64)
    stored = int(nnz_col.sum())
    print(f"--- density {density}: {stored} stored entries of {sum(x.size for x in batches)} "
          f"({12.0 * stored / 1e9:.2f} GB as CSC, {8.0 * sum(x.size for x in batches) / 1e9:.2f} GB dense); made in "
          f"{time.perf_counter() - t0:.0f} s", flush=True)
    entries = sum(int(nnz_col[np.asarray(l) - 1].sum() + nnz_col[np.asarray(r) - 1].sum()) for l, r in pairs)
    nbytes = 2 * 12.0 * entries                                      # two passes

    def path_a():
        return bx.mnnDeltaVariance(*csc, pairs=pairs)

    def path_b():
        return bx.mnnDeltaVariance(*[c.toarray(order="F") for c in csc], pairs=pairs)

    def path_c():
        return bx.mnnDeltaVariance(*kept, pairs=pairs)

    paths = (("a: sparse handle", path_a), ("b: toarray() + dense handle", path_b), ("c: dense handle, dense input", path_c))
    wall = {name: [] for name, _ in paths}
    passes = {name: [] for name, _ in paths}
    last = {}
    for rep in range(reps + 1):                                      # round 0 warms every path up
        for name, fn in paths:
            t0 = time.perf_counter()
            out = fn()
            t = time.perf_counter() - t0
            st = out.stats["stage_ms"]
            print(f"round {rep} {name}: host to host {t * 1e3:.0f} ms; " + ", ".join(f"{k} {v:.2f}" for k, v in st.items()),
                  flush=True)
            if rep > 0:
                wall[name].append(t)
                passes[name].append(st["pair_passes"] * 1e-3)
            last[name] = out
    a, b, c = (name for name, _ in paths)
    for name in (a, b, c):
        w = np.asarray(wall[name]) * 1e3
        print(f"{name}: host to host median {np.median(w):.0f} ms, fastest {w.min():.0f} ms, spread {w.max() - w.min():.0f} ms; "
              f"pair passes fastest {min(passes[name]) * 1e3:.2f} ms", flush=True)
    ka = min(passes[a])
    print(f"(a) pair passes: {ka * 1e3:.2f} ms for {nbytes / 1e9:.3f} GB that must move ({entries} entries of the pairs' columns "
          f"x 12 bytes x 2 passes) = {nbytes / ka / 1e12:.3f} TB/s = {nbytes / ka / COPY_BW:.1%} of the plain-copy figure",
          flush=True)
    print(f"kernel-level ratio (a) / (c), pair passes: {ka / min(passes[c]):.2f}", flush=True)
    gain = np.median(wall[b]) - np.median(wall[a])
    spread = max(wall[b]) - min(wall[b])
    print(f"acceptance at this density: (a) is faster than (b) host to host by {gain * 1e3:.0f} ms (medians), the spread of (b) "
          f"is {spread * 1e3:.0f} ms: {'met' if gain > spread else 'NOT met'}; slowest (a) {max(wall[a]) * 1e3:.0f} ms, fastest "
          f"(b) {min(wall[b]) * 1e3:.0f} ms", flush=True)
    sa, sc = last[a], last[c]
    rel = max(float((np.abs(ta.total - tc.total) / tc.total).max()) for ta, tc in zip(sa.per_step, sc.per_step))
    print(f"(a) against (c): means bitwise equal {all(np.array_equal(ta.mean, tc.mean) for ta, tc in zip(sa.per_step, sc.per_step))}, "
          f"max rel diff of the totals {rel:.2e}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--cos-norm", action="store_true")
    ap.add_argument("--ref", action="store_true")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--sparse", type=float, nargs="+", default=[], metavar="DENSITY")
    a = ap.parse_args()
    G, n, B = a.genes, a.cells, a.batches
    _lib.require_gpu()
    t0 = time.perf_counter()
    batches = make(G, n, B)
    print(f"mnnDeltaVariance, {B} x {n} cells x {G} genes ({8.0 * G * n * B / 1e9:.2f} GB); input made in "
          f"{time.perf_counter() - t0:.0f} s", flush=True)
    t0 = time.perf_counter()
    pairs = bx.fastMNN(*batches).merge_info.pairs
    counts = [int(len(l)) for l, _ in pairs]
    print(f"fastMNN: {time.perf_counter() - t0:.1f} s; pairs per merge step {counts}", flush=True)
    nbytes = 2 * sum(2.0 * P * G * 8 for P in counts)  # two passes

    best_kernel, best_wall, out = float("inf"), float("inf"), None
    for rep in range(a.reps):  # the first run warms up (code objects, staging ring, allocations)
        del out
        t0 = time.perf_counter()
        out = bx.mnnDeltaVariance(*batches, pairs=pairs, cos_norm=a.cos_norm)
        wall = time.perf_counter() - t0
        st = out.stats["stage_ms"]
        print(f"run {rep}: host to host {wall * 1e3:.0f} ms; " + ", ".join(f"{k} {v:.2f}" for k, v in st.items()), flush=True)
        if rep > 0 or a.reps == 1:
            best_kernel, best_wall = min(best_kernel, st["pair_passes"] * 1e-3), min(best_wall, wall)
    print(f"pair passes: {best_kernel * 1e3:.2f} ms (fastest of the warm runs) for {nbytes / 1e9:.2f} GB that must move = "
          f"{nbytes / best_kernel / 1e12:.2f} TB/s = {nbytes / best_kernel / COPY_BW:.0%} of the plain-copy figure "
          f"({COPY_BW / 1e12:.2f} TB/s), {nbytes / best_kernel / HBM_SPEC:.0%} of the data sheet's {HBM_SPEC / 1e12:.0f} TB/s",
          flush=True)
    print(f"host to host: {best_wall * 1e3:.0f} ms (fastest of the warm runs), upload {st['upload']:.0f} ms of it", flush=True)
    again = bx.mnnDeltaVariance(*batches, pairs=pairs, cos_norm=a.cos_norm)
    print("bitwise equal to the run before:", bool(np.array_equal(again.total, out.total) and np.array_equal(again.mean, out.mean)),
          flush=True)

    if a.ref:
        if a.cos_norm:
            raise SystemExit("--ref times the pair statistics only: run it without --cos-norm")
        steps = [(np.asarray(l), np.asarray(r)) for l, r in pairs]
        t0 = time.perf_counter()
        mean, total = restatement_by_gene_block(batches, steps, a.threads)
        t = time.perf_counter() - t0
        dm = max(float(np.abs(mean[:, s] - out.per_step[s].mean).max()) for s in range(len(steps)))
        dt = max(float((np.abs(total[:, s] - out.per_step[s].total) / total[:, s]).max()) for s in range(len(steps)))
        print(f"restatement (numpy, {a.threads} threads over gene blocks): {t:.1f} s = {t / best_wall:.0f} x the device call "
              f"host to host, {t / best_kernel:.0f} x the pair passes; max abs diff of the means {dm:.2e}, max rel diff of the "
              f"totals {dt:.2e}", flush=True)

    for density in a.sparse:
        if a.cos_norm:
            raise SystemExit("--sparse compares the pair statistics: run it without --cos-norm")
        sparse_paths(batches, pairs, density, max(1, a.reps - 1))


if __name__ == "__main__":
    main()
