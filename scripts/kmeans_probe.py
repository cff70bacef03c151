"""One Lloyd iteration of kmeans() by HIP events (the handle's stage_ms), assignment and centre update apart (default:
200 000 observations x 50 dimensions, 200 centres): the assignment against the 2 n K d flops of its products and the FP64
matrix peak of the data sheet, the update against two reads of the n d 8 bytes of the observations and the HBM peak
bench.py's roofline uses.

    python scripts/kmeans_probe.py [--n 200000] [--d 50] [--k 200] [--reps 5]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from batchelor_amd.kmeans import _KmeansHandle  # noqa: E402

HBM_PEAK = 8e12       # bytes / s, as in bench.py's streaming roofline
FP64_PEAK = 78.6e12   # flop / s, FP64 matrix (data sheet)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--d", type=int, default=50)
    ap.add_argument("--k", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n, d, K = a.n, a.d, a.k
    rng = np.random.default_rng(0)
    mu = rng.normal(scale=1.5, size=(K, d))
    x = mu[rng.integers(0, K, n)] + rng.normal(size=(n, d))
    init = x[rng.choice(n, K, replace=False)]
    flops, nbytes = 2.0 * n * K * d, 2.0 * n * d * 8
    print(f"kmeans {n} x {d}, {K} centres: one iteration = {flops / 1e9:.2f} GFLOP of products, "
          f"two reads of the observations = {nbytes / 1e6:.1f} MB")
    h = _KmeansHandle(x, 0)
    try:
        before = h.stage_ms()
        for rep in range(a.reps):  # the first run warms up (code objects, allocations)
            h.run(init, 1)         # one assignment, one update
            now = h.stage_ms()
            t_as, t_up = now["assign"] - before["assign"], now["update"] - before["update"]
            before = now
            print(f"run {rep}: assign {t_as:.3f} ms = {flops / t_as / 1e9:.2f} TFLOP/s = {flops / t_as / 1e-3 / FP64_PEAK:.1%} "
                  f"of the FP64 matrix peak; update {t_up:.3f} ms = {nbytes / t_up / 1e9:.3f} TB/s = "
                  f"{nbytes / t_up / 1e-3 / HBM_PEAK:.1%} of the HBM peak; withinss "
                  f"{now['withinss']:.3f} ms in all")
    finally:
        h.close()


if __name__ == "__main__":
    main()
