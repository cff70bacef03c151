"""Stage times of rescaleBatches() (log base 2 and 10) and regressBatches() (default design and a design of p columns) at
clusterMNN's probe size (default: 4 batches x 200 000 cells x 2 000 genes, 12.8 GB), with, per kernel stage, the bytes per
second against the plain-copy figure and the FP64 operations per second against the vector peak; the host-to-host wall
time against the same bytes sent up and brought straight back (the floor) and (--ref) the numpy restatement
(tests/linear_correct_ref.py) on the same input (the baseline).  --variants adds the A/B runs of EXPERIMENTS.md.

    python scripts/linear_correct_probe.py [--cells 200000] [--batches 4] [--genes 2000] [--p 8] [--reps 2] [--ref]
                                           [--variants] [--only NAME]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import batchelor_amd as bx  # noqa: E402
from batchelor_amd import _lib, linear_correct as lc  # noqa: E402

COPY_BW = 6.29e12    # bytes / s a plain copy reaches on this part
FP64_PEAK = 78.6e12  # FP64 vector operations / s


def make(G, n, B, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for b in range(B):
        x = np.empty((G, n), order="F")
        for a in range(0, n, 20000):
            m = min(20000, n - a)
            x[:, a:a + m] = np.log2(rng.integers(0, 40 + 10 * b, (m, G)).T + 1.0)
        out.append(x)
    return out


def report(name, fn, reps, elements, ops1, ops2):
    """ops1 / ops2: FP64 operations per element of the two passes that are counted (adds, multiplies; None: the pass
    evaluates pow / exp2 / log, whose operation count is the library's, so only elements per second are given)."""
    out = None
    for rep in range(reps):  # the first run warms up (code objects, staging rings, allocations)
        del out
        t0 = time.perf_counter()
        out = fn()
        wall = time.perf_counter() - t0
        st = out.stats["stage_ms"]
        print(f"{name} run {rep}: wall {wall * 1e3:.0f} ms; " + ", ".join(f"{k} {v:.2f}" for k, v in st.items()), flush=True)
    for stage, nbytes, ops in (("first_pass", 8.0 * elements, ops1), ("second_pass_kernels", 16.0 * elements, ops2)):
        t = st[stage] * 1e-3
        line = f"  {stage}: {t * 1e3:.2f} ms, {nbytes / t / 1e12:.2f} TB/s = {nbytes / t / COPY_BW:.0%} of the copy figure, " \
               f"{elements / t / 1e12:.3f} T elements/s"
        if ops is not None:
            line += f", {ops * elements / t / 1e12:.2f} TFLOP/s = {ops * elements / t / FP64_PEAK:.1%} of the FP64 vector peak"
        print(line, flush=True)
    return out, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=200000)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--genes", type=int, default=2000)
    ap.add_argument("--p", type=int, default=8)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--ref", action="store_true")
    ap.add_argument("--variants", action="store_true")
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    G, n, B, p = a.genes, a.cells, a.batches, a.p
    _lib.require_gpu()
    batches = make(G, n, B)
    elements = float(G) * n * B
    print(f"linear corrections, {B} x {n} cells x {G} genes ({8 * elements / 1e9:.2f} GB in, as much out)", flush=True)
    rng = np.random.default_rng(1)
    ids = np.repeat(np.arange(B), n)
    design = np.concatenate([np.ones((B * n, 1)), (ids[:, None] == np.arange(1, B)[None]).astype(float),
                             rng.normal(size=(B * n, p - B))], axis=1)
    p16 = -(-p // 16) * 16
    cases = {
        "rescale base 2": (lambda: bx.rescaleBatches(*batches), None, None),
        "rescale base 10": (lambda: bx.rescaleBatches(*[x for x in batches], log_base=10), None, None),
        "regress default": (lambda: bx.regressBatches(*batches), 1.0, 1.0),
        f"regress p={p}": (lambda: bx.regressBatches(*batches, design=design), 2.0 * p16, 2.0 * p16 + 1.0),
    }
    walls, outs = {}, {}
    for name, (fn, o1, o2) in cases.items():
        if a.only and a.only != name:
            continue
        out, walls[name] = report(name, fn, a.reps, elements, o1, o2)
        outs[name] = out.corrected[:, ::997].copy()
        del out

    # the floor: the same bytes up through the staging ring and straight back through the download ring, no kernel
    floor = float("inf")
    for rep in range(a.reps + 1):
        t0 = time.perf_counter()
        h = lc._LinearHandle(G, 0)
        try:
            for x in batches:
                h.add_batch(x, None)
            back = h.fetch()
            st = h.stage_ms()
        finally:
            h.close()
        wall = time.perf_counter() - t0
        floor = min(floor, wall)
        print(f"floor run {rep}: wall {wall * 1e3:.0f} ms; upload {st['upload']:.0f}, download {st['second_pass_wall']:.0f}",
              flush=True)
    assert np.array_equal(back[:, :n:997], batches[0][:, ::997])
    del back
    for name, w in walls.items():
        print(f"  {name}: host to host {w * 1e3:.0f} ms = {w / floor:.2f} x the floor ({floor * 1e3:.0f} ms, the fastest run)",
              flush=True)

    if a.variants:
        for label, attr, value in (("sums after the upload instead of behind it", "OVERLAP", False),
                                   ("unlogged values kept in HBM for the second pass", "KEEP_UNLOGGED", True)):
            old = getattr(lc, attr)
            setattr(lc, attr, value)
            try:
                for name in ("rescale base 2", "rescale base 10") + (("regress default",) if attr == "OVERLAP" else ()):
                    print(f"variant: {label}", flush=True)
                    out, _ = report(name, cases[name][0], a.reps, elements, cases[name][1], cases[name][2])
                    print("  bitwise equal to the default on the sampled cells:",
                          bool(np.array_equal(out.corrected[:, ::997], outs[name])), flush=True)
                    del out
            finally:
                setattr(lc, attr, old)

    if a.ref:
        from tests import linear_correct_ref as ref
        t0 = time.perf_counter()
        want = ref.rescale_batches(batches)[0]
        t = time.perf_counter() - t0
        print(f"restatement of rescaleBatches (numpy, CPU): wall {t:.1f} s = {t / walls['rescale base 2']:.1f} x the device "
              f"call; max abs diff on the sampled cells {np.abs(want[:, ::997] - outs['rescale base 2']).max():.2e}", flush=True)
        del want
        t0 = time.perf_counter()
        want = np.concatenate([x - x.mean(axis=1, keepdims=True) for x in batches], axis=1)
        t = time.perf_counter() - t0
        print(f"regressBatches' default design in numpy (x - rowMeans(x) per batch, CPU): wall {t:.1f} s = "
              f"{t / walls['regress default']:.1f} x the device call; max abs diff on the sampled cells "
              f"{np.abs(want[:, ::997] - outs['regress default']).max():.2e}", flush=True)


if __name__ == "__main__":
    main()
