#!/usr/bin/env python3
"""CPU replay of the threshold selection of a kNN candidate pass with the references as they come and in key order
(csrc/knn_order.hpp): how many values a query hands to its lists ("survivors") in either case.  No GPU.

The data are bench.py's (synth_batches(3, ...): 8 batches x 100 000 cells x 50 PCs, k = 20).  The searches of merge m:
  first   queries = batch m + 1, references = the left node (batches 1 .. m, each moved by the difference of the means onto
          batch 1: a perfect correction), the earlier batch vectors projected out of both sides;
  second  queries = cells of the left node, references = batch m + 1 (100 000);
  tricube queries = batch m + 1, references = a 65 % subset of it (c_Q is about the references' mean).
Model: the running threshold of a query is refreshed every 128 rows, sits at its 20th best value so far plus 0.1 and starts
from the 20th best of the first S rows; a value below the threshold when its block is swept is a survivor.  A perfect
threshold lets through about 23.  No lazy compaction, no groups of four: a model, not a measurement.

    python scripts/ref_order_replay.py [--queries 256] > profiles/ref_order_replay.txt
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import synth_batches  # noqa: E402

K, MARGIN, BLOCK, BUCKETS = 20, 0.1, 128, 256


def survivors(d2, S):
    """d2 [nq, nr] in sweep order -> mean survivors per query over rows [S, nr) (the sample's rows only set the start)."""
    nq, nr = d2.shape
    best = np.sort(d2[:, :S], axis=1)[:, :K]
    count = np.zeros(nq)
    for r0 in range(S, nr, BLOCK):
        blk = d2[:, r0:r0 + BLOCK]
        tau = best[:, K - 1] + MARGIN
        count += (blk < tau[:, None]).sum(axis=1)
        best = np.sort(np.concatenate([best, blk], axis=1), axis=1)[:, :K]
    return count.mean()


def bucket_order(key):
    lo, hi = key.min(), key.max()
    b = np.clip(((key - lo) * (BUCKETS / (hi - lo))).astype(np.int64), 0, BUCKETS - 1) if hi > lo else np.zeros(key.size, int)
    return np.argsort(b, kind="stable")


def case(name, R, Q, sizes, cq):
    d2 = (((Q * Q).sum(1)[:, None] - 2.0 * Q @ R.T) + (R * R).sum(1)[None, :]).astype(np.float32)
    key = ((R - cq) ** 2).sum(1)
    exact, bucketed = np.argsort(key, kind="stable"), bucket_order(key)
    cols = [f"as it is S={sizes[0]}: {survivors(d2, sizes[0]):.0f}"]
    for S in sizes:
        cols.append(f"sorted S={S}: {survivors(d2[:, exact], S):.0f} (256 buckets: {survivors(d2[:, bucketed], S):.0f})")
    print(f"{name} ({R.shape[0]} references): " + "; ".join(cols), flush=True)


def project_out(M, vecs):
    for v in vecs:
        M = M - np.outer(M @ v, v)
    return M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--merges", default="1,4,7")
    a = ap.parse_args()
    B = synth_batches(3, [100000] * 8, 50)
    rng = np.random.Generator(np.random.PCG64(1))
    for m in (int(x) for x in a.merges.split(",")):
        right = B[m]
        left = np.vstack([B[b] - (B[b].mean(0) - B[0].mean(0)) for b in range(m)])
        vecs = []
        for b in range(1, m):  # the batch vectors of the earlier merges, orthonormalised
            v = project_out((B[b].mean(0) - B[0].mean(0))[None, :], vecs)[0]
            if np.linalg.norm(v) > 1e-12:
                vecs.append(v / np.linalg.norm(v))
        L, R = project_out(left, vecs), project_out(right, vecs)
        q = rng.choice(R.shape[0], a.queries, replace=False)
        case(f"first search, merge {m}", L, R[q], [24576, 8192, 4096], R.mean(0))
        ql = rng.choice(L.shape[0], a.queries, replace=False)
        case(f"second search, merge {m}", R, L[ql], [4096, 8192], L.mean(0))
    sub = rng.choice(100000, 65000, replace=False)
    q = rng.choice(100000, a.queries, replace=False)
    case("tricube search", B[1][np.sort(sub)], B[1][q], [16250, 8192, 4096], B[1].mean(0))


if __name__ == "__main__":
    main()
