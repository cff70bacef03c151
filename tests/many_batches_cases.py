"""The inputs of the many-batch tests, shared by tests/test_cpu_many_batches.py (the oracle's pair lists do not move when
the inputs are perturbed in their last digits: a pair mismatch on the device is then a finding, not a near-tie) and
tests/test_gpu_many_batches.py (the device against the oracle).

The merge engine treats a node's original batches as SEGMENTS, walked in groups of 16 (correct.hip: rows_multi), and its
earlier non-skipped merges as batch VECTORS, applied in launches of 8 (PASS_EMAX); above 16 segments the column means no
longer come from the cached segment statistics (engine.hip: node_mean / node_means).  Every case states which of these
boundaries it crosses (`reach`), and both test files assert that from the merge_info of the result they look at."""
import functools
from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np

from tests.conftest import synth_batches

SEG_GROUP = 16   # segments per group of rows_multi
VEC_LAUNCH = 8   # batch vectors per launch (PASS_EMAX)


def draw_sizes(seed, nb):
    return [int(x) for x in np.random.default_rng(seed).integers(150, 400, nb)]


def perturb(mats, seed=77):
    """Every input multiplied by 1 + 1e-11 N(0, 1): a hundred times the device's distance from the oracle."""
    rng = np.random.default_rng(seed)
    return [m * (1.0 + 1e-11 * rng.standard_normal(m.shape)) for m in mats]


def balanced_tree(lo, hi):
    """Leaves lo..hi (1-based, inclusive) halved again and again."""
    if lo == hi:
        return lo
    mid = (lo + hi) // 2
    return [balanced_tree(lo, mid), balanced_tree(mid + 1, hi)]


def merge_shape(info):
    """Per merge: the segment count and, per side, the number of batch vectors the side carries -- the non-skipped
    earlier merges among that side's batches."""
    out = []
    for m, (left, right) in enumerate(zip(info.left, info.right)):
        vec = []
        for side in (left, right):
            s = set(side)
            vec.append(sum(1 for e in range(m) if not info.skipped[e] and set(info.left[e]) | set(info.right[e]) <= s))
        out.append({"segments": len(left) + len(right), "seg_left": len(left), "seg_right": len(right),
                    "vec_left": vec[0], "vec_right": vec[1]})
    return out


def max_segments(shape):
    return max(m["segments"] for m in shape)


def max_vectors(shape):
    return max(max(m["vec_left"], m["vec_right"]) for m in shape)


@dataclass(frozen=True)
class Case:
    id: str
    nb: int
    d: int
    reach: Callable                       # merge_shape -> bool: the boundary the case is there for
    kw: dict = field(default_factory=dict)
    restrict: bool = False                # about two thirds of every batch's cells
    labels: bool = False                  # one matrix, shuffled, with batch= labels
    skips: Optional[tuple] = None         # the merges (0-based) the oracle skips; None: none

    @property
    def seed(self):
        return 9000 + 10 * self.nb + self.d

    def sizes(self):
        return draw_sizes(self.seed, self.nb)

    def batches(self):
        return synth_batches(500 + self.nb, self.sizes(), self.d)

    def call(self, fn, batches):
        """fn = reducedMNN or the oracle's reduced_mnn, on `batches` (those of batches(), or a perturbed copy)."""
        kw = dict(self.kw)
        if self.restrict:
            rng = np.random.default_rng(self.seed + 1)
            kw["restrict"] = [np.sort(rng.choice(n, size=(2 * n) // 3, replace=False)) + 1 for n in self.sizes()]
        if self.labels:
            sizes = self.sizes()
            lab = np.repeat([f"s{b:02d}" for b in range(self.nb)], sizes)
            shuffle = np.random.default_rng(self.seed + 2).permutation(sum(sizes))
            return fn(np.vstack(batches)[shuffle], batch=lab[shuffle], **kw)
        return fn(*batches, **kw)


def _seq(segs, vecs, exact_vecs=False):
    """Sequential merges: merge m (from 1) has m + 1 segments and m - 1 vectors on its left; the last one the most."""
    def reach(shape):
        mv = max_vectors(shape)
        return max_segments(shape) >= segs and (mv == vecs if exact_vecs else mv >= vecs)
    return reach


def _two_sided(shape):
    """Some merge whose BOTH sides have more than one group of segments and more than one launch of vectors."""
    return any(min(m["seg_left"], m["seg_right"]) > SEG_GROUP and min(m["vec_left"], m["vec_right"]) > VEC_LAUNCH
               for m in shape)


def _beyond_both(shape):
    return max_segments(shape) > SEG_GROUP and max_vectors(shape) > VEC_LAUNCH


# min.batch.skip: synth_batches moves batch b away from batch 1 in proportion to b, so a chain that starts at batch 1 meets
# its near neighbours 2 and 3 between far ones at merges 6 and 11.  The oracle's batch sizes there are 0.46 and 0.61, every
# other merge's is 0.72 or more (measured on the CPU; test_cpu_many_batches.py asserts the pattern): 0.65 skips those two
# and corrects the rest, and the vector count stops tracking the merge count.
SKIP_ORDER = [1, 8, 9, 10, 11, 12, 2, 13, 14, 15, 16, 3, 17, 18, 19, 4, 5, 6, 7]
SKIP_MIN = 0.65
SKIPPED = (5, 10)


def _skip_reach(shape):
    # 19 segments; 18 merges of which 2 skipped: the last merge's left side carries 15 vectors, not 17
    return max_segments(shape) > SEG_GROUP and shape[-1]["vec_left"] == len(shape) - 1 - len(SKIPPED) > VEC_LAUNCH


CASES = [
    # sequential merges
    Case("seq10_d20", 10, 20, _seq(10, 8, exact_vecs=True)),   # 8 vectors exactly: one full launch that also carries the statistics
    Case("seq11_d20", 11, 20, _seq(11, 9)),                    # 9 vectors: second launch
    Case("seq17_d20", 17, 20, _seq(17, 15)),                   # 17 segments: second group of one; the means fall back
    Case("seq18_d7", 18, 7, _seq(18, 16)),                     # 16 vectors; odd d: rows_pass, not the 16-byte forms
    Case("seq19_d7", 19, 7, _seq(19, 17)),                     # 17 vectors
    Case("seq34_d20", 34, 20, _seq(34, 32)),                   # 33-34 segments: third group; 32 vectors
    Case("seq19_d100", 19, 100, _seq(19, 17)),                 # the 64-lane form
    Case("seq19_d140", 19, 140, _seq(19, 17)),                 # d > 128: rows_pass again, FP64 kNN scan
    # trees
    Case("tree18x18_d20", 36, 20, _two_sided, kw={"merge_order": [list(range(1, 19)), list(range(19, 37))]}),
    Case("balanced34_d100", 34, 100, _beyond_both, kw={"merge_order": balanced_tree(1, 34)}),
    # options
    Case("auto18_d20", 18, 20, _beyond_both, kw={"auto_merge": True}),
    Case("restrict18_d20", 18, 20, _beyond_both, restrict=True),
    Case("labels20_d20", 20, 20, _beyond_both, labels=True),
    Case("propk18_d20", 18, 20, _beyond_both, kw={"prop_k": 0.05}),
    Case("skip19_d20", 19, 20, _skip_reach, kw={"merge_order": SKIP_ORDER, "min_batch_skip": SKIP_MIN}, skips=SKIPPED),
]


def by_id(cid):
    return next(c for c in CASES if c.id == cid)


@functools.lru_cache(maxsize=None)
def reference(cid):
    """The oracle's result of a case: computed once per process, shared by the tests that need it, never written to."""
    from oracle import fastmnn_oracle
    case = by_id(cid)
    return case.call(fastmnn_oracle.reduced_mnn, case.batches())


# ---- the front ends -----------------------------------------------------------------------------------------------
def fastmnn_batches(nb=18, G=300, r=8, seed=1200018):
    """Genes x cells: five shared populations in an r-dimensional latent space plus batch offsets (as
    tests/test_gpu_fastmnn.py::test_fast_mnn_front_end_device_pca), nb batches of 150..399 cells."""
    rng = np.random.default_rng(seed)
    load = rng.standard_normal((G, r)) * 2.0
    cent = rng.standard_normal((r, 5)) * 2.0
    out = []
    for b, n in enumerate(draw_sizes(seed + 1, nb)):
        z = cent[:, rng.integers(0, 5, n)] + rng.standard_normal((r, n))
        out.append(np.abs(load @ z + 0.5 * rng.standard_normal((G, n)) + 6.0 + 0.15 * ((b * 7) % nb - nb / 2)))
    return out


def mnncorrect_batches(nb=18, G=10, seed=18 * 7 + 10):
    """Genes x cells, the generator of tests/test_gpu_mnn_correct.py at 18 batches of about 150 cells."""
    rng = np.random.default_rng(seed)
    ncells = [int(x) for x in rng.integers(130, 171, nb)]
    base = rng.normal(size=(G, 4))
    out = []
    for i, n in enumerate(ncells):
        lat = rng.normal(size=(4, n))
        out.append(np.abs(base @ lat + rng.normal(scale=0.3, size=(G, n)) + 1.0 * i * rng.normal(size=(G, 1))))
    return out
