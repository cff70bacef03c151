"""The cases of tests/test_gpu_correct_forms.py (the device against the long-double reference of tests/correct_ref.py and
against the oracle) and tests/test_cpu_correct_ref.py (the FP64 oracle against the same reference, at the same
tolerances: the inputs are conditioned well enough for them).  Both files import the tables from here.

Every case names the kernel it selects, by the host-side dispatch of batchelor_amd/csrc/correct.hip:
  rows_multi          even d <= 64: rows_pass_v2<.,.,32>; even d in 66..128: rows_pass_v2<.,.,64>; odd d or d in 130..256:
                      rows_pass; <APPLY, STATS> = <true,false> for a centring, <false,true> for a variance, <true,true> in the
                      engine's fused passes; workgroups of PASS_ROWS rows; d > 256 refused
  tricube_apply       k <= 32 and even d: tricube_apply_half<true>, d / 2 pieces of 16 bytes walked 32 at a time ("trips");
                      else tricube_apply_kernel<true>
  average_correction  even d <= 64 and k1 <= 32: average_correction_half; else (d <= 256) average_correction_kernel
  col_reduce          the restricted column mean of a centring: blocks of RED_ROWS positions of the restrict list"""
import functools
import math
import os
import re
from dataclasses import dataclass

import numpy as np

from tests.conftest import synth_batches

_CORRECT_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "batchelor_amd", "csrc",
                            "correct.hip")


def kernel_constant(name):
    """`constexpr int NAME = value;` of correct.hip."""
    with open(_CORRECT_HIP) as fh:
        return int(re.search(r"constexpr int %s = (\d+);" % name, fh.read()).group(1))


RED_ROWS = kernel_constant("RED_ROWS")     # 512 when the tables below were written; the CPU test holds them to it
PASS_ROWS = kernel_constant("PASS_ROWS")


def rows_form(d):
    """The kernel rows_multi launches at d dimensions (its `form`)."""
    if d > 256:
        return "refused"
    if d % 2 or d > 128:
        return "rows_pass"
    return "rows_pass_v2<32>" if d <= 64 else "rows_pass_v2<64>"


def tricube_form(k, d, U):
    """(kernel, trips of the piece loop) tricube_apply launches; k is capped at the number of MNN-involved cells."""
    k = min(k, U)
    if k <= 32 and d % 2 == 0:
        return "tricube_apply_half", -(-(d // 2) // 32)
    return "tricube_apply_kernel", 0


def average_form(d, k1):
    if d % 2 == 0 and d <= 64 and k1 <= 32:
        return "average_correction_half"
    return "average_correction_kernel" if d <= 256 else "average_correction_wide"


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- tolerances: those of tests/test_gpu_primitives.py for the same primitives ---------------------------------------
CENTRE_TOL = dict(rtol=1e-12, atol=1e-13)
TRICUBE_TOL = dict(rtol=1e-11, atol=1e-13, equal_nan=True)
AVERAGE_TOL = dict(rtol=1e-12, atol=1e-14)
VARIANCE_RTOL = 1e-12
ENGINE_ERR = 1e-10      # the per-column error tests/test_gpu_engine.py::test_config1_two_batches holds


# ---- centring ---------------------------------------------------------------------------------------------------------
# d: 1 3 63 65 127 129 255 (odd) -> rows_pass<true,false>, one .. four columns a lane (129: the third, 255: the fourth)
#    2 64                        -> rows_pass_v2<true,false,32>, first and last width
#    66 128                      -> rows_pass_v2<true,false,64>, first and last width
#    130 256                     -> rows_pass<true,false>, first and last even width above the 16-byte forms
# n: 1 and 7 (less than one trip of a wave), 511 / 512 / 513 (one workgroup short of full, full, a second of one row),
#    1100 (three workgroups)
CENTRE_D = (1, 2, 3, 63, 64, 65, 66, 127, 128, 129, 130, 255, 256)
CENTRE_N = (1, 7, 511, 512, 513, 1100)
CENTRE_OFFSETS = (0.0, 100.0)
CENTRE_CASES = [(d, n, off) for d in CENTRE_D for n in CENTRE_N for off in CENTRE_OFFSETS]
CENTRE_REFUSED_D = 257


def centre_id(case):
    return "d%d-n%d-off%g" % case


@functools.lru_cache(maxsize=None)
def _centre_draw(d, n):
    rng = np.random.default_rng([1200101, d, n])
    return _frozen(rng.standard_normal((n, d)), rng.standard_normal(d))


def centre_inputs(d, n, offset):
    """(cells [n x d] with every coordinate moved by `offset`, batch vector): the same draw at every offset."""
    test, batch = _centre_draw(d, n)
    return _frozen(test + offset)[0], batch


# restrict lists at one d of each form of rows_multi: 10 (v2<32>), 100 (v2<64>), 131 (rows_pass).  The column mean runs
# over the POSITIONS of the list in blocks of RED_ROWS: lengths either side of one block, and a list that names rows twice
# (longer than one block, shorter than the matrix, some rows named twice and some not at all)
RESTRICT_D = (10, 100, 131)
RESTRICT_N = 2 * RED_ROWS + 76
RESTRICT_KINDS = ("subset-1", "subset+0", "subset+1", "twice")
RESTRICT_CASES = [(d, kind) for d in RESTRICT_D for kind in RESTRICT_KINDS]


def restrict_list(d, kind):
    """1-based; `subset+j`: RED_ROWS + j distinct rows in shuffled order; `twice`: 700 distinct rows then 400 of them again."""
    perm = np.random.default_rng([1200102, d]).permutation(RESTRICT_N)
    if kind == "twice":
        return np.concatenate([perm[:700], perm[150:550]]) + 1
    return perm[:RED_ROWS + int(kind[len("subset"):])] + 1


# ---- total variance ---------------------------------------------------------------------------------------------------
# rows_pass*<false,true,.>: d 1 129 256 -> rows_pass, 2 64 -> rows_pass_v2<.,.,32>, 66 128 -> rows_pass_v2<.,.,64>.
# Data of sd 3 around 1e5: (mean / sd)^2 = 1e9 of cancellation for a pass that loses its pivot (first-row shift).
VARIANCE_D = (1, 2, 64, 66, 128, 129, 256)
VARIANCE_N = (2, 511, 512, 513, 1500)
VARIANCE_CASES = [(d, n) for d in VARIANCE_D for n in VARIANCE_N]
VARIANCE_MEAN, VARIANCE_SD = 1e5, 3.0


@functools.lru_cache(maxsize=None)
def variance_input(d, n):
    rng = np.random.default_rng([1200103, d, n])
    return _frozen(rng.standard_normal((n, d)) * VARIANCE_SD + VARIANCE_MEAN)[0]


# ---- tricube ----------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Tricube:
    k: int
    d: int
    U: int          # MNN-involved cells (rows of the correction)
    n: int
    ndist: float = 3
    clamp: bool = False   # groups of exact copies and 1e-9 near-copies among the MNN-involved cells

    @property
    def id(self):
        return "k%d-d%d-U%d-n%d-ndist%g%s" % (self.k, self.d, self.U, self.n, self.ndist, "-clamp" if self.clamp else "")


CLAMP_GROUPS, CLAMP_NEAR = 4, 3
TRICUBE_CASES = [
    Tricube(32, 64, 300, 1001),            # tricube_apply_half<true>, 32 pieces: one full trip; the last k of the form
    Tricube(33, 64, 300, 1001),            # tricube_apply_kernel<true>: the first k beyond the form
    Tricube(20, 9, 200, 700),              # tricube_apply_kernel<true>: odd d
    Tricube(20, 66, 200, 700),             # tricube_apply_half<true>, 33 pieces: a second trip for ONE piece
    Tricube(20, 130, 200, 403),            # tricube_apply_half<true>, 65 pieces: three trips; an odd row count (idle half)
    Tricube(5, 256, 60, 130),              # tricube_apply_half<true>, 128 pieces: four full trips
    Tricube(1, 10, 50, 97, ndist=3),       # tricube_apply_half<true>, one neighbour: weight 1
    Tricube(1, 10, 50, 97, ndist=1),       # ... at rel = 1: 0 / 0 = NaN rows (all but the MNN-involved cells themselves)
    Tricube(20, 10, 5, 64),                # U < k: safe_k = 5
    Tricube(20, 10, 1, 1),                 # one cell, its own neighbour
    Tricube(20, 10, 160, 400, clamp=True),  # tricube_apply_half<true>: bandwidth at the 1e-8 floor, weights exactly 0
    Tricube(20, 9, 160, 400, clamp=True),   # tricube_apply_kernel<true>: the same
]
TRICUBE_K0 = Tricube(0, 10, 50, 97)        # no neighbours: the input comes back bit for bit


@functools.lru_cache(maxsize=None)
def tricube_inputs(case):
    """(cells [n x d], correction [U x d], in_mnn [U] 1-based ascending)."""
    rng = np.random.default_rng([1200104, case.k, case.d, case.U, case.n])
    if not case.clamp:
        test = rng.standard_normal((case.n, case.d))
        involved = np.sort(rng.permutation(case.n)[:case.U])
    else:
        # per group: an MNN-involved cell, ceil(k / 2) exact copies of it (so the middle distance of every one of them is
        # 0 and the bandwidth the floor) and CLAMP_NEAR cells j 1e-9 away (rel about 0.1 j: weights strictly inside (0, 1));
        # whatever else fills the k neighbours is at rel > 1: weight exactly 0.  All of them MNN-involved.
        copies = math.ceil(case.k / 2)
        extra = CLAMP_GROUPS * (copies + CLAMP_NEAR)
        n0, U0 = case.n - extra, case.U - extra
        base = rng.standard_normal((n0, case.d))
        involved0 = np.sort(rng.permutation(n0)[:U0])
        rows = [base]
        for s in involved0[rng.choice(U0, CLAMP_GROUPS, replace=False)]:
            rows.append(np.tile(base[s], (copies, 1)))
            direction = rng.standard_normal(case.d)
            direction /= np.linalg.norm(direction)
            rows.append(base[s] + 1e-9 * np.arange(1, CLAMP_NEAR + 1)[:, None] * direction)
        test = np.vstack(rows)
        involved = np.concatenate([involved0, np.arange(n0, case.n)])
    correction = rng.standard_normal((case.U, case.d))
    return _frozen(test, correction, (involved + 1).astype(np.int32))


@functools.lru_cache(maxsize=None)
def tricube_neighbours(case):
    """The oracle's queryKNN(query=cells, X=cells[in_mnn], k=min(k, U)): (index 1-based into in_mnn, distance)."""
    from oracle import fastmnn_oracle
    test, _, involved = tricube_inputs(case)
    return _frozen(*fastmnn_oracle.query_knn(test[involved - 1], test, min(case.k, case.U)))


# ---- pair averaging ---------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Average:
    d: int
    k: int
    n1: int
    n2: int
    cluster: bool = False   # the left batch a tight cluster: the k right cells nearest to it pair with EVERY left cell

    @property
    def id(self):
        return "d%d-k%d-n%d-%d%s" % (self.d, self.k, self.n1, self.n2, "-cluster" if self.cluster else "")


AVERAGE_CASES = [
    Average(64, 32, 32, 200, cluster=True),   # average_correction_half with exactly 32 partners: every lane of the half
    Average(64, 33, 33, 200, cluster=True),   # average_correction_kernel with 33 partners: the first k1 beyond the form
    Average(9, 20, 600, 900),                 # average_correction_kernel: odd d
    Average(2, 5, 300, 400),                  # average_correction_half: one piece
    Average(66, 20, 500, 700),                # average_correction_kernel: the first even d beyond the form, two columns a lane
    Average(130, 20, 400, 500),               # average_correction_kernel: three columns a lane
    Average(256, 5, 200, 300),                # average_correction_kernel: its last width, four columns a lane
    Average(10, 33, 500, 800),                # average_correction_kernel: narrow rows, k1 > 32
]


@functools.lru_cache(maxsize=None)
def average_inputs(case):
    """(left [n1 x d], right [n2 x d])."""
    rng = np.random.default_rng([1200105, case.d, case.k, case.n1, case.n2])
    if case.cluster:
        right = rng.standard_normal((case.n2, case.d))
        left = 0.25 * rng.standard_normal(case.d) + 0.01 * rng.standard_normal((case.n1, case.d))
    else:
        left = rng.standard_normal((case.n1, case.d))
        right = rng.standard_normal((case.n2, case.d)) + 0.5
    return _frozen(left, right)


@functools.lru_cache(maxsize=None)
def average_pairs(case):
    """The oracle's findMutualNN(left, right, k, k): (first, second) 1-based."""
    from oracle import fastmnn_oracle
    left, right = average_inputs(case)
    return _frozen(*fastmnn_oracle.find_mutual_nn(left, right, case.k, case.k))


# ---- fused passes through the engine ----------------------------------------------------------------------------------
# three batches: two merges, the second with two segments on its left, the first merge's vector to orthogonalise against
# and the segments' old means as the pivots of the fused statistics
@dataclass(frozen=True)
class Engine:
    d: int
    offset: float = 0.0

    @property
    def id(self):
        return "d%d-off%g" % (self.d, self.offset)


ENGINE_SIZES = (600, 500, 400)
ENGINE_CASES = [
    Engine(66),               # rows_pass_v2<true,true,64>, its first width
    Engine(128),              # rows_pass_v2<true,true,64>, its last width
    Engine(130),              # rows_pass<true,true>, the first even width above the 16-byte forms
    Engine(50, offset=1e5),   # rows_pass_v2<true,true,32> with every batch translated by 1e5
]


@functools.lru_cache(maxsize=None)
def engine_batches(case):
    return _frozen(*[b + case.offset for b in synth_batches(40 + case.d, list(ENGINE_SIZES), case.d)])


@functools.lru_cache(maxsize=None)
def engine_reference(case):
    """The oracle's reduced_mnn of a case: computed once per process, shared, never written to."""
    from oracle import fastmnn_oracle
    return fastmnn_oracle.reduced_mnn(*engine_batches(case))


def nudge(mats, seed=78):
    """Every input multiplied by 1 + 1e-15 N(0, 1): a few units in the last place of every coordinate, whatever its size."""
    rng = np.random.default_rng(seed)
    return [m * (1.0 + 1e-15 * rng.standard_normal(m.shape)) for m in mats]
