"""The inputs of tests/test_gpu_knn_scale.py (the exact kNN outside unit scale, against the oracle) and of
tests/test_cpu_knn_scale_cases.py, which holds them to what the GPU tests assume of them.  No GPU import here.

What the cases pin, in batchelor_amd/csrc (the certificate `kth < tmin / s^2 + |q~|^2 - eps` of knn_refine.hip and everything
that feeds it):
  power-of-two scales   pass_scale (knn_select.hpp): s is a power of two, so the fp16 images of
                        2^e X are those of X bit for bit, and every term of the certificate scales by exactly 2^(2e)
  general position      the same with mantissas that change; an offset that the centring (candidate_pass, knn.hip) must absorb
  far queries           the NaN norm of a query whose -2 q' s leaves the fp16 range (prep_rows_f16<1>)
  one far reference     eps_den: the ordinary cells' scaled coordinates are fp16 subnormals
  degenerate norms      the scale = 1 branch of pass_scale (largest centred norm 0, below 1e-150, above 1e150)
  two clusters          the exponent window of the unscaled split-bf16 tier (pass_window, knn_select.hpp)"""
import numpy as np

from tests.conftest import synth_batches

# 4223 references: 33 ring slots of the fp16 sweep and a ragged tile; 300 queries: one full workgroup and a ragged one;
# d = 50: NS = 4, the benchmark's configuration
NR, NQ, D = 4223, 300, 50
EXPONENTS = (-80, -40, -12, 12, 40, 80)
FACTORS = (1e-6, 1e-3, 1e4, 1e6)


def scaled(arrays, e):
    """Every array times 2^e (exact: no element leaves the normal range of a double at the exponents used here)."""
    return [np.ldexp(a, e) for a in arrays]


def base():
    """Case 1 (and 3, 5, 6): references and queries of the shape above."""
    return synth_batches(51, [NR, NQ], D)


def base_wide():
    """Case 2: d = 70, k = 30 -- no fp16 list is that long beyond 61 columns, so the split-bf16 tier is the first tier."""
    return synth_batches(52, [3000, NQ], 70)


def base_large_k():
    """Case 8: k = 50 on 3000 x 200 x 50 -- four partitions of 750 rows searched at k = 36 (large_k_search)."""
    return synth_batches(58, [3000, 200], 50)


def offsets():
    """Case 3: name -> (X, Q) of the base with every coordinate + 1e4, and with column 11 + 1e6."""
    X, Q = base()
    one = np.zeros(D)
    one[11] = 1e6
    return {"all+1e4": (X + 1e4, Q + 1e4), "col11+1e6": (X + one, Q + one)}


# ---- case 5: far queries ---------------------------------------------------------------------------------------------
# first and last lane of a wave, both queries of a 16x16x32 lane (j and j + 16), the last query of a workgroup, the ragged one
FAR_POSITIONS = (0, 31, 32, 47, 255, 256, 299)
FAR_RATIOS = (30, 300, 3000, 30000)
FAR_COLUMN = 7
# -2 q' s leaves the fp16 range when |q'_c| s > 32752; s puts the largest reference norm into (24, 48]
POISONED_ABOVE = 32752 / 24
CLEAN_BELOW = 32752 / 48


def ref_centre_and_norm(X):
    """The centre candidate_pass takes (the mean of the references: all of them below 16 384 rows) and the largest centred norm."""
    c = X.mean(axis=0)
    return c, np.sqrt(((X - c) ** 2).sum(axis=1).max())


def far_queries(X, Q, ratio):
    """Q with the queries at FAR_POSITIONS moved along FAR_COLUMN to `ratio` largest reference norms from the centre."""
    c, rmax = ref_centre_and_norm(X)
    Q = Q.copy()
    Q[list(FAR_POSITIONS), FAR_COLUMN] = c[FAR_COLUMN] + ratio * rmax
    return Q


def far_ratio(X, Q):
    """Per query: its largest centred coordinate over the largest centred reference norm."""
    c, rmax = ref_centre_and_norm(X)
    return np.abs(Q - c).max(axis=1) / rmax


ONE_SIDED_K, ONE_SIDED_N, ONE_SIDED_RATIO = 20, 25, 3000


def one_sided_far_queries():
    """(X, Q, side): the case in which the NaN norm is the ONLY thing between a far query and a wrong certified row.  Without it
    the query's image holds -inf in FAR_COLUMN, so a reference's value is -inf where its centred coordinate there is positive
    and +inf (or NaN) where it is not.  Column FAR_COLUMN of the references is -delta, but +delta for ONE_SIDED_N rows (side):
    k <= 25 < KS = 32 values of -inf, a list that never fills, a threshold that stays at +inf -- and `kth < +inf` holds for
    the 20 nearest of those 25 rows.  delta is so small that the column decides nothing: the true neighbours are other rows."""
    X, Q = base()
    _, rmax = ref_centre_and_norm(X)
    delta = 1e-6 * rmax
    side = np.zeros(NR, dtype=bool)
    side[100:100 + 96 * ONE_SIDED_N:96] = True
    X = X.copy()
    X[:, FAR_COLUMN] = np.where(side, delta, -delta)
    return X, far_queries(X, Q, ONE_SIDED_RATIO), side


# ---- case 6: one far reference ---------------------------------------------------------------------------------------
FAR_REFERENCES = (17, 4222)


def far_reference(X, row, e):
    X = X.copy()
    X[row] = np.ldexp(X[row], e)
    return X


# ---- case 7: degenerate norms ----------------------------------------------------------------------------------------
DEGENERATE_FACTORS = (1.0, 1e-170, 1e170)


def one_row():
    """Small integers: 500 copies sum exactly, and the sum times fl(1 / 500) rounds back to the row, so the device's centre IS
    the row and the largest centred norm is exactly 0 (held by the CPU test, in the device's order of operations)."""
    rng = np.random.Generator(np.random.PCG64(7001))
    return rng.integers(-8, 9, D).astype(np.float64)


def equal_references(factor):
    """500 references all equal to one row and 300 random queries around it, everything times `factor`."""
    rng = np.random.Generator(np.random.PCG64(7002))
    row = one_row()
    X = np.tile(row * factor, (500, 1))
    Q = (row + rng.standard_normal((NQ, D))) * factor
    return X, Q


def equal_queries():
    X, Q = base()
    return X, np.tile(Q[5], (NQ, 1))


# ---- case 4: two clusters, beyond the f32 window of the unscaled tier --------------------------------------------------
CLUSTER_K = 30
CLUSTER_LIST = 40  # KS of the split-bf16 tier for k in 21..36: what a pass without information may keep is 40 rows


def two_clusters():
    """(X [3000 x 70], Q [256 x 70], second [256] bool): clusters at -10 and +10 along the first axis, sd 0.05; reference rows
    r % 4 == 3 and queries q % 4 == 3 are in the second."""
    rng = np.random.Generator(np.random.PCG64(4004))
    d = 70
    X = 0.05 * rng.standard_normal((3000, d))
    Q = 0.05 * rng.standard_normal((256, d))
    X[:, 0] += np.where(np.arange(3000) % 4 == 3, 10.0, -10.0)
    second = np.arange(256) % 4 == 3
    Q[:, 0] += np.where(second, 10.0, -10.0)
    return X, Q, second
