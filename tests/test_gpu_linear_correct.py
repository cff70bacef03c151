"""rescaleBatches() / regressBatches() on the device against the numpy restatement (tests/linear_correct_ref.py).

Inputs are log-transformed counts, as in the reference's tests: log.base^x - pseudo.count returns to a count, so the
subtraction does not cancel and the relative tolerance of the project's averaging kernels applies
(rtol=1e-12, atol=1e-13, tests/test_gpu_primitives.py:62-75).  For a general design the error carries the design's
conditioning: the bound is ten times the spread between two solvers of the restatement (lstsq against an explicit QR
solve, same inputs) or 1e-12, whichever is larger.  Every test prints the figure it asserts on; every cell and gene of a
result is compared (the probe-size case compares every cell of its sampled genes)."""
import numpy as np
import pytest

import batchelor_amd as bx
from batchelor_amd import linear_correct as lc
from tests import linear_correct_ref as ref

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-12, 1e-13


def make(G, sizes, seed, log_base=2.0, pseudo=1.0):
    """Log-counts of `sizes` cells each; gene 0 is all zero in batch 0 only, gene 1 in every batch."""
    rng = np.random.default_rng(seed)
    means = 2.0 ** rng.gamma(2.0, 1.0, G)
    out = []
    for b, n in enumerate(sizes):
        a = rng.poisson((means * rng.uniform(0.3, 2.0, G))[:, None], (G, n)).astype(np.float64)
        if b == 0:
            a[0] = 0
        a[1] = 0
        out.append(np.log(a + pseudo) / np.log(log_base))
    return out


def restrictions(sizes, seed):
    rng = np.random.default_rng(seed)
    return [np.sort(rng.choice(n, max(1, (2 * n) // 3), replace=False)) + 1 for n in sizes]


def excess(got, want, rtol=RTOL, atol=ATOL):
    """max of |got - want| / (atol + rtol |want|): at most 1 where numpy.allclose holds."""
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    return float(np.nanmax(np.abs(got - want) / (atol + rtol * np.abs(want))))


SIZES = {10: (700, 1500, 90), 500: (300, 1300), 2000: (900, 257, 1100, 40)}   # chunks of 256 cells: several in a batch


@pytest.mark.parametrize("G", [10, 500, 2000])
@pytest.mark.parametrize("restricted", [False, True])
@pytest.mark.parametrize("log_base,pseudo", [(2.0, 1.0), (10.0, 3.2), (np.e, 1.0)])
def test_rescale(G, restricted, log_base, pseudo):
    B = make(G, SIZES[G], 100 + G, log_base, pseudo)
    r = restrictions(SIZES[G], G) if restricted else None
    got = bx.rescaleBatches(*B, restrict=r, log_base=log_base, pseudo_count=pseudo)
    want, avg, reference = ref.rescale_batches(B, log_base, pseudo, None, r)
    e = excess(got.corrected, want)
    ea = max(excess(got.averages, avg), excess(got.reference, reference))
    print(f"rescale G={G} restrict={restricted} base={log_base:.3g} pseudo={pseudo}: error / allowance: corrected {e:.3g}, "
          f"averages {ea:.3g}")
    assert e <= 1.0 and ea <= 1.0
    assert got.batch.tolist() == np.repeat(np.arange(1, len(B) + 1), SIZES[G]).tolist()
    assert set(got.stats["stage_ms"]) == set(lc.STAGES)


EDGE_SIZES = (1, 3, 4, 5, 255, 256, 257, 513)      # chunks of 1, 3, 4, 5, 255, 256 and 257 cells, and two chunks plus one
EDGE_RESTRICTED = (1, 2, 3, 5, 6, 7, 255, 257)     # restricted lists of 4k + 1, 4k + 2 and 4k + 3 cells


@pytest.mark.parametrize("G", [1, 2, 255, 256, 257, 258])   # a single lane of a second tile of 256 genes at 257
@pytest.mark.parametrize("restricted", [False, True])
def test_edges_of_the_chunk_walk(G, restricted):
    rng = np.random.default_rng(130 + G)
    B = [np.log2(rng.poisson(rng.uniform(2.0, 30.0, (G, 1)), (G, n)) + 1.0) for n in EDGE_SIZES]
    r = [np.sort(rng.choice(n, m, replace=False)) + 1 for n, m in zip(EDGE_SIZES, EDGE_RESTRICTED)] if restricted else None
    got = bx.rescaleBatches(*B, restrict=r)
    want, avg, reference = ref.rescale_batches(B, 2.0, 1.0, None, r)
    e = max(excess(got.corrected, want), excess(got.averages, avg), excess(got.reference, reference))
    reg = bx.regressBatches(*B, restrict=r)
    want, labels, coef = ref.regress(B, restrict=r)
    e2 = max(excess(reg.corrected, want), excess(reg.coefficients, coef))
    print(f"chunk edges G={G} restrict={restricted}: error / allowance: rescale {e:.3g}, regress {e2:.3g}")
    assert e <= 1.0 and e2 <= 1.0


def test_rescale_rows_of_zeros_stay_zero():
    B = make(500, SIZES[500], 150)
    got = bx.rescaleBatches(*B).corrected
    print("genes without counts in one batch / in all: max abs", np.abs(got[:2]).max())
    assert np.array_equal(got[:2], np.zeros((2, sum(SIZES[500]))))


@pytest.mark.parametrize("G", [10, 500, 2000])
@pytest.mark.parametrize("restricted", [False, True])
def test_regress_default(G, restricted):
    B = make(G, SIZES[G], 200 + G)
    r = restrictions(SIZES[G], G) if restricted else None
    got = bx.regressBatches(*B, restrict=r)
    want, labels, coef = ref.regress(B, restrict=r)
    e = max(excess(got.corrected, want), excess(got.coefficients, coef))
    print(f"regress default G={G} restrict={restricted}: error / allowance {e:.3g}")
    assert e <= 1.0
    assert np.array_equal(got.batch, labels)


@pytest.mark.parametrize("fn", ["rescale", "regress"])
@pytest.mark.parametrize("restricted", [False, True])
def test_single_object_with_batch(fn, restricted):
    G, sizes = 500, (300, 1300, 600)
    B = make(G, sizes, 300)
    rng = np.random.default_rng(301)
    shuffle = rng.permutation(sum(sizes))
    x = np.concatenate(B, axis=1)[:, shuffle]
    batch = np.repeat(["b", "a", "c"], sizes)[shuffle]
    r = [rng.random(x.shape[1]) < 0.7] if restricted else None
    f = bx.rescaleBatches if fn == "rescale" else bx.regressBatches
    got = f(x, batch=batch, restrict=r)
    want = getattr(ref, fn)([x], batch=batch, restrict=r)
    e = excess(got.corrected, want[0])
    print(f"{fn} batch= on a shuffled matrix, restrict={restricted}: error / allowance {e:.3g}")
    assert e <= 1.0
    assert np.array_equal(got.batch, want[1])


@pytest.mark.parametrize("fn", ["rescale", "regress"])
def test_subset_row_and_correct_all(fn):
    B = make(500, SIZES[500], 400)
    sub = np.random.default_rng(401).permutation(500)[:123] + 1
    f = bx.rescaleBatches if fn == "rescale" else bx.regressBatches
    a = f(*B, subset_row=sub).corrected
    b = f(*[m[sub - 1] for m in B]).corrected
    c = f(*B, subset_row=sub, correct_all=True).corrected
    d = f(*B).corrected
    print(f"{fn} subset_row: {a.shape}, correct_all: {c.shape}")
    assert np.array_equal(a, b) and np.array_equal(c, d) and c.shape[0] == 500


def designs(sizes, seed):
    n = sum(sizes)
    b = np.repeat(np.arange(len(sizes)), sizes)
    factor = np.concatenate([np.ones((n, 1)), (b[:, None] == np.arange(1, len(sizes))[None]).astype(float)], axis=1)
    cov = np.random.default_rng(seed).normal(size=n)
    return {"factor": factor, "factor+covariate": np.concatenate([factor, ((cov - cov.mean()) / cov.std())[:, None]], axis=1)}


def general_bound(B, design, keep, r):
    a = ref.regress(B, design=design, keep=keep, restrict=r, solver="lstsq")[0]
    b = ref.regress(B, design=design, keep=keep, restrict=r, solver="qr")[0]
    spread = float(np.abs(a - b).max())
    return a, spread, max(10.0 * spread, 1e-12)


@pytest.mark.parametrize("G", [10, 500, 2000])
@pytest.mark.parametrize("which", ["factor", "factor+covariate"])
@pytest.mark.parametrize("restricted,keep", [(False, None), (True, None), (False, [1])])
def test_regress_design(G, which, restricted, keep):
    B = make(G, SIZES[G], 500 + G)
    design = designs(SIZES[G], G)[which]
    r = restrictions(SIZES[G], G) if restricted else None
    want, spread, bound = general_bound(B, design, keep, r)
    got = bx.regressBatches(*B, design=design, keep=keep, restrict=r)
    err = float(np.abs(got.corrected - want).max())
    print(f"regress design={which} G={G} restrict={restricted} keep={keep}: lstsq-vs-QR spread {spread:.3g}, "
          f"bound {bound:.3g}, device max abs error {err:.3g}")
    assert got.corrected.shape == want.shape and err <= bound
    if which == "factor" and keep is None:   # ~factor(b) spans the default design (test-regress-batch.R:56-57)
        e = float(np.abs(got.corrected - bx.regressBatches(*B, restrict=r).corrected).max())
        print(f"    against the default design: max abs {e:.3g}")
        assert e <= bound


def test_regress_single_object_with_design_is_one_batch():
    B = make(500, SIZES[500], 600)
    design = designs(SIZES[500], 6)["factor+covariate"]
    want, spread, bound = general_bound(B, design, None, None)
    got = bx.regressBatches(np.concatenate(B, axis=1), design=design)
    err = float(np.abs(got.corrected - want).max())
    print(f"single object + design: spread {spread:.3g}, bound {bound:.3g}, device max abs error {err:.3g}")
    assert err <= bound and np.all(got.batch == 1)


def test_regress_keep_with_default_design():
    B = make(500, SIZES[500], 700)
    got = bx.regressBatches(*B, keep=[2])
    want, spread, bound = general_bound(B, np.repeat(np.eye(2), SIZES[500], axis=0), [2], None)
    err = float(np.abs(got.corrected - want).max())
    print(f"default design, keep=[2]: spread {spread:.3g}, bound {bound:.3g}, device max abs error {err:.3g}")
    assert err <= bound and np.array_equal(got.corrected[:, SIZES[500][0]:], B[1])


def test_regress_pcs():
    B = make(500, SIZES[500], 800)
    got = bx.regressBatches(*B, d=5)
    parts = [got.corrected[:, :SIZES[500][0]], got.corrected[:, SIZES[500][0]:]]
    want = np.concatenate(bx.multiBatchPCA(*parts, d=5)["pcs"], axis=0)
    diff = float(np.abs(np.abs(got.pcs) - np.abs(want)).max() / np.abs(want).max())
    print("pcs", got.pcs.shape, "against multiBatchPCA of the residuals, up to sign: max rel", diff)
    assert got.pcs.shape == (sum(SIZES[500]), 5) and diff < 1e-6


@pytest.mark.parametrize("case", ["rescale2", "rescale10", "regress", "design"])
@pytest.mark.parametrize("restricted", [False, True])
def test_blocked_upload_and_repeats_are_bitwise_equal(case, restricted, monkeypatch):
    G, sizes = 2000, (900, 257, 1100, 40)
    B = make(G, sizes, 900, 10.0, 3.2) if case == "rescale10" else make(G, sizes, 900)
    r = restrictions(sizes, 9) if restricted else None
    design = designs(sizes, 9)["factor+covariate"]

    def run():
        if case == "rescale2":
            return bx.rescaleBatches(*B, restrict=r).corrected
        if case == "rescale10":
            return bx.rescaleBatches(*B, restrict=r, log_base=10, pseudo_count=3.2).corrected
        if case == "regress":
            return bx.regressBatches(*B, restrict=r).corrected
        return bx.regressBatches(*B, restrict=r, design=design).corrected

    whole = run()
    again = run()
    monkeypatch.setattr(lc, "BLOCK_BYTES", 8 * G * 100)   # blocks of 100 cells: they end inside the chunks of 256
    blocked = run()
    monkeypatch.setattr(lc, "BLOCK_BYTES", 8 * G * 37)
    blocked37 = run()
    monkeypatch.setattr(lc, "OVERLAP", False)             # the sums taken after the upload instead of behind it
    late = run()
    assert np.all(np.isfinite(whole))
    same = [bool(np.array_equal(whole, o)) for o in (again, blocked, blocked37, late)]
    print(f"{case} restrict={restricted}: bitwise equal to the whole upload: repeat, blocks of 100, of 37, sums after "
          f"the upload: {same}")
    assert all(same)


def test_kept_unlogged_values_give_the_same_bits(monkeypatch):
    B = make(500, SIZES[500], 1000, 10.0)
    a = bx.rescaleBatches(*B, log_base=10).corrected
    assert np.all(np.isfinite(a))
    monkeypatch.setattr(lc, "KEEP_UNLOGGED", not lc.KEEP_UNLOGGED)
    b = bx.rescaleBatches(*B, log_base=10).corrected
    print("recomputed against kept unlogged values: bitwise equal", bool(np.array_equal(a, b)))
    assert np.array_equal(a, b)


def test_probe_size_on_sampled_genes():
    """4 x 200 000 cells x 2 000 genes (12.8 GB), the size of scripts/linear_correct_probe.py: the restatement on 16
    sampled genes, every cell of them."""
    G, n, nb = 2000, 200_000, 4
    rng = np.random.default_rng(1100)
    B = []
    for b in range(nb):
        x = np.empty((G, n), order="F")
        for a in range(0, n, 20_000):
            x[:, a:a + 20_000] = np.log2(rng.integers(0, 40 + 10 * b, (20_000, G)).T + 1.0)
        B.append(x)
    genes = np.sort(rng.choice(G, 16, replace=False))
    small = [m[genes] for m in B]
    got = bx.rescaleBatches(*B)
    e1 = excess(got.corrected[genes], ref.rescale_batches(small)[0])
    del got
    got = bx.regressBatches(*B)
    e2 = excess(got.corrected[genes], ref.regress(small)[0])
    print(f"probe size, 16 sampled genes x {nb * n} cells: rescale error / allowance {e1:.3g}, regress {e2:.3g}")
    assert e1 <= 1.0 and e2 <= 1.0
