"""mnnDeltaVariance() on scipy.sparse batches, on the device, against the numpy restatement (tests/delta_variance_ref.py) on
the densified batches.

Inputs and bounds come from tests/test_cpu_delta_variance_sparse.py: the dense tests' batches with entries kept at a given
density, the dense tests' bounds (8 P u total, 4 P u mean(|x_left| + |x_right|) / 2 against the longdouble restatement),
and the check, made without a GPU, that the float64 restatement of the sparse order of operations stays inside them on
every input used here.  Shapes are relative to the sparse gene tile Ts and the pair chunk C, asked of the library.  Every
gene of every step is compared; every test prints the figures it asserts on."""
import numpy as np
import pytest
import scipy.sparse as sp

import batchelor_amd as bx
from batchelor_amd import delta_variance as dv
from batchelor_amd import multi_batch_pca as mbp
from tests.test_cpu_delta_variance import Bounds
from tests.test_cpu_delta_variance_sparse import (COS_NORM_CASES, DENSITY_CASES, PATTERN_CASES, SHAPE_CASES, case_id,
                                                  sparse_bounds, sparse_case, tile_and_chunk)

pytestmark = pytest.mark.gpu


def raw(c, mats=None):
    """The kernels' per-step values for a case: mean and total [genes x steps]; `mats`: the batches to give instead of the
    case's CSC ones (its dense copies)."""
    mats = list(c.batches if mats is None else mats)
    plan = dv.plan_genes(c.kwargs.get("subset_row"), c.kwargs.get("compute_all", False), mats[0].shape[0])
    steps = dv.check_pairs(c.pairs, sum(m.shape[1] for m in mats))
    if sp.issparse(mats[0]):
        mats = dv.csc_batches(mats, plan.rows)
    elif plan.rows is not None:
        mats = [m[plan.rows - 1] for m in mats]
    mean, total, _ = dv.device_statistics(mats, steps, c.kwargs.get("cos_norm", False), plan.norm_genes0)
    return mean, total


def call(c, **more):
    return bx.mnnDeltaVariance(*c.batches, pairs=c.pairs if len(c.pairs) > 1 else c.pairs[0], **c.kwargs, **more)


def check_steps(name, b, mean, total):
    for i in range(len(b.steps)):
        em, et = b.worst(i, mean[:, i], total[:, i])
        print(f"{name} step {i} P={b.steps[i]['P']} G={mean.shape[0]}: device error / allowance: mean {em:.3g}, total {et:.3g}")
        assert em <= 1.0 and et <= 1.0


def check_against_the_dense_handle(name, c, b, mean, total):
    """Without cos_norm: `mean` is the dense handle's bit for bit, `total` within the two allowances."""
    dmean, dtotal = raw(c, c.dense)
    same = bool(np.array_equal(mean, dmean, equal_nan=True))
    worst = 0.0
    for i, s in enumerate(b.steps):
        if s["P"] >= 2:
            err = np.abs(total[:, i].astype(np.longdouble) - dtotal[:, i])
            with np.errstate(divide="ignore", invalid="ignore"):
                worst = max(worst, float(np.where(err == 0, 0.0, err / (2 * s["tol_total"])).max()))
        else:
            assert np.all(np.isnan(total[:, i])) and np.all(np.isnan(dtotal[:, i]))
    print(f"{name}: mean bitwise equal to the dense handle's: {same}; |total - dense total| / (two allowances) {worst:.3g}")
    assert same and worst <= 1.0


@pytest.mark.parametrize("name,dens", SHAPE_CASES + DENSITY_CASES, ids=case_id)
def test_shapes_and_densities(name, dens):
    c, b = sparse_case(name, dens), sparse_bounds(name, dens)
    mean, total = raw(c)
    label = f"{name} dens {dens}"
    check_steps(label, b, mean, total)                    # (asserts the NaNs where P < 1, P < 2)
    check_against_the_dense_handle(label, c, b, mean, total)
    out = call(c)
    P = b.steps[0]["P"]
    assert out.npairs.tolist() == [P] and out.per_step is None and out.trend is None and out.adjusted is None
    assert out.gene_index.tolist() == list(range(1, mean.shape[0] + 1)) and set(out.stats["stage_ms"]) == set(dv.STAGES)
    if P >= 2:
        assert np.array_equal(out.mean, mean[:, 0]) and np.array_equal(out.total, total[:, 0])
    else:
        assert np.all(np.isnan(out.mean)) and np.all(np.isnan(out.total))


@pytest.mark.parametrize("name,dens", PATTERN_CASES, ids=case_id)
def test_patterns(name, dens):
    c, b = sparse_case(name, dens), sparse_bounds(name, dens)
    mean, total = raw(c)
    check_steps(name, b, mean, total)
    check_against_the_dense_handle(name, c, b, mean, total)
    out = call(c)
    if name == "patterns":
        print("a gene no paired cell stores: mean", mean[3, 0], "total", total[3, 0])
        assert mean[3, 0] == 0.0 and total[3, 0] == 0.0
    if name == "only-one-pair-twice":
        print("the same pair twice and nothing else: total max abs", np.abs(total).max())
        assert np.array_equal(total[:, 0], np.zeros(total.shape[0]))
    if len(c.pairs) > 1:
        assert len(out.per_step) == len(c.pairs)
        for i, t in enumerate(out.per_step):
            assert np.array_equal(t.mean, mean[:, i]) and np.array_equal(t.total, total[:, i], equal_nan=True)


@pytest.mark.parametrize("name,dens", COS_NORM_CASES, ids=case_id)
def test_cosine_norms_and_subsets(name, dens):
    c, b = sparse_case(name, dens), sparse_bounds(name, dens)
    if name.startswith("cos-zero-cell"):
        assert min(int(m.getnnz(axis=0).min()) for m in c.batches) == 0    # a cell without a stored entry: the clamp
    mean, total = raw(c)
    check_steps(name, b, mean, total)
    out = call(c)
    assert np.array_equal(out.mean, mean[:, 0]) and np.array_equal(out.total, total[:, 0])
    if name.startswith("subset"):
        sub = np.asarray(c.kwargs["subset_row"])
        G = c.dense[0].shape[0]
        assert out.gene_index.tolist() == (list(range(1, G + 1)) if c.kwargs["compute_all"] else sub.tolist())
        if not c.kwargs["compute_all"]:   # subset first, then forgotten: the same call on the rows themselves
            same = bx.mnnDeltaVariance(*[sp.csr_matrix(m[sub - 1]) for m in c.dense], pairs=c.pairs[0], cos_norm=c.kwargs["cos_norm"])
            assert np.array_equal(same.total, out.total) and np.array_equal(same.mean, out.mean)


@pytest.mark.parametrize("name", ["three-steps", "subset-all-cos", "left-run"])
def test_repeats_and_blocked_uploads_are_bitwise_equal(name, monkeypatch):
    c = sparse_case(name, 0.1)
    first = raw(c)
    same = {"a second run": raw(c)}
    for width in (1, 7, 10 ** 6):
        monkeypatch.setattr(dv, "SPARSE_BLOCK_CELLS", width)
        same[f"blocks of {width} cells"] = raw(c)
    same = {k: bool(np.array_equal(first[0], o[0]) and np.array_equal(first[1], o[1], equal_nan=True)) for k, o in same.items()}
    print(f"{name}: bitwise equal to the first run: {same}")
    assert all(same.values())


def test_three_steps_in_one_call_equal_three_calls_bit_for_bit():
    c = sparse_case("three-steps", 0.1)
    together = call(c)
    for i, step in enumerate(c.pairs):
        alone = bx.mnnDeltaVariance(*c.batches, pairs=step)
        same = bool(np.array_equal(alone.mean, together.per_step[i].mean) and
                    np.array_equal(alone.total, together.per_step[i].total))
        print(f"step {i} (P={len(step[0])}) alone against the same step of the joint call: bitwise equal {same}")
        assert same and alone.per_step is None


def test_the_chain_from_sparse_counts():
    """Sparse counts -> multiBatchNorm -> fastMNN on its sparse logcounts -> mnnDeltaVariance on them, unconverted."""
    G, sizes, d = 64, (30, 20, 15), 5              # 64 rows, 65 cells: the smallest shape the device PCA takes
    assert mbp.device_pca_takes(G, sum(sizes), d) and not mbp.device_pca_takes(G - 1, sum(sizes), d)
    assert not mbp.device_pca_takes(G, sum(sizes) - 1, d)
    rng = np.random.default_rng(17)
    base = rng.gamma(2.0, 1.0, size=(G, 3))
    counts = []
    for i, n in enumerate(sizes):
        lam = base[:, rng.integers(3, size=n)] * (0.4 + 0.2 * i) * rng.gamma(4.0, 0.25, size=(G, 1))
        counts.append(sp.csc_matrix(rng.poisson(lam).astype(np.float64)))
    logcounts = bx.multiBatchNorm(*counts).logcounts
    assert all(sp.issparse(m) for m in logcounts)
    out = bx.fastMNN(*logcounts, d=d, k=5)
    pairs = out.merge_info.pairs
    assert len(pairs) == 2 and all(len(l) >= 2 for l, _ in pairs)
    got = bx.mnnDeltaVariance(*logcounts, pairs=pairs)
    dense = [m.toarray() for m in logcounts]
    steps = [(np.asarray(l), np.asarray(r)) for l, r in pairs]
    b = Bounds(dense, steps)
    mean = np.stack([t.mean for t in got.per_step], axis=1)
    total = np.stack([t.total for t in got.per_step], axis=1)
    print(f"stored entries {[m.nnz for m in logcounts]} of {[G * n for n in sizes]}; pairs per step {got.npairs.tolist()}")
    check_steps("the chain", b, mean, total)
    assert got.npairs.tolist() == [len(l) for l, _ in pairs]


def test_tile_and_chunk_are_what_the_cases_assume():
    Ts, C = tile_and_chunk()
    assert (Ts, C) == (dv.sparse_gene_tile(), dv.pair_chunk())
    print("sparse gene tile", Ts, "pair chunk", C)
