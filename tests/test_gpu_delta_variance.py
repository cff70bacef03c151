"""mnnDeltaVariance() on the device against the numpy restatement (tests/delta_variance_ref.py).

Inputs and bounds come from tests/test_cpu_delta_variance.py, which derives the bounds (8 P u total for the variance,
4 P u mean(|x_left| + |x_right|) / 2 for the mean, against the longdouble restatement) and checks without a GPU that the
float64 restatement itself stays inside them on every input used here.  The shapes are taken relative to the gene-tile
width T and the pair-chunk length C that the kernels use, asked of the library.  Every gene of every step is compared;
every test prints the figures it asserts on."""
import numpy as np
import pytest

import batchelor_amd as bx
from batchelor_amd import delta_variance as dv
from tests import delta_variance_ref as ref
from tests.test_cpu_delta_variance import Bounds, G_LABELS, OTHER_CASES, P_LABELS, bounds, case, tile_and_chunk
from tests.test_gpu_mnn_correct import _batches

pytestmark = pytest.mark.gpu


def raw(c):
    """The kernels' per-step values for a case: mean and total [genes x steps]."""
    mats = [np.asarray(b) for b in c.batches]
    plan = dv.plan_genes(c.kwargs.get("subset_row"), c.kwargs.get("compute_all", False), mats[0].shape[0])
    steps = dv.check_pairs(c.pairs, sum(m.shape[1] for m in mats))
    if plan.rows is not None:
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


@pytest.mark.parametrize("p", P_LABELS)
@pytest.mark.parametrize("g", G_LABELS)
def test_shapes(g, p):
    name = f"shape:{g}:{p}"
    c, b = case(name), bounds(name)
    mean, total = raw(c)
    check_steps(name, b, mean, total)
    out = call(c)
    P = b.steps[0]["P"]
    assert out.npairs.tolist() == [P] and out.per_step is None and out.trend is None and out.adjusted is None
    assert out.gene_index.tolist() == list(range(1, mean.shape[0] + 1)) and set(out.stats["stage_ms"]) == set(dv.STAGES)
    if P >= 2:   # one valid step: the combination is that step
        assert np.array_equal(out.mean, mean[:, 0]) and np.array_equal(out.total, total[:, 0])
    else:        # no valid step (:172): NaN
        assert np.all(np.isnan(out.mean)) and np.all(np.isnan(out.total))


# the cosine norms over a list of 63, 64 and 65 genes: a wave takes 64 of them at a time.  (A list of one gene makes that
# gene's scaled values all equal, so its total has no allowance to be held to; tests/test_gpu_cluster_mnn.py has that list.)
NORM_LIST_CASES = [f"subset-all-cos:{n}" for n in (63, 64, 65)]


@pytest.mark.parametrize("name", OTHER_CASES + NORM_LIST_CASES)
def test_cases(name):
    c, b = case(name), bounds(name)
    mean, total = raw(c)
    check_steps(name, b, mean, total)
    out = call(c)
    if name == "only-one-pair-twice":
        print("the same pair twice and nothing else: total max abs", np.abs(total).max())
        assert np.array_equal(total[:, 0], np.zeros(total.shape[0]))
    if name.startswith("subset"):
        sub = np.asarray(c.kwargs["subset_row"])
        G = c.batches[0].shape[0]
        assert out.gene_index.tolist() == (list(range(1, G + 1)) if c.kwargs["compute_all"] else sub.tolist())
        if not c.kwargs["compute_all"]:   # subset first, then forgotten (:113-119): the same call on the rows themselves
            same = bx.mnnDeltaVariance(*[m[sub - 1] for m in c.batches], pairs=c.pairs[0], cos_norm=c.kwargs["cos_norm"])
            assert np.array_equal(same.total, out.total) and np.array_equal(same.mean, out.mean)
    if len(c.pairs) > 1:
        assert len(out.per_step) == len(c.pairs)
        for i, t in enumerate(out.per_step):
            assert np.array_equal(t.mean, mean[:, i]) and np.array_equal(t.total, total[:, i], equal_nan=True)
        # the combination: within the weighted mean of the steps' allowances plus the rounding of the weighted mean itself
        w = np.asarray([s["P"] if s["P"] >= 2 else 0 for s in b.steps], dtype=np.longdouble)
        for f, tol in (("mean", "tol_mean"), ("total", "tol_total")):
            steps = [s for s in b.steps if s["P"] >= 2]
            allowed = sum(s["P"] * s[tol] for s in steps) / w.sum() + 4 * 2.0 ** -53 * np.abs(b.exact[f])
            err = np.abs(getattr(out, f).astype(np.longdouble) - b.exact[f])
            print(f"{name} combined {f}: error / allowance {float((err / allowed).max()):.3g}")
            assert np.all(err <= allowed)


def test_trend_fit_on_the_device_values():
    c = case("subset-all-cos")
    seen = []

    def trend_fit(m, t):
        seen.append(m.size)
        coef = np.polyfit(m, t, 1)
        return lambda at: np.polyval(coef, at)

    out = call(c, trend_fit=trend_fit)
    want = ref.mnn_delta_variance(c.batches, c.pairs, trend_fit=trend_fit, **c.kwargs)
    G = c.batches[0].shape[0]
    assert seen == [len(c.kwargs["subset_row"])] * 2 and out.trend.shape == (G,)
    assert np.array_equal(out.adjusted, out.total - out.trend)
    # a straight line through values that agree to the bounds: its coefficients move by about as much
    err = float(np.abs(out.trend - want["trend"]).max() / np.abs(want["trend"]).max())
    print("trend fitted on the subset, every gene: max rel difference to the restatement", err)
    assert err < 1e-9


def test_three_steps_in_one_call_equal_three_calls_bit_for_bit():
    c = case("three-steps")
    together = call(c)
    for i, step in enumerate(c.pairs):
        alone = bx.mnnDeltaVariance(*c.batches, pairs=step)
        same = bool(np.array_equal(alone.mean, together.per_step[i].mean) and
                    np.array_equal(alone.total, together.per_step[i].total))
        print(f"step {i} (P={len(step[0])}) alone against the same step of the joint call: bitwise equal {same}")
        assert same and alone.per_step is None


@pytest.mark.parametrize("name", ["three-steps", "subset-all-cos", "left-run"])
def test_repeats_and_blocked_uploads_are_bitwise_equal(name, monkeypatch):
    c = case(name)
    first = raw(c)
    again = raw(c)
    monkeypatch.setattr(dv, "BLOCK_BYTES", 8 * c.batches[0].shape[0] * 37)   # column blocks of 37 cells
    blocked = raw(c)
    same = [bool(np.array_equal(first[0], o[0]) and np.array_equal(first[1], o[1], equal_nan=True)) for o in (again, blocked)]
    print(f"{name}: bitwise equal to the first run: a second run, an upload in blocks of 37 cells: {same}")
    assert all(same)


@pytest.mark.parametrize("front", ["fastMNN", "mnnCorrect"])
def test_pairs_straight_from_a_correction(front):
    B = _batches(77, [300, 310, 290], 200)
    if front == "fastMNN":
        pairs = bx.fastMNN(*B, d=20).merge_info.pairs
    else:
        pairs = bx.mnnCorrect(*B).merge_info.pairs
    assert len(pairs) == 2 and all(len(l) >= 2 for l, _ in pairs)
    for cos_norm in (False, True):
        out = bx.mnnDeltaVariance(*B, pairs=pairs, cos_norm=cos_norm)
        b = Bounds(B, [(np.asarray(l), np.asarray(r)) for l, r in pairs], cos_norm=cos_norm)
        mean = np.stack([t.mean for t in out.per_step], axis=1)
        total = np.stack([t.total for t in out.per_step], axis=1)
        check_steps(f"{front} pairs, cos_norm={cos_norm}", b, mean, total)
        assert out.npairs.tolist() == [len(l) for l, _ in pairs] and max(out.npairs) <= 10_000
        f64 = ref.mnn_delta_variance(B, [(np.asarray(l), np.asarray(r)) for l, r in pairs], cos_norm=cos_norm)
        for i, t in enumerate(f64["per_step"]):   # these inputs exist only here: the restatement is held to the bounds here
            em, et = b.worst(i, t["mean"], t["total"])
            print(f"    float64 restatement, step {i}: error / allowance: mean {em:.3g}, total {et:.3g}")
            assert em <= 1.0 and et <= 1.0


def test_tile_and_chunk_are_what_the_cases_assume():
    T, C = tile_and_chunk()
    assert (T, C) == (dv.gene_tile(), dv.pair_chunk())
    print("gene tile", T, "pair chunk", C)
