"""adjust_shift_variance in strict mode (var_adj_strict): the tiled form settles a cell one of three ways -- 0 the histogram
quantile (well conditioned, equal to the reference to 1e-8), 1 the literal re-run (flagged, bit-equal), 2 flagged but with
more kept addends than the re-run holds (the histogram quantile again, which may land on ANOTHER quantile).  Strict mode
records the ways per call, compacts the mode-2 cells into an ascending list and sends exactly those through the literal
wide form, whose values are the exact form's bits.  The hooks "asv_fast" (tiled form at any size) and "asv_cap" (addends a
chain of the re-run keeps; 0 = no re-run, so every flagged cell is mode 2) bring all of it down to a thousand cells."""
import numpy as np
import pytest

from tests.conftest import synth_batches
from tests.test_gpu_primitives import _asv_edges_data, _asv_shapes

pytestmark = pytest.mark.gpu

SIGMA = 0.3
CAPS = (0, 64, -1)


@pytest.fixture
def nat():
    from batchelor_amd import natives
    return natives


@pytest.fixture(scope="module")
def hole(oracle):
    """The "100d" shape at sigma 0.3: the oracle once, and the strict runs at the three caps with the ways each took
    (asv_modes) and the call's own counts.  Read-only for the tests that share it."""
    from batchelor_amd import _lib, natives
    a, b, v = _asv_shapes()["100d"]
    r1, r2 = np.arange(a.shape[1]), np.arange(b.shape[1])
    ref = oracle.adjust_shift_variance(a, b, v, SIGMA, r1, r2)
    runs = {}
    try:
        _lib.dev_set("asv_fast", 1)
        _lib.dev_set("asv_modes", b.shape[1])
        for cap in CAPS:
            _lib.dev_set("asv_cap", cap)
            out, counts = natives.adjust_shift_variance(a, b, v, SIGMA, r1, r2, strict=True, counts=True)
            modes = _lib.dev_get_bytes("asv_modes", b.shape[1])
            runs[cap] = (out, counts, modes)
        _lib.dev_set("asv_cap", 0)
        plain = natives.adjust_shift_variance(a, b, v, SIGMA, r1, r2)
    finally:
        _lib.dev_set("reset", 0)
    for x in (ref, plain, *[y for run in runs.values() for y in run]):
        x.setflags(write=False)
    return {"data": (a, b, v, r1, r2), "ref": ref, "runs": runs, "plain": plain}


@pytest.mark.parametrize("cap", CAPS)
def test_strict_closes_the_hole(hole, cap):
    out, counts, modes = hole["runs"][cap]
    ref = hole["ref"]
    n2 = ref.size
    assert set(np.unique(modes).tolist()) <= {0, 1, 2}
    flagged = modes > 0
    assert np.array_equal(out[flagged], ref[flagged]), (cap, int((out[flagged] != ref[flagged]).sum()))
    close = np.isclose(out, ref, rtol=1e-8, atol=1e-12, equal_nan=True)
    share = close[~flagged].mean() if (~flagged).any() else 1.0
    print(f"cap {cap}: counts {counts.tolist()}, modes 0/1/2 = {[int((modes == m).sum()) for m in (0, 1, 2)]}, "
          f"{share:.6f} of the unflagged cells equal to the oracle")
    assert share >= 0.999, (cap, share)
    assert counts[0] == n2
    assert counts[1] == int((modes == 1).sum())
    assert counts[2] == int((modes == 2).sum()) == counts[3]
    if cap == 0:
        assert counts[1] == 0 and counts[3] > 0


def test_without_strict_the_hole_is_open(hole):
    """The same call at cap 0 without strict: cells the strict run marks as mode 2 are NOT the oracle's (DESIGN.md quotes 0.41
    of all cells equal here).  This is what strict mode is for."""
    _, _, modes = hole["runs"][0]
    close = np.isclose(hole["plain"], hole["ref"], rtol=1e-8, atol=1e-12, equal_nan=True)
    print(f"no strict, cap 0: {close.mean():.4f} of all cells and {close[modes == 2].mean():.4f} of the "
          f"{int((modes == 2).sum())} mode-2 cells equal to the oracle")
    assert (modes == 2).any() and not close[modes == 2].all()


def test_strict_gives_one_answer_whatever_the_cap(hole):
    o0, o64, odef = (hole["runs"][cap][0] for cap in CAPS)
    assert np.array_equal(o0, o64, equal_nan=True) and np.array_equal(o0, odef, equal_nan=True)


def test_strict_chunk_edges(hole, nat, dev):
    """The strict pass walks the list chunk by chunk ("asv_chunk" cells at a time): one cell, a chunk that leaves a short
    last one, exactly the list, and more than the list."""
    a, b, v, r1, r2 = hole["data"]
    out0, counts0, _ = hole["runs"][0]
    C = int(counts0[3])
    dev("asv_fast", 1)
    dev("asv_cap", 0)
    for chunk in (1, 7, C, C + 1):
        dev("asv_chunk", chunk)
        out, counts = nat.adjust_shift_variance(a, b, v, SIGMA, r1, r2, strict=True, counts=True)
        assert np.array_equal(out, out0, equal_nan=True), chunk
        assert counts.tolist() == counts0.tolist(), chunk


@pytest.mark.parametrize("g", [62, 126, 200])
def test_strict_every_stream_form_and_restrict_edges(oracle, nat, dev, g):
    """The three stream forms of the tile kernel, restrict vectors that leave cells out and repeat cells, a zero gradient."""
    from batchelor_amd import _lib
    d1, d2, cv, r1, r2 = _asv_edges_data(g)
    ref = oracle.adjust_shift_variance(d1, d2, cv, 0.05, r1, r2)
    dev("asv_fast", 1)
    dev("asv_cap", 0)
    dev("asv_modes", d2.shape[1])
    out, counts = nat.adjust_shift_variance(d1, d2, cv, 0.05, r1, r2, strict=True, counts=True)
    modes = _lib.dev_get_bytes("asv_modes", d2.shape[1])
    flagged = modes > 0
    print(f"g {g}: counts {counts.tolist()}")
    assert counts[3] == int((modes == 2).sum()) and counts[3] > 0
    assert np.array_equal(out[flagged], ref[flagged], equal_nan=True), int((out[flagged] != ref[flagged]).sum())
    assert np.isnan(out[17]) and np.isnan(ref[17])
    again = nat.adjust_shift_variance(d1, d2, cv, 0.05, r1, r2, strict=True)
    assert np.array_equal(out, again, equal_nan=True)
    # a SPARSE record: some cells are not flagged here.  The strict pass leaves them exactly what the same call without
    # strict gives (the list holds the mode-2 cells and no other), and the whole result meets the bar of
    # test_adjust_shift_variance_tiled_form_every_stream_form on this data.
    plain = nat.adjust_shift_variance(d1, d2, cv, 0.05, r1, r2)
    assert 0 < int((~flagged).sum()) < modes.size
    assert np.array_equal(out[~flagged], plain[~flagged], equal_nan=True)
    assert not np.array_equal(out[flagged], plain[flagged], equal_nan=True)   # (and the flagged ones did move)
    close = np.isclose(out, ref, rtol=1e-8, atol=1e-12, equal_nan=True)
    print(f"g {g}: {int((~flagged).sum())} unflagged cells, {close[~flagged].mean():.6f} of them and {close.mean():.6f} of all "
          f"cells equal to the oracle")
    assert close.mean() >= 0.999, (g, close.mean())


@pytest.mark.parametrize("sigma", [1.0, 0.05])
def test_strict_smallest_inputs(oracle, nat, dev, sigma):
    """The shapes of test_adjust_shift_variance_tiled_form_tiny_and_empty (without its one-dimension entry, whose exact integer
    ties lie outside the flag) with its criterion: an empty restrict2, one reference cell, fewer cells than a tile, one cell
    against one -- and wherever no cell is flagged an empty list, for which nothing is launched."""
    dev("asv_fast", 1)
    rng = np.random.default_rng(100035)
    for g, n1, n2, nr1, nr2 in [(7, 50, 20, 50, 0), (7, 50, 20, 1, 20), (7, 50, 20, 3, 5), (100, 3, 2, 3, 2), (25, 1, 1, 1, 1),
                                (50, 300, 17, 300, 17)]:
        d1 = rng.standard_normal((g, n1)) * 0.5
        d2 = rng.standard_normal((g, n2)) * 0.5 + 0.2
        cv = rng.standard_normal((n2, g))
        r1 = rng.permutation(n1)[:nr1]
        r2 = rng.permutation(n2)[:nr2]
        ref = oracle.adjust_shift_variance(d1, d2, cv, sigma, r1, r2)
        for cap in (0, -1):
            dev("asv_cap", cap)
            out, counts = nat.adjust_shift_variance(d1, d2, cv, sigma, r1, r2, strict=True, counts=True)
            close = np.isclose(out, ref, rtol=1e-8, atol=1e-12, equal_nan=True)
            assert close.all(), (g, n1, n2, nr1, nr2, cap, out, ref)
            assert counts[0] == n2 and 0 <= counts[3] <= n2 and counts[2] == counts[3]


def test_strict_is_a_no_op_on_the_exact_plan(nat):
    a, b, v = _asv_shapes()["25d"]
    r1, r2 = np.arange(a.shape[1]), np.arange(b.shape[1])
    assert nat.adjust_shift_variance_form(b.shape[1], r1.size, r2.size) == "exact"
    off = nat.adjust_shift_variance(a, b, v, SIGMA, r1, r2)
    on, counts = nat.adjust_shift_variance(a, b, v, SIGMA, r1, r2, strict=True, counts=True)
    assert np.array_equal(on, off, equal_nan=True)
    assert counts.tolist() == [-1, -1, -1, -1]


def test_strict_off_reports_no_counts(nat, dev):
    dev("asv_fast", 1)
    a, b, v = _asv_shapes()["25d"]
    r1, r2 = np.arange(a.shape[1]), np.arange(b.shape[1])
    _, counts = nat.adjust_shift_variance(a, b, v, SIGMA, r1, r2, counts=True)
    assert counts.tolist() == [-1, -1, -1, -1]


def test_knob_makes_every_call_strict(nat, dev):
    """The testing knob "asv_strict" = 1 (what times strict mode on a workload whose driver has no switch for it): a call
    that does not ask for strict runs strict all the same, with the scratch to match, through each of the three callers."""
    import batchelor_amd as bx
    a, b, v = _asv_shapes()["100d"]
    r1, r2 = np.arange(a.shape[1]), np.arange(b.shape[1])
    dev("asv_fast", 1)
    dev("asv_cap", 0)
    asked, counts_asked = nat.adjust_shift_variance(a, b, v, SIGMA, r1, r2, strict=True, counts=True)
    plain = nat.adjust_shift_variance(a, b, v, SIGMA, r1, r2)
    dev("asv_strict", 1)
    knob, counts = nat.adjust_shift_variance(a, b, v, SIGMA, r1, r2, counts=True)
    assert counts[3] > 0 and counts.tolist() == counts_asked.tolist()
    assert np.array_equal(knob, asked, equal_nan=True) and not np.array_equal(knob, plain, equal_nan=True)
    eng = bx.MnnEngine()
    try:
        eng.upload(synth_batches(5, [1200, 900], 100), restrict=[None, np.arange(1, 801)])
        eng.run(var_adj=True, sigma=SIGMA)
        assert eng.var_adj_strict_cells()[0] > 0
    finally:
        eng.close()
    rng = np.random.default_rng(100037)
    res = bx.mnnCorrect(rng.standard_normal((60, 300)), rng.standard_normal((60, 250)) + 0.5, cos_norm_in=False,
                        cos_norm_out=False)
    assert res.strict_cells[0, 0] > 0
    dev("asv_strict", -1)
    _, counts = nat.adjust_shift_variance(a, b, v, SIGMA, r1, r2, counts=True)
    assert counts.tolist() == [-1, -1, -1, -1]


def _engine_snapshot_share(oracle, strict):
    import batchelor_amd as bx
    B = synth_batches(5, [1200, 900], 100)
    eng = bx.MnnEngine()
    try:
        eng.upload(B, restrict=[None, np.arange(1, 801)])
        eng.set_snapshot(0)
        eng.run(var_adj=True, sigma=SIGMA, var_adj_strict=strict)
        snap = eng.snapshot_var_adj()
        modes = eng.snapshot_var_adj_modes(snap["right"].shape[0])
        cells = eng.var_adj_strict_cells()
    finally:
        eng.close()
    ref = oracle.adjust_shift_variance(snap["left"].T, snap["right"].T, snap["correction"], SIGMA, snap["restrict1"],
                                       snap["restrict2"])
    close = np.isclose(snap["scaling"], ref, rtol=1e-8, atol=1e-12, equal_nan=True)
    return snap["scaling"], ref, modes, cells, float(close.mean())


def test_engine_strict_merge_is_the_oracles(oracle, dev):
    """MnnEngine.run(var_adj_strict=True): the snapshot merge's scalings against the oracle on the snapshot's own inputs."""
    dev("asv_fast", 1)
    dev("asv_cap", 0)
    dev("asv_modes", 900)
    got, ref, modes, cells, share = _engine_snapshot_share(oracle, True)
    print(f"engine, strict: {share:.6f} of 900 cells equal to the oracle, strict cells per merge {cells}")
    assert set(np.unique(modes).tolist()) <= {0, 1, 2}
    assert np.array_equal(got[modes > 0], ref[modes > 0], equal_nan=True)
    assert share == 1.0
    assert len(cells) == 1 and cells[0] > 0 and cells[0] == int((modes == 2).sum())
    _, _, _, cells_off, share_off = _engine_snapshot_share(oracle, False)
    print(f"engine, no strict: {share_off:.6f}")
    assert share_off < 1.0 and cells_off == [-1]


def test_mnn_correct_strict_is_the_exact_forms(dev):
    """mnnCorrect(var_adj_strict=True) with every flagged cell beyond the re-run against the same call on the exact form (the
    reference's bits).  Two batches only: a third merge would feed 1e-8 differences into another quantile walk.  Without the
    cosine normalisation: on unit vectors the squared distances (about 2) are some 20 bandwidths at the default sigma, the
    weights of 250 cells stay spread and no cell is flagged; on the raw Gaussians they are about 120 (1 200 bandwidths), every
    cell's own-batch weight sits on the cell itself and all 250 right cells are flagged."""
    import batchelor_amd as bx
    rng = np.random.default_rng(100037)
    b1 = rng.standard_normal((60, 300))
    b2 = rng.standard_normal((60, 250)) + 0.5
    kw = dict(cos_norm_in=False, cos_norm_out=False)
    exact = bx.mnnCorrect(b1, b2, **kw)
    assert exact.strict_cells.tolist() == [[-1, -1]]
    dev("asv_fast", 1)
    dev("asv_cap", 0)
    strict = bx.mnnCorrect(b1, b2, var_adj_strict=True, **kw)
    plain = bx.mnnCorrect(b1, b2, **kw)
    print("mnnCorrect strict cells per merge and call:", strict.strict_cells.tolist())
    assert np.allclose(strict.corrected, exact.corrected, rtol=1e-7, atol=1e-12)
    assert not np.allclose(plain.corrected, exact.corrected, rtol=1e-7, atol=1e-12)
    assert strict.strict_cells[0, 0] > 0 and plain.strict_cells.tolist() == [[-1, -1]]
    # the defaults (cosine normalisation on): no cell is beyond the re-run there, and strict leaves the call what the tiled
    # form makes of it -- the exact form's result to rounding
    dev("asv_fast", 0)
    exact_cos = bx.mnnCorrect(b1, b2)
    dev("asv_fast", 1)
    strict_cos = bx.mnnCorrect(b1, b2, var_adj_strict=True)
    assert strict_cos.strict_cells[0, 0] >= 0
    assert np.allclose(strict_cos.corrected, exact_cos.corrected, rtol=1e-7, atol=1e-12)
