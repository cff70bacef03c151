"""kmeans() on the device against its numpy restatement (tests/kmeans_ref.py).

The device takes a distance as |c|^2 - 2 x.c on the FP64 matrix cores; the restatement takes sum((x - c)^2) directly.  Where
two centres are nearly equally near the two may choose differently, so a single assignment is held to near-optimality
within the rounding bound of the expanded form, exact ties are tested on integer data where both forms are exact, and
whole runs are compared on inputs whose smallest tie margin (measured on the restatement alone) is orders above that bound.
"Relative" below is the project's max |a - b| / max |b|."""
import warnings

import numpy as np
import pytest

from tests.kmeans_ref import direct_distances, kmeans_ref
from tests.test_cpu_kmeans import blobs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bx():
    import batchelor_amd
    return batchelor_amd


def rel(a, b):
    top = float(np.abs(b).max())
    return float(np.abs(a - b).max()) / (top if top > 0 else 1.0)


def quiet(fn, *args, **kw):
    """fn(...) with the 'did not converge' warning of a run cut short on purpose put aside."""
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message="did not converge")
        return fn(*args, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# one assignment
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 1e3, 1e-3])
@pytest.mark.parametrize("n,d,K", [(1, 1, 1), (63, 3, 2), (65, 4, 15), (257, 50, 17), (1000, 130, 33), (2051, 10, 257),
                                   (1500, 5, 1024)])
def test_one_assignment_is_near_optimal(bx, n, d, K, scale):
    rng = np.random.default_rng(1000 * n + K)
    x = rng.normal(size=(n, d)) * scale + 5.0 * scale
    init = x[rng.choice(n, K, replace=False)]
    out = quiet(bx.kmeans, x, init, iter_max=1)
    assert out.iter == 1 and not out.converged
    chosen = out.cluster.astype(np.int64) - 1
    assert chosen.min() >= 0 and chosen.max() < K
    D = direct_distances(x, init)
    got = D[np.arange(n), chosen]
    bound = (d + 4) * 2.0 ** -52 * ((x * x).sum(1) + (init[chosen] ** 2).sum(1))
    excess = got - D.min(axis=1)
    print(f"n={n} d={d} K={K} scale={scale}: max excess / bound = {float((excess / bound).max()):.3g}, "
          f"labels off the direct argmin: {int((chosen != D.argmin(1)).sum())}")
    assert (excess <= bound).all()      # every observation


def test_exact_ties_go_to_the_lowest_index(bx):
    """Integer data: every product and sum is exact in both forms, so the labels are those of the restatement bit for bit.
    Ties between centres of one lane (3, 19), of different 16-wide sub-tiles (3 vs 20, 15 vs 16), of different 64-wide tiles
    (2 vs 66), and three-way."""
    K, d = 70, 4
    c = np.zeros((K, d))
    c[:, 0] = 100.0 * np.arange(K)
    c[19] = [300, 10, 10, 0]
    c[20] = [300, 20, 0, 0]
    c[16] = [1500, 20, 0, 0]
    c[21] = [500, 20, 0, 0]
    c[22] = [510, 10, 0, 0]
    c[66] = [200, 0, 20, 0]
    ties = np.array([[300, 10, 0, 0],      # 3, 19, 20
                     [300, 10, 0, 7],      # 3, 19, 20
                     [300, 15, 5, 0],      # 19, 20
                     [1500, 10, 0, 0],     # 15, 16
                     [1500, 10, -3, 2],    # 15, 16
                     [500, 10, 0, 0],      # 5, 21, 22
                     [505, 15, 1, 1],      # 21, 22
                     [200, 0, 10, 0],      # 2, 66
                     [200, 3, 10, -4],     # 2, 66
                     [6650, 0, 0, 0]], dtype=np.float64)   # untied: 67
    x = np.vstack([ties, c, np.tile(ties, (20, 1))])        # more than one workgroup, every centre has a member
    ref = kmeans_ref(x, c, iter_max=1)
    D = direct_distances(ties, c)
    ntied = (D == D.min(1, keepdims=True)).sum(1)
    assert ntied.tolist() == [3, 3, 2, 2, 2, 3, 2, 2, 2, 1] and ref.margin == 0.0
    assert (ref.cluster[:10] - 1).tolist() == [3, 3, 19, 15, 15, 5, 21, 2, 2, 67]
    out = quiet(bx.kmeans, x, c, iter_max=1)
    assert np.array_equal(out.cluster, ref.cluster)
    assert np.array_equal(out.size, ref.size)


# ---------------------------------------------------------------------------------------------------------------------
# whole runs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("n,d,K", [(1000, 3, 17), (2051, 50, 33), (1500, 130, 15), (4099, 10, 257)])
def test_whole_run_equals_the_restatement(bx, n, d, K, seed):
    x = blobs(seed, n, d, K, spread=1.5, noise=1.0)
    init = x[np.random.default_rng(seed).choice(n, K, replace=False)]
    ref = kmeans_ref(x, init, iter_max=100)
    print(f"n={n} d={d} K={K} seed={seed}: restatement margin {ref.margin:.3g}, iter {ref.iter}, converged {ref.converged}")
    assert ref.margin > 1e-9       # the condition under which the two forms of the distance must agree on every label
    out = quiet(bx.kmeans, x, init, iter_max=100)
    assert np.array_equal(out.cluster, ref.cluster)
    assert out.iter == ref.iter and out.converged == ref.converged
    assert np.array_equal(out.size, ref.size)
    print(f"  centres {rel(out.centers, ref.centers):.3g}, withinss {rel(out.withinss, ref.withinss):.3g}")
    assert rel(out.centers, ref.centers) <= 1e-12
    assert rel(out.withinss, ref.withinss) <= 1e-12
    assert abs(out.tot_withinss - ref.tot_withinss) <= 1e-12 * ref.tot_withinss


@pytest.mark.parametrize("n,d,K", [(1, 1, 1), (700, 7, 1), (3000, 70, 40), (2500, 600, 9), (1_100_000, 2, 5)])
def test_invariants_of_an_unconverged_run(bx, n, d, K):
    """Two assignments: the centres are the means of the returned labels whatever the state of the run.  (1 100 000
    observations: the ranking pass walks chunks of more than 256.)"""
    x = blobs(n % 1000 + K, n, d, K)
    init = x[np.random.default_rng(K).choice(n, K, replace=False)]
    out = quiet(bx.kmeans, x, init, iter_max=2)
    lab = out.cluster.astype(np.int64) - 1
    assert out.iter == 2 and out.cluster.dtype == np.int32 and lab.min() >= 0 and lab.max() < K
    size = np.bincount(lab, minlength=K)
    assert np.array_equal(out.size, size) and size.min() > 0
    means = np.stack([np.bincount(lab, weights=x[:, k], minlength=K) for k in range(d)], axis=1) / size[:, None]
    diff = x - means[lab]
    wss = np.bincount(lab, weights=np.einsum("ik,ik->i", diff, diff), minlength=K)
    print(f"n={n} d={d} K={K}: centres {rel(out.centers, means):.3g}, withinss {rel(out.withinss, wss):.3g}")
    assert rel(out.centers, means) <= 1e-12
    assert rel(out.withinss, wss) <= 1e-12
    assert abs(out.tot_withinss - out.withinss.sum()) <= 1e-12 * out.tot_withinss if n > 1 else out.tot_withinss == 0.0
    assert abs(out.tot_withinss - wss.sum()) <= 1e-12 * wss.sum() if n > 1 else True
    assert set(out.stats["stage_ms"]) == {"upload", "assign", "update", "withinss", "download"}


@pytest.mark.parametrize("d", [1, 65])
def test_clusters_at_the_edges_of_a_wave_and_of_a_piece(bx, d):
    """Well separated clusters of 1, 63, 64 and 65 members (a wave of the update adds 64), of one piece of 256 and of a
    piece plus one member: the labels are the planted ones and the centres their means."""
    sizes = np.array([1, 63, 64, 65, 256, 257])
    K = sizes.size
    rng = np.random.default_rng(40 + d)
    planted = np.zeros((K, d))
    planted[:, 0] = 100.0 * np.arange(K)
    lab = rng.permutation(np.repeat(np.arange(K), sizes))
    x = planted[lab] + rng.normal(size=(lab.size, d))
    out = quiet(bx.kmeans, x, planted + 0.5, iter_max=2)
    assert np.array_equal(out.cluster.astype(np.int64) - 1, lab) and np.array_equal(out.size, sizes)
    means = np.stack([np.bincount(lab, weights=x[:, k], minlength=K) for k in range(d)], axis=1) / sizes[:, None]
    diff = x - means[lab]
    wss = np.bincount(lab, weights=np.einsum("ik,ik->i", diff, diff), minlength=K)
    print(f"sizes {sizes.tolist()} d={d}: centres {rel(out.centers, means):.3g}, withinss {rel(out.withinss, wss):.3g}")
    assert rel(out.centers, means) <= 1e-12
    assert rel(out.withinss, wss) <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# reproducibility, starts, blocks
# ---------------------------------------------------------------------------------------------------------------------
def same(a, b):
    return (np.array_equal(a.cluster, b.cluster) and np.array_equal(a.centers, b.centers)
            and np.array_equal(a.withinss, b.withinss) and a.tot_withinss == b.tot_withinss
            and np.array_equal(a.size, b.size) and a.iter == b.iter and a.converged == b.converged)


def test_runs_are_reproducible_and_the_best_start_is_kept(bx):
    from batchelor_amd.kmeans import start_indices
    n, d, K = 3001, 20, 12
    x = blobs(77, n, d, K)
    a = quiet(bx.kmeans, x, K, iter_max=5, nstart=4, seed=9)
    b = quiet(bx.kmeans, x, K, iter_max=5, nstart=4, seed=9)
    assert same(a, b)
    singles = [quiet(bx.kmeans, x, x[idx], iter_max=5) for idx in start_indices(n, K, 4, 9)]
    tots = [s.tot_withinss for s in singles]
    print("tot_withinss of the four starts:", tots, "kept:", a.stats["start"])
    assert a.stats["start"] == int(np.argmin(tots)) and same(a, singles[a.stats["start"]])
    one = quiet(bx.kmeans, x, K, iter_max=5, nstart=1, seed=9)
    assert one.stats["start"] == 0 and same(one, singles[0])


def test_blocked_upload_changes_nothing(bx):
    from batchelor_amd.kmeans import _KmeansHandle
    x = blobs(5, 2000, 33, 6)
    init = x[:6]
    res = []
    for block_bytes in (None, 33 * 8 * 300):
        h = _KmeansHandle(x, 0, block_bytes=block_bytes)
        try:
            res.append(h.run(init, 3))
        finally:
            h.close()
    assert same(res[0], res[1])


# ---------------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_handle_usable(bx):
    from batchelor_amd.kmeans import _KmeansHandle
    x = blobs(3, 500, 4, 3)
    good = x[[0, 10, 20]]
    far = np.vstack([x[:2], np.full((1, 4), 1e6)])
    h = _KmeansHandle(x, 0)
    try:
        first = h.run(good, 10)
        with pytest.raises(bx.BatchelorMI355XError, match="empty cluster: try a better set of initial centers") as e:
            h.run(far, 10)
        assert e.value.code == -6
        with pytest.raises(bx.BatchelorMI355XError, match="initial centers are not distinct"):
            h.run(x[[0, 10, 0]], 10)
        with pytest.raises(bx.BatchelorMI355XError, match=r"1 <= K <= min\(n, 1024\)"):
            h.run(np.vstack([x, x[:1] + 1.0]), 10)            # K = n + 1
        with pytest.raises(bx.BatchelorMI355XError, match="'iter_max' must be positive"):
            h.run(good, 0)
        with pytest.raises(bx.BatchelorMI355XError, match="'centers' must be finite"):
            h.run(np.where(np.eye(3, 4) > 0, np.nan, good), 10)
        with pytest.raises(bx.BatchelorMI355XError, match="already holds its observations"):
            h._call("begin", __import__("ctypes").c_int64(5))
        assert same(h.run(good, 10), first)
    finally:
        h.close()
    big = np.arange(1100.0)[:, None]
    h = _KmeansHandle(big, 0)
    try:
        with pytest.raises(bx.BatchelorMI355XError, match=r"1 <= K <= min\(n, 1024\)"):
            h.run(big[:1025], 10)                              # K > 1024
        assert h.run(big[:1024], 1).size.sum() == 1100
    finally:
        h.close()
    with pytest.raises(ValueError, match="empty cluster"):
        kmeans_ref(x, far)                                     # the restatement agrees on the errors
    with pytest.raises(bx.BatchelorMI355XError, match="empty cluster"):
        bx.kmeans(x, far)
    with pytest.raises(bx.BatchelorMI355XError, match="not distinct"):
        bx.kmeans(np.vstack([x[:5], x[:5]]), 10, seed=0)       # ten rows, five distinct: every draw of ten has twins
    with pytest.raises(ValueError, match="more cluster centers than observations"):
        bx.kmeans(x[:3], 4)
    with pytest.raises(ValueError, match="at most 1024 centers"):
        bx.kmeans(big, 1025)
