"""multiBatchPCA's subset_row / get_all_genes / get_variance on the device (csrc/pca.hip: PcaGenes and its kernel) and
through fastMNN, against the longdouble restatement of tests/pca_genes_ref.py, which derives the allowances;
tests/test_cpu_pca_genes.py holds a float64 restatement to them on every input used here and shows that they reject
planted faults.  The checks are identities on whatever `fit` returned (its own pcs, d and centers), so there is no sign
alignment and no spectral gap; every test prints the device's error / allowance and asserts that it is at most 1."""
import functools

import numpy as np
import pytest

import batchelor_amd as bx
from batchelor_amd import _lib
from tests import pca_genes_ref as ref

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def device_record(name):
    c, B, subset1 = ref.case(name)
    return bx.multiBatchPCA(*B, iters=c.iters, subset_row=subset1, get_all_genes=True, get_variance=True, **c.kwargs())


@pytest.mark.parametrize("name", ref.DEVICE)
def test_extension_identity_centres_and_variance(name):
    c, B, subset1 = ref.case(name)
    out = device_record(name)
    assert out["path"] == "device", out["path"]
    assert out["rotation"].shape == (c.G_all, c.d) and out["centers"].shape == (c.G_all,)
    r = ref.ratios(ref.reference(name), out)
    print(f"case {name}: device error / allowance {r}")
    assert all(v <= 1.0 for v in r.values()), r
    assert np.array_equal(out["var_explained"], out["d"] ** 2 / len(B))


def test_scale_of_a_cell_that_is_zero_on_the_subset_reaches_the_other_rows():
    c, B, subset1 = ref.case("f")
    ex = ref.reference("f")
    b, cell = c.zero_subset
    assert float(ex.scale[b][cell]) == 1e8 and np.abs(B[b][ex.left, cell]).min() > 0
    # what that one cell adds to mu_L is far above the allowance: the check above would not pass without it
    share = float((ex.w[b] / ex.w.sum() * np.abs(ex.yL[b][:, cell]) / ex.n[b] / ex.centers_left_allow()).min())
    print(f"case f: the zero-subset cell's share of mu_L is at least {share:.3g} allowances")
    assert share > 1e6


def _stream(B, subset1, c, block):
    """The handles driven directly: subset rows resident, the others in blocks of `block` cells (None: whole batches)."""
    sub, left = ref.split_rows(c.G_all, subset1)
    w = ref.pca_ref.weight_vector(c.sizes, c.weights)
    pca = bx.DevicePCA(sub.size)
    try:
        for m, wi in zip(B, w):
            pca.add_batch(m[sub], weight=wi, cos_norm=c.cos_norm)
        out = pca.fit(d=c.d, iters=c.iters)
        out["pcs"] = [pca.project(b) for b in range(len(B))]
        genes = pca.genes(left.size)
        try:
            for b, m in enumerate(B):
                genes.begin_batch(b)
                step = m.shape[1] if block is None else block
                for lo in range(0, m.shape[1], step):
                    genes.add_block(m[left][:, lo:lo + step])
            cen, rot = genes.finish()
            total = genes.total_variance()
        finally:
            genes.close()
    finally:
        pca.close()
    full_rot, full_cen = np.zeros((c.G_all, c.d)), np.zeros(c.G_all)
    full_rot[sub], full_cen[sub] = out["rotation"], out["centers"]
    full_rot[left], full_cen[left] = rot, cen
    out.update(rotation=full_rot, centers=full_cen, var_total=total / len(B), var_explained=out["d"] ** 2 / len(B))
    return out


def test_blocks_of_any_size_and_bitwise_repeat():
    """Case a fed whole, in blocks of 37 cells (offsets into the norms that are multiples of nothing, a ragged last
    32-cell step) and cell by cell: each within the allowance; the same run twice gives the same bits."""
    c, B, subset1 = ref.case("a")
    ex = ref.reference("a")
    runs = {block: _stream(B, subset1, c, block) for block in (None, 37, 1)}
    for block, out in runs.items():
        r = ref.ratios(ex, out)
        print(f"case a, blocks of {block} cells: device error / allowance {r}")
        assert all(v <= 1.0 for v in r.values()), (block, r)
    again = _stream(B, subset1, c, 37)
    same = {k: bool(np.array_equal(runs[37][k], again[k])) for k in ("rotation", "centers", "d", "var_total")}
    print(f"case a, blocks of 37 cells, a second run: bitwise equal {same}")
    assert all(same.values()), same
    front = device_record("a")     # the front end feeds whole batches
    assert np.array_equal(front["rotation"], runs[None]["rotation"]) and np.array_equal(front["centers"], runs[None]["centers"])
    assert front["var_total"] == runs[None]["var_total"]


@pytest.mark.parametrize("name", ["a", "c"])
def test_subset_row_is_the_call_on_the_subset(name):
    c, B, subset1 = ref.case(name)
    out = device_record(name)
    sliced = bx.multiBatchPCA(*[x[subset1 - 1] for x in B], iters=c.iters, **c.kwargs())
    assert out["path"] == "device" and sliced["path"] == "device"
    same = {"d": np.array_equal(out["d"], sliced["d"]),
            "pcs": all(np.array_equal(p, q) for p, q in zip(out["pcs"], sliced["pcs"])),
            "centers": np.array_equal(out["centers"][subset1 - 1], sliced["centers"]),
            "rotation": np.array_equal(out["rotation"][subset1 - 1], sliced["rotation"])}
    print(f"case {name}: subset_row= against the sliced call, bitwise equal: {same}")
    assert all(same.values()), same
    only = bx.multiBatchPCA(*B, iters=c.iters, subset_row=subset1, **c.kwargs())   # no get_all_genes: the subset's rows
    assert np.array_equal(only["rotation"], sliced["rotation"]) and "var_total" not in only


def test_fallback_to_the_host_path_carries_the_arguments():
    c, B, subset1 = ref.case("e")
    out = bx.multiBatchPCA(*B, iters=c.iters, subset_row=subset1, get_all_genes=True, get_variance=True, **c.kwargs())
    assert out["path"].startswith("host"), out["path"]
    direct = bx.multiBatchPCA_host(*B, d=c.d, weights=c.weights, subset_row=subset1, get_all_genes=True, get_variance=True)
    for k in ("rotation", "centers", "d", "var_total", "var_explained"):
        assert np.array_equal(out[k], direct[k]), k
    assert out["rotation"].shape == (c.G_all, c.d) and [p.shape for p in out["pcs"]] == [(n, c.d) for n in c.sizes]
    ex = ref.reference("e")
    r = {"centers_left": ref.pca_ref.worst(out["centers"][ex.left] - ex.centers_left(), ex.centers_left_allow()),
         "var_total": float(abs(out["var_total"] - ex.var_total(out)) / ex.var_total_allow(out))}
    print(f"case e (host path): error / allowance {r}")
    assert all(v <= 1.0 for v in r.values()), r
    assert np.array_equal(out["var_explained"], out["d"] ** 2 / len(B))


def test_cosine_norm_takes_the_subset_first():
    c, B, subset1 = ref.case("a")
    x = B[0]
    got = bx.cosineNorm(x, mode="all", subset_row=subset1)
    want = bx.cosineNorm(x[subset1 - 1], mode="all")
    assert got["matrix"].shape == (c.nS, x.shape[1])
    assert np.array_equal(got["matrix"], want["matrix"]) and np.array_equal(got["l2norm"], want["l2norm"])
    # |S| squares summed in any order and a root, on either side: (|S| + 2) u each, relative
    assert np.allclose(got["l2norm"], np.sqrt((x[subset1 - 1] ** 2).sum(axis=0)), rtol=2 * (c.nS + 2) * ref.U, atol=0)


# ------------------------------------------------------------------------------------- fastMNN end to end
@functools.lru_cache(maxsize=None)
def _fastmnn_inputs():
    rng = np.random.default_rng(11)
    subset1 = rng.permutation(130)[:64] + 1
    load = rng.standard_normal((130, 6)) * np.linspace(3.0, 1.0, 6)
    B = [load @ rng.standard_normal((6, n)) + 0.3 * rng.standard_normal((130, n)) + 3.0 + 0.2 * i
         for i, n in enumerate((150, 170))]
    return B, subset1


def _check_fastmnn(full, sliced, B, subset1, batch_of_cell):
    assert np.array_equal(full.corrected, sliced.corrected)
    assert len(full.merge_info.pairs) == len(sliced.merge_info.pairs)
    for (a, b), (p, q) in zip(full.merge_info.pairs, sliced.merge_info.pairs):
        assert np.array_equal(a, p) and np.array_equal(b, q)
    assert np.array_equal(full.merge_info.lost_var, sliced.merge_info.lost_var)
    assert full.rotation.shape == (130, 10) and full.centers.shape == (130,)
    assert np.array_equal(full.rotation[subset1 - 1], sliced.rotation)
    assert sliced.var_total is None and sliced.var_explained is None
    assert full.var_explained.shape == (10,) and full.var_total > 0
    rows, cells = np.array([129, 0, 5, 64]), np.arange(0, 320, 7)
    assert np.array_equal(full.reconstructed(rows, cells), full.rotation[rows] @ full.corrected[cells].T)
    assert full.reconstructed().shape == (130, 320)
    # the leftover rows against the run's own PCA record: the same arguments give the same record, bit for bit
    rec = bx.multiBatchPCA(*B, d=10, cos_norm=True, subset_row=subset1, get_all_genes=True, get_variance=True)
    assert np.array_equal(rec["rotation"], full.rotation) and np.array_equal(rec["centers"], full.centers)
    assert rec["var_total"] == full.var_total and np.array_equal(rec["var_explained"], full.var_explained)
    r = ref.ratios(ref.exact(B, subset1, None, True), rec)
    print(f"fastMNN's PCA record: device error / allowance {r}")
    assert all(v <= 1.0 for v in r.values()), r


def test_fastmnn_with_a_subset_corrects_all_genes():
    B, subset1 = _fastmnn_inputs()
    full = bx.fastMNN(*B, d=10, k=5, subset_row=subset1, correct_all=True, get_variance=True)
    sliced = bx.fastMNN(*[x[subset1 - 1] for x in B], d=10, k=5)
    _check_fastmnn(full, sliced, B, subset1, None)


def test_fastmnn_single_object_with_a_subset():
    B, subset1 = _fastmnn_inputs()
    batch = np.array(["p", "q"])[(np.arange(320) * 7 % 320 >= 150).astype(int)]    # interleaved, 150 and 170 cells
    assert (batch == "p").sum() == 150
    x = np.empty((130, 320))
    x[:, batch == "p"], x[:, batch == "q"] = B[0], B[1]
    full = bx.fastMNN(x, batch=batch, d=10, k=5, subset_row=subset1, correct_all=True, get_variance=True)
    sliced = bx.fastMNN(x[subset1 - 1], batch=batch, d=10, k=5)
    _check_fastmnn(full, sliced, B, subset1, batch)
    host = bx.fastMNN(x, batch=batch, d=10, k=5, subset_row=subset1, correct_all=True, get_variance=True, pca="host")
    assert host.rotation.shape == (130, 10) and host.var_explained.shape == (10,) and host.var_total > 0


# ------------------------------------------------------------------------------------- misuse
def test_misuse_is_an_error_never_a_wrong_answer():
    c, B, subset1 = ref.case("b")
    sub, left = ref.split_rows(c.G_all, subset1)
    pca = bx.DevicePCA(sub.size)
    try:
        for m in B:
            pca.add_batch(m[sub])
        with pytest.raises(_lib.BatchelorMI355XError, match="bmx_pca_fit has not been run"):
            pca.genes(left.size)
        pca.fit(d=c.d, iters=1)
        genes = pca.genes(left.size)
        try:
            with pytest.raises(_lib.BatchelorMI355XError, match="bmx_pca_genes_begin_batch has not been called"):
                genes.add_block(B[0][left])
            with pytest.raises(_lib.BatchelorMI355XError, match="must be begun in order"):
                genes.begin_batch(1)
            genes.begin_batch(0)
            with pytest.raises(_lib.BatchelorMI355XError, match="does not fit into the batch announced"):
                genes.add_block(B[1][left])                  # two cells into a batch of one
            genes.add_block(B[0][left])
            with pytest.raises(_lib.BatchelorMI355XError, match="batch index out of range"):
                genes.begin_batch(4)
            with pytest.raises(_lib.BatchelorMI355XError, match="has not received all its cells"):
                genes.finish()                               # three batches have not come at all
            genes.begin_batch(1)
            genes.add_block(B[1][left][:, :1])
            with pytest.raises(_lib.BatchelorMI355XError, match="previous batch has not received all its cells"):
                genes.begin_batch(2)
            genes.add_block(B[1][left][:, 1:])
            for b in (2, 3):
                genes.begin_batch(b)
                genes.add_block(B[b][left][:, :40])
                if b == 3:
                    with pytest.raises(_lib.BatchelorMI355XError, match="has not received all its cells"):
                        genes.finish()                       # the last batch is short of cells
                genes.add_block(B[b][left][:, 40:])
            cen, rot = genes.finish()                        # and the handle is still good
            assert rot.shape == (left.size, c.d) and np.all(np.isfinite(rot))
            pca.add_batch(B[0][sub])                         # the PCA moves on: the handle must not read it again
            for call in (genes.finish, genes.total_variance, lambda: genes.begin_batch(0)):
                with pytest.raises(_lib.BatchelorMI355XError, match="re-fitted or given a batch"):
                    call()
        finally:
            genes.close()
    finally:
        pca.close()
