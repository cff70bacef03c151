"""batchelor_amd.inputs without a GPU or the library: the messages every front end gives for malformed arguments before
it asks for a device, divide_into_batches / reindex_pairings against the independent restatements (oracle/, tests/*_ref.py),
and the packing of restrictions for the C ABI."""
import ctypes

import numpy as np
import pytest

from oracle import fastmnn_oracle as orc
from tests import linear_correct_ref as lin_ref

RNG = np.random.default_rng(20240)
G, D = 12, 4
A, B = RNG.normal(size=(G, 9)), RNG.normal(size=(G, 11))          # genes x cells
X = np.concatenate([A, B], axis=1)
BATCH = np.repeat([1, 2], [9, 11])
FIRST = [np.arange(1, 10)]                                        # a restriction that leaves batch 2 without cells
CL = [np.arange(9) % 2, np.arange(11) % 2]

TWO = "at least two batches must be specified"
NEED_BATCH = "'batch' must be specified if '...' has only one object"
ROWS = "number of rows is not the same across batches"
COLS = "number of columns is not the same across batches"
RLEN = "'restrictions' must of length equal to the number of batches"
EMPTY = "no cells remaining in a batch after restriction"
NAMES = "names of batches should be unique"
SUBSET = "subset indices out of range"
RANGE = "'restrict' indices out of range"


def _gene_space(fn, kw, names=True, subset=True, ncol="'length(batch)' and 'ncol(x)' are not the same"):
    """The cases of a front end that takes genes x cells batches and checks everything before it asks for a device."""
    rows = [(fn, (), {}, TWO), (fn, (A,), {}, NEED_BATCH), (fn, (A, B[:5]), {}, ROWS), (fn, (A, B), {"restrict": [None]}, RLEN),
            (fn, (X,), {"batch": BATCH, "restrict": FIRST}, EMPTY), (fn, (X,), {"batch": BATCH[:-1]}, ncol)]
    if names:
        rows.append((fn, (A, B), {"names": ["a", "a"]}, NAMES))
    if subset:
        rows.append((fn, (A, B), {"subset_row": [0, 1]}, SUBSET))
    return [(f, a, dict(kw(a), **k), m) for f, a, k, m in rows]


def _clusters(args):
    return {"clusters": CL[:max(1, len(args))] if len(args) != 1 else [np.concatenate(CL)[:args[0].shape[1]]]}


LINEAR_BATCH = "'length(batch)' should be equal to number of cells in '...'"
PINNED = (
    # fastMNN: the PCA comes before the restrictions and the names, so those need a device
    [("fastMNN", (), {}, TWO), ("fastMNN", (A,), {}, NEED_BATCH), ("fastMNN", (A, B[:5]), {}, ROWS),
     ("fastMNN", (X,), {"batch": BATCH[:-1]}, "'length(batch)' and 'ncol(x)' are not the same")]
    + [("reducedMNN", (), {}, TWO), ("reducedMNN", (A.T,), {}, NEED_BATCH), ("reducedMNN", (A.T, B.T[:, :5]), {}, COLS),
       ("reducedMNN", (A.T, B.T), {"restrict": [None]}, RLEN),
       ("reducedMNN", (X.T,), {"batch": BATCH, "restrict": FIRST}, EMPTY),
       ("reducedMNN", (A.T, B.T), {"names": ["a", "a"]}, NAMES),
       ("reducedMNN", (X.T,), {"batch": BATCH[:-1]}, "'length(batch)' and 'nrow(x)' are not the same")]
    + _gene_space("mnnCorrect", lambda a: {})
    + _gene_space("clusterMNN", _clusters, names=False)
    + _gene_space("rescaleBatches", lambda a: {}, ncol=LINEAR_BATCH)
    + _gene_space("regressBatches", lambda a: {}, ncol=LINEAR_BATCH)
    + [("multiBatchPCA", (), {}, "at least one batch must be specified"), ("multiBatchPCA", (A, B[:5]), {}, ROWS)]
)

# Where the front ends disagreed on malformed input that nothing pinned, all now take the strictest behaviour there was.
STRICT = [
    (fn, args, {"restrict": r}, msg)
    for fn, args in (("reducedMNN", (A.T, B.T)), ("mnnCorrect", (A, B)))
    for r, msg in (([np.ones(5, dtype=bool), None], RANGE), ([[1, 10], None], RANGE), ([[0, 1], None], RANGE))
] + [
    # restrict=[None] with a single object is no restriction: the call gets as far as the next refusal
    ("mnnCorrect", (X,), {"batch": BATCH, "restrict": [None], "svd_dim": 2}, "svd.dim"),
    ("reducedMNN", (X.T,), {"batch": BATCH, "restrict": [np.ones(5, dtype=bool)]}, RANGE),
    ("mnnCorrect", (X,), {"batch": BATCH, "restrict": [np.ones(5, dtype=bool)]}, RANGE),
    ("mnnCorrect", (X,), {"batch": BATCH, "restrict": [[1, 21]]}, RANGE),
]


def _ids(table):
    return [f"{fn}-{i}" for i, (fn, *_rest) in enumerate(table)]


def _refused(fn, args, kwargs, msg):
    import batchelor_amd as bx
    with pytest.raises(ValueError) as err:
        getattr(bx, fn)(*args, **kwargs)
    assert msg in str(err.value)
    assert not isinstance(err.value, bx.BatchelorMI355XError)  # (refused before a device was asked for)


@pytest.mark.parametrize("fn,args,kwargs,msg", PINNED, ids=_ids(PINNED))
def test_pinned_messages(fn, args, kwargs, msg):
    _refused(fn, args, kwargs, msg)


@pytest.mark.parametrize("fn,args,kwargs,msg", STRICT, ids=_ids(STRICT))
def test_strictest_behaviour_everywhere(fn, args, kwargs, msg):
    _refused(fn, args, kwargs, msg)


# ---------------------------------------------------------------------------------------------- divide_into_batches
N = 40
LEVELS = [np.array(["b", "a", "c", "solo"]), np.array([3, 1, 2])]


def _batch_vector(levels, rng):
    batch = rng.choice(levels[:3], N)
    batch[:3] = levels[:3]                       # every level is there ...
    if len(levels) > 3:
        batch[17] = levels[3]                    # ... and one has a single cell
    return batch


@pytest.mark.parametrize("levels", LEVELS, ids=["strings", "integers"])
@pytest.mark.parametrize("form", ["none", "index", "mask"])
@pytest.mark.parametrize("byrow", [True, False])
def test_divide_into_batches(levels, form, byrow):
    from batchelor_amd import inputs
    rng = np.random.default_rng(7)
    batch = _batch_vector(levels, rng)
    mask = rng.random(N) < 0.6
    mask[[0, 1, 2, 17]] = True                   # no level loses all its cells
    restrict = {"none": None, "index": rng.permutation(np.flatnonzero(mask) + 1), "mask": mask}[form]
    x = rng.normal(size=(N, 5) if byrow else (5, N))
    labels = np.arange(N) * 10
    div = inputs.divide_into_batches(x, batch, restrict, byrow=byrow, also=(labels,))
    if byrow:
        parts, lev, reorder, restricted = orc.divide_into_batches(x, batch, restrict)
    else:
        parts, restricted, lev, reorder = lin_ref.divide_by_column(x, batch, restrict)
    assert div.levels == lev and len(lev) == len(levels) and len(div.parts) == len(parts)
    for a, b in zip(div.parts, parts):
        assert np.array_equal(a, b)
    assert np.array_equal(div.reorder, reorder)
    if form == "none":
        assert div.restricted is None and restricted is None
    else:
        assert len(div.restricted) == len(restricted)
        for a, b in zip(div.restricted, restricted):
            assert a.dtype == np.int32 and np.array_equal(a, b)
    whole = np.concatenate(div.parts, axis=0 if byrow else 1)
    assert np.array_equal(whole[div.reorder - 1] if byrow else whole[:, div.reorder - 1], x)
    assert np.array_equal(np.concatenate(div.also[0])[div.reorder - 1], labels)
    if "solo" in div.levels:
        assert div.parts[div.levels.index("solo")].shape[0 if byrow else 1] == 1


def test_divide_refusals():
    from batchelor_amd import inputs
    x, batch = np.zeros((3, 6)), np.array([1, 1, 1, 2, 2, 2])
    with pytest.raises(ValueError, match="no cells remaining in a batch after restriction"):
        inputs.divide_into_batches(x, batch, [1, 2])
    with pytest.raises(ValueError, match="'restrict' indices out of range"):
        inputs.divide_into_batches(x, batch, [1, 7])
    with pytest.raises(ValueError, match="'restrict' indices out of range"):
        inputs.divide_into_batches(x, batch, np.ones(5, dtype=bool))
    with pytest.raises(ValueError, match=r"'length\(batch\)' and 'ncol\(x\)' are not the same"):
        inputs.divide_into_batches(x, batch[:-1])
    with pytest.raises(ValueError, match=r"'length\(batch\)' and 'nrow\(x\)' are not the same"):
        inputs.divide_into_batches(x, batch, byrow=True)


def test_reindex_pairings_inverts():
    from batchelor_amd import inputs
    from batchelor_amd.reduced_mnn import _reindex_pairings
    rng = np.random.default_rng(1000011)
    S = rng.permutation(40) + 1
    pairings = [(rng.integers(1, 11, 20), np.arange(11, 31)), (np.arange(30, 0, -1), rng.integers(33, 41, 30))]
    out = inputs.reindex_pairings(pairings, S)
    for (ol, orr), (pl, pr), (gl, gr) in zip(out, pairings, orc.reindex_pairings(pairings, S)):
        assert np.array_equal(S[ol - 1], pl) and np.array_equal(S[orr - 1], pr)
        assert np.array_equal(ol, gl) and np.array_equal(orr, gr)
    assert _reindex_pairings is inputs.reindex_pairings


def test_old_names_stay_importable():
    import batchelor_amd as bx
    from batchelor_amd import reduced_mnn
    assert bx.divideIntoBatches is reduced_mnn.divideIntoBatches
    d = bx.divideIntoBatches(np.arange(12.0).reshape(6, 2), ["y", "x", "y", "x", "y", "y"], [1, 2])
    assert sorted(d) == ["batches", "levels", "reorder", "restricted"] and d["levels"] == ["x", "y"]
    assert [r.tolist() for r in d["restricted"]] == [[1], [1]] and d["reorder"].tolist() == [3, 1, 4, 2, 5, 6]


# ---------------------------------------------------------------------------------------------- restrictions for the ABI
def test_restrict_index_and_list():
    from batchelor_amd import inputs
    assert inputs.restrict_index(None, 5) is None
    for r in ([2, 5, 2], np.array([False, True, False, False, True])):
        got = inputs.restrict_index(r, 5)
        assert got.dtype == np.int32 and got.tolist() == ([2, 5, 2] if isinstance(r, list) else [2, 5])
    for bad, msg in (([], EMPTY), (np.zeros(5, dtype=bool), EMPTY), ([0], RANGE), ([6], RANGE), (np.ones(4, dtype=bool), RANGE)):
        with pytest.raises(ValueError, match=msg):
            inputs.restrict_index(bad, 5)
    assert inputs.restrict_list(None, [5, 6]) is None
    with pytest.raises(ValueError, match="'restrictions' must of length"):
        inputs.restrict_list([None], [5, 6])
    got = inputs.restrict_list([None, [6, 1]], [5, 6])
    assert got[0] is None and got[1].tolist() == [6, 1]
    assert inputs.subset_index(None, 4) is None and inputs.subset_index([True, False, True, False], 4).tolist() == [1, 3]
    with pytest.raises(ValueError, match=SUBSET):
        inputs.subset_index([1, 5], 4)


def test_pack_restrictions():
    from batchelor_amd import inputs
    keep, ptrs, counts = inputs.pack_restrictions(None, 3)
    assert keep == [] and ptrs is None and counts.dtype == np.int32 and counts.tolist() == [-1, -1, -1]
    rlist = inputs.restrict_list([np.array([True, False, True, True]), None, [3, 1]], [4, 9, 3])
    keep, ptrs, counts = inputs.pack_restrictions(rlist, 3)
    assert counts.dtype == np.int32 and counts.tolist() == [3, -1, 2]
    assert not ptrs[1] and keep[1] is None
    del rlist
    for b, want in ((0, [1, 3, 4]), (2, [3, 1])):
        assert keep[b].dtype == np.int32 and keep[b].flags.c_contiguous and ptrs[b] == keep[b].ctypes.data
        seen = np.ctypeslib.as_array(ctypes.cast(ptrs[b], ctypes.POINTER(ctypes.c_int32)), shape=(int(counts[b]),))
        assert seen.tolist() == want             # 1-based, read through the pointer the library gets
