"""The split-bf16 candidate tier (csrc/knn_bf16.hip, its prep in csrc/knn_prep.hip) at its edges, every search forced to it with
the testing hook "knn_tier" = 2: indices and distances equal to the oracle's, bitwise, as test_gpu_knn.py holds query_knn.

Forced to tier 2, a query that fails the certificate goes on to the exact FP64 paths and still matches the oracle, so a broken
image or filter could hide as fall-backs.  Two conditions keep that from happening:
  * every case: last_knn_exact_fallbacks() <= nq // 100 (test_gpu_knn.py's bound for this data: Gaussian rows at unit scale
    are far inside the split-bf16 error bound);
  * the cases whose searches run a single reference range (force_c = 1, or fewer than 4096 references and no force_c): the
    count equals the one recorded in tests/golden/knn_bf16_edges_parent.json with the library of the commit before this tier
    was split by role (its "source" field says which).  Such a search shares no thresholds between workgroups, so the count is
    deterministic.  Multi-range cases are not pinned: the shared threshold tau_g is racy by design.
Every shape uses the data of seed SEED: none of them exceeded nq // 100 with the recorded library, so no seed was replaced."""
import json
import os

import numpy as np
import pytest

from tests.conftest import synth_batches
from tests.find_knn_ref import find_knn_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "knn_bf16_edges_parent.json")
SEED = 31


def _case(nr, nq, d, k, sample=None, force_c=None):
    name = f"nr{nr}-nq{nq}-d{d}-k{k}"
    if sample is not None:
        name += f"-sample{sample}-c{force_c}"
    return {"id": name, "nr": nr, "nq": nq, "d": d, "k": k, "sample": sample, "force_c": force_c}


# every fragment-count class at its largest d (NS = 1, 2, 3, 4, 6, 8, 10, 13, 16, 19, 24), lists of 24; lists of 40 where the
# kernel has them (NS <= 16).  1000 references, one full query block of either workgroup (256 / 128 queries) plus one query.
CLASS_D = (4, 9, 15, 20, 31, 41, 52, 68, 84, 100, 127)
CLASSES = [_case(1000, 257, d, 20) for d in CLASS_D] + [_case(1000, 257, d, 30) for d in CLASS_D if d <= 84]
# the producers and the ring: 49 references are the fewest the tier takes (two tiles, the second padded with +inf rows), 300
# the first wrap of the 8-slot ring, 352 / 384 / 416 are 11 / 12 / 13 tiles: either side of the producers' 3 x NPROD rotation
RING = [_case(nr, nq, 50, 20) for nr in (49, 300, 352, 384, 416) for nq in (1, 31, 257)]
# the sample pass (none, a short one, the usual one) against 1, 2 and 5 reference ranges with shared thresholds
SAMPLE = [_case(3000, 300, 50, 20, sample=s, force_c=c) for s in (0, 64, 1024) for c in (1, 2, 5)]
FIND_KNN_ID = "find_knn-n1500-d50-k20"


def single_range(case):
    return case["force_c"] == 1 or (case["force_c"] is None and case["nr"] < 4096)


def run_case(nb, dev_set, case):
    """The search of a case, forced to tier 2 -> (X, Q, idx, dist, queries that went to the exact paths)."""
    dev_set("knn_tier", 2)
    if case["sample"] is not None:
        dev_set("sample", case["sample"])
        dev_set("force_c", case["force_c"])
    X, Q = synth_batches(SEED, [case["nr"], case["nq"]], case["d"])
    idx, dist = nb.query_knn(X, Q, case["k"])
    return X, Q, idx, dist, nb.last_knn_exact_fallbacks()


def run_find_knn(nb, dev_set):
    dev_set("knn_tier", 2)
    X, = synth_batches(SEED, [1500], 50)
    idx, dist = nb.find_knn(X, 20)
    return X, idx, dist, nb.last_knn_exact_fallbacks()


@pytest.fixture(scope="module")
def nb():
    from batchelor_amd import neighbors
    return neighbors


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)["fallbacks"]


def test_every_single_range_case_is_recorded(recorded):
    assert sorted(recorded) == sorted([c["id"] for c in CLASSES + RING + SAMPLE if single_range(c)] + [FIND_KNN_ID])


@pytest.mark.parametrize("case", CLASSES + RING + SAMPLE, ids=lambda c: c["id"])
def test_tier2_matches_oracle(oracle, nb, dev, recorded, case):
    X, Q, idx, dist, fallbacks = run_case(nb, dev, case)
    oi, od = oracle.query_knn(X, Q, case["k"])
    print(f"{case['id']}: {fallbacks} of {case['nq']} queries to the exact paths")
    assert np.array_equal(idx, oi)
    assert np.array_equal(dist, od)
    assert fallbacks <= case["nq"] // 100
    if single_range(case):
        assert fallbacks == recorded[case["id"]]


def test_find_knn_through_the_bf16_prep(oracle, nb, dev, recorded):
    # the self-search path (seeded with each row's distance to itself) through knn_prep_bf16
    X, idx, dist, fallbacks = run_find_knn(nb, dev)
    ri, rd = find_knn_ref(oracle, X, 20, None)
    print(f"{FIND_KNN_ID}: {fallbacks} of 1500 queries to the exact paths")
    assert np.array_equal(idx, ri)
    assert np.array_equal(dist, rd)
    assert fallbacks <= 1500 // 100
    assert fallbacks == recorded[FIND_KNN_ID]
