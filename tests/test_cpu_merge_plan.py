"""The host-side merge plan (csrc/merge_plan.hpp) under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/host/merge_plan_host.cpp is a stand-alone program that makes no HIP call and includes no HIP header.  What it prints is
compared with what the oracle's tree walk (resolve_merge_tree / get_next_merge / update_tree), its pick_best_merge and
update_remainders' matrix, and a dictionary restatement of the restrict chains give for the same inputs."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from batchelor_amd.merge_tree import encode_postorder
from oracle import fastmnn_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BMX_ERR_SUBSET, BMX_ERR_TREE = -4, -7
TWO_CHILDREN = "merge tree structure should contain two children per node"
BAD_LEAVES = "invalid leaf nodes specified in 'merge.order'"

TREES = {  # name: (batches, merge.order)
    "two": (2, None),
    "progressive3": (3, None),
    "progressive19": (19, None),
    "balanced8": (8, [[[1, 2], [3, 4]], [[5, 6], [7, 8]]]),
    "right_deep5": (5, [1, [2, [3, [4, 5]]]]),
    "left_deep5": (5, [[[[1, 2], 3], 4], 5]),
    "out_of_order": (5, [[3, 1], [2, [5, 4]]]),
}
REJECTED = [  # (batches, code, text)
    (2, [1, 0], TWO_CHILDREN),
    (2, [1, 2], BAD_LEAVES),
    (2, [1, 1, 0], BAD_LEAVES),
    (2, [1, 3, 0], BAD_LEAVES),
    (2, [0], TWO_CHILDREN),
    (2, [1, 2, 0, 0], TWO_CHILDREN),
    (2, [], BAD_LEAVES),
    (3, [1, 2, 0], BAD_LEAVES),
]
RESTRICTS = [  # (cells, 1-based vector)
    (3, [3, 1, 2]),
    (4, [2, 2, 2]),
    (3, [1, 3, 1, 2, 3, 1]),
    (5, [4]),
    (3, [1, 0]),
    (3, [2, 4]),
]
COUNTS = [
    np.array([[0, 0, 0, 0], [5, 0, 0, 0], [9, 2, 0, 0], [4, 9, 9, 0]], dtype=np.int64),  # the maximum three times
    np.array([[0, 0], [7, 0]], dtype=np.int64),  # one remainder is left
]


@pytest.fixture(scope="module")
def run_cases(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    exe = str(tmp_path_factory.mktemp("merge_plan") / "merge_plan_host")
    # (the sanitizers' runtimes are linked statically: the program stands alone)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I" + os.path.join(ROOT, "batchelor_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "merge_plan_host.cpp"), "-o", exe], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr  # (non-zero: a sanitizer spoke)
        assert "merge plan cases done" in out.stdout
        got = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
        assert len(got) == len(lines)
        return got

    return run


def words(kind, *values):
    return " ".join([kind] + [str(int(v)) for v in values])


def oracle_walk(nbatches, merge_order):
    """The merges and the leaves in the order they are first needed, from the oracle's tree functions on integer trees: a
    finished merge is the tuple of its batch ids (get_next_merge takes anything that is no list for finished)."""
    tree = orc.resolve_merge_tree(nbatches, merge_order)
    code = encode_postorder(tree)
    row0, r = {}, 0
    for b in code[code != 0]:  # rows follow the leaves left to right; batch b has b cells
        row0[int(b)] = r
        r += int(b)

    def side(x):
        batches = list(x) if isinstance(x, tuple) else [x]
        return {"leaf": not isinstance(x, tuple), "batches": batches, "row0": row0[batches[0]], "n": sum(batches)}

    merges, need = [], []
    for _ in range(nbatches - 1):
        left, right, path = orc.get_next_merge(tree)
        need += [x for x in (left, right) if not isinstance(x, tuple)]
        ls, rs = side(left), side(right)
        merges.append({"left": ls, "right": rs, "row0": ls["row0"], "n": ls["n"] + rs["n"]})
        tree = orc.update_tree(tree, path, tuple(ls["batches"] + rs["batches"]))
    assert tree == tuple(int(b) for b in code[code != 0])
    return code, merges, need


@pytest.mark.parametrize("name", list(TREES))
def test_merge_sequence_and_leaf_order_follow_the_oracle_walk(run_cases, name):
    nbatches, order = TREES[name]
    code, merges, need = oracle_walk(nbatches, order)
    got = run_cases([words("tree", nbatches, *code)])[0]
    assert got["merges"] == merges
    assert got["need"] == need
    assert sorted(got["need"]) == list(range(1, nbatches + 1))
    assert got["nodes"] == 2 * nbatches - 1 and got["root"] == got["nodes"] - 1
    for m in merges:  # (the two children of a merge are adjacent row ranges)
        assert m["right"]["row0"] == m["left"]["row0"] + m["left"]["n"]


def test_rejected_codes_keep_their_code_and_text(run_cases):
    got = run_cases([words("tree", b, *code) for b, code, _ in REJECTED])
    for g, (_, code, text) in zip(got, REJECTED):
        assert g == {"error": BMX_ERR_TREE, "text": text}, code


def chains(vector):
    """head: the first occurrence of a cell; next: the next position of the same cell."""
    seen, nxt, head = {}, [-1] * len(vector), []
    for i, v in enumerate(vector):
        head.append(0 if v in seen else 1)
        if v in seen:
            nxt[seen[v]] = i
        seen[v] = i
    return nxt, head


def test_restrict_chains(run_cases):
    got = run_cases([words("restrict", n, *vec) for n, vec in RESTRICTS])
    for g, (n, vec) in zip(got, RESTRICTS):
        if min(vec) < 1 or max(vec) > n:
            assert g == {"error": BMX_ERR_SUBSET, "text": "subset indices out of range"}
            continue
        nxt, head = chains(vec)
        assert g == {"rows": [v - 1 for v in vec], "next": nxt, "head": head, "dups": len(set(vec)) < len(vec)}
    assert [("error" in g) for g in got] == [False, False, False, False, True, True]
    assert [g.get("dups") for g in got[:4]] == [False, True, True, False]


def test_pick_best_merge_and_count_matrix_update(run_cases, monkeypatch):
    # the matrix part of update_remainders: the new node's counts are the caller's business, zeros here as in the header
    monkeypatch.setattr(orc, "_count_mnn_pairs", lambda node, rem, upto, *rest: np.zeros(upto, dtype=np.int64))
    got = run_cases([words("counts", len(st), *st.ravel()) for st in COUNTS])
    for g, st in zip(got, COUNTS):
        rem = list(range(len(st)))
        left, right, chosen = orc.pick_best_merge(rem, st)
        assert (g["left"], g["right"], g["count"]) == (left, right, st.max()) == (chosen[0], chosen[1], st[chosen])
        new_rem, new = orc.update_remainders(rem, st, chosen, "merged", 20, None, 1)
        if new is None:  # the merged node is all that is left: the oracle stops, the header hands back its lone zero
            assert new_rem == "merged" and g["keep"] == [] and g["next"] == [[0]]
            continue
        assert g["keep"] == new_rem[:-1] and new_rem[-1] == "merged"
        assert np.array_equal(np.array(g["next"], dtype=np.int64), new)
    assert (got[0]["left"], got[0]["right"]) == (2, 0)  # the first of the tied maxima in column-major order
    assert "keep" in got[1] and got[1]["keep"] == []
