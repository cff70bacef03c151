"""The shared-nearest-neighbour graph by the reverse ("host") lists, in plain Python: the reference the SNN tests share
(tests/test_cpu_snn_graph.py holds it against a brute-force set intersection over all pairs).

index [n x k], 1-based: each row's k nearest OTHER rows.  L(c) = (c, index[c, 0], ..., index[c, k - 1]) at ranks 0..k.  Cells
a > b share an edge exactly when L(a) and L(b) meet; rank_sum = the smallest rank_a(s) + rank_b(s) over the shared cells s,
count = their number."""
import numpy as np

SNN_TYPES = ("rank", "number", "jaccard")


def snn_graph_ref(index):
    """(first, second, rank_sum, count): 1-based int32 ends with first > second, ascending first then second; int64 rank sums
    and counts."""
    index = np.asarray(index)
    n, k = index.shape
    members = np.concatenate([np.arange(n)[:, None], index.astype(np.int64) - 1], axis=1)  # L(c), 0-based, rank = column
    hosts = [[] for _ in range(n)]            # for each cell the (host, rank) of the lists that hold it
    for c in range(n):
        for r in range(k + 1):
            hosts[members[c, r]].append((c, r))
    first, second, rank_sum, count = [], [], [], []
    for j in range(n):
        best = {}
        for t in range(k + 1):
            for h, r in hosts[members[j, t]]:
                if h < j:
                    got = best.get(h)
                    best[h] = (t + r, 1) if got is None else (min(got[0], t + r), got[1] + 1)
        for h in sorted(best):
            first.append(j + 1)
            second.append(h + 1)
            rank_sum.append(best[h][0])
            count.append(best[h][1])
    return (np.array(first, dtype=np.int32), np.array(second, dtype=np.int32), np.array(rank_sum, dtype=np.int64),
            np.array(count, dtype=np.int64))


def snn_weights(k, rank_sum, count, type):
    """The three weightings, float64: exact for "rank" and "number", one IEEE division for "jaccard"."""
    if type == "rank":
        return np.maximum(float(k) - 0.5 * rank_sum.astype(np.float64), 1e-6)
    if type == "number":
        return np.maximum(count.astype(np.float64), 1e-6)
    if type == "jaccard":
        return count.astype(np.float64) / (2.0 * (k + 1) - count.astype(np.float64))
    raise ValueError(type)


def snn_brute_force(index):
    """The definition itself: every pair a > b, the two lists intersected as sets."""
    index = np.asarray(index)
    n, k = index.shape
    lists = [[c] + [int(v) - 1 for v in index[c]] for c in range(n)]
    ranks = [{s: r for r, s in enumerate(L)} for L in lists]
    first, second, rank_sum, count = [], [], [], []
    for a in range(n):
        for b in range(a):
            shared = ranks[a].keys() & ranks[b].keys()
            if shared:
                first.append(a + 1)
                second.append(b + 1)
                rank_sum.append(min(ranks[a][s] + ranks[b][s] for s in shared))
                count.append(len(shared))
    return (np.array(first, dtype=np.int32), np.array(second, dtype=np.int32), np.array(rank_sum, dtype=np.int64),
            np.array(count, dtype=np.int64))


# ---- crafted indices (1-based) the CPU and GPU tests share ----
def hub_index(n, k):
    """Every row lists rows 1..k; rows 1..k + 1 take k of the first k + 1 rows without themselves: in-degrees of about n."""
    idx = np.tile(np.arange(1, k + 1), (n, 1))
    for c in range(k + 1):
        idx[c] = [v for v in range(1, k + 2) if v != c + 1][:k]
    return idx.astype(np.int32)


def chain_index(n, k):
    """Row i lists i + 1, ..., i + k, wrapped at the end."""
    return ((np.arange(n)[:, None] + np.arange(1, k + 1)[None, :]) % n + 1).astype(np.int32)


def complete_index(n):
    """n = k + 1: every row lists every other row, ascending."""
    return np.array([[v for v in range(1, n + 1) if v != c + 1] for c in range(n)], dtype=np.int32)
