// The merge order of a run, decided once on the host (R/MNN_tree.R:48-107,196-226): the post-order tree code decoded and
// validated, the sequence .get_next_merge walks, the order in which the leaves are first needed, a restrict vector as
// 0-based rows with the chains of its repeated cells, and the bookkeeping of auto-merge's count matrix.  No HIP call and no
// device buffer: the engine (engine.hip) and mnnCorrect (mnn_correct.hip) both plan with it, and
// tests/host/merge_plan_host.cpp pins it on the CPU.
#pragma once
#include <cstdint>
#include <vector>

#include "host_basics.hpp"

namespace bmx {

struct PlanNode {
    int left = -1, right = -1;  // children (indices into MergePlan::nodes), -1 for a leaf
    int batch = -1;             // a leaf: its batch (0-based)
    int64_t row0 = 0, n = 0;    // the node's rows: the leaves' rows follow each other left to right in the tree
};

struct MergePlan {
    std::vector<PlanNode> nodes;  // in the order of the post-order code; the last one is the root
    std::vector<int> merges;      // B - 1 nodes in the order .get_next_merge reaches them: left = child 1, right = child 2
    std::vector<int> need_order;  // the batches (0-based) in the order those merges first ask for them
};

// tree[0, len): leaf = 1-based batch id, 0 = merge of the two top stack entries (R/MNN_tree.R:96-105 for the leaf checks).
// The first offending entry decides the error.
inline MergePlan plan_merges(const int32_t* tree, int len, int B, const int32_t* nrows) {
    MergePlan P;
    std::vector<int> stack;
    std::vector<char> seen((size_t)B + 1, 0);
    int64_t rows = 0;
    int leaves = 0;
    for (int i = 0; i < len; ++i) {
        const int v = tree[i];
        PlanNode s;
        if (v == 0) {
            if (stack.size() < 2) throw Error(BMX_ERR_TREE, "merge tree structure should contain two children per node");
            s.right = stack.back();
            stack.pop_back();
            s.left = stack.back();
            stack.pop_back();
            s.row0 = P.nodes[s.left].row0;
            s.n = P.nodes[s.left].n + P.nodes[s.right].n;
        } else {
            if (v < 1 || v > B || seen[v]) throw Error(BMX_ERR_TREE, "invalid leaf nodes specified in 'merge.order'");
            seen[v] = 1;
            ++leaves;
            s.batch = v - 1;
            s.row0 = rows;
            s.n = nrows[v - 1];
            rows += s.n;
        }
        P.nodes.push_back(s);
        stack.push_back((int)P.nodes.size() - 1);
    }
    if (stack.size() != 1 || leaves != B) throw Error(BMX_ERR_TREE, "invalid leaf nodes specified in 'merge.order'");
    // .get_next_merge (R/MNN_tree.R:61-69): both children finished -> merge; else descend into child 2 if it is still a
    // list, otherwise into child 1
    std::vector<char> done(P.nodes.size(), 0);
    for (size_t i = 0; i < P.nodes.size(); ++i) done[i] = P.nodes[i].batch >= 0;
    for (int mdx = 0; mdx < B - 1; ++mdx) {
        int cur = stack.back();
        while (!(done[P.nodes[cur].left] && done[P.nodes[cur].right]))
            cur = !done[P.nodes[cur].right] ? P.nodes[cur].right : P.nodes[cur].left;
        for (int child : {P.nodes[cur].left, P.nodes[cur].right})
            if (P.nodes[child].batch >= 0) P.need_order.push_back(P.nodes[child].batch);
        P.merges.push_back(cur);
        done[cur] = 1;  // .update_tree (R/MNN_tree.R:71-77)
    }
    return P;
}

// A restrict vector in the caller's order (any R subsetting vector: any order, a cell may be named more than once).  The
// positions of the same cell are chained: next[i] = the next position of the cell at position i (-1: none), head[i] = 1 at
// its first position.
struct RestrictChains {
    std::vector<int32_t> rows;   // [m] 0-based
    std::vector<int32_t> chain;  // [2 m]: next, then head
    bool dups = false;           // some cell repeats
    const int32_t* next() const { return chain.data(); }
    const int32_t* head() const { return chain.data() + rows.size(); }
};

// idx[0, m): rows of a batch or node of n cells, counted from `base` (1: the caller's vector, 0: a node's rows)
inline RestrictChains restrict_chains(const int32_t* idx, int m, int n, int base) {
    RestrictChains c;
    c.rows.resize((size_t)m);
    c.chain.assign((size_t)2 * m, -1);
    std::vector<int32_t> last((size_t)n, -1);
    for (int i = 0; i < m; ++i) {
        const int64_t v = (int64_t)idx[i] - base;
        if (v < 0 || v >= n) throw Error(BMX_ERR_SUBSET, "subset indices out of range");
        c.rows[i] = (int32_t)v;
        c.chain[(size_t)m + i] = last[v] < 0 ? 1 : 0;  // head
        if (last[v] >= 0) {
            c.chain[last[v]] = i;  // next
            c.dups = true;
        }
        last[v] = i;
    }
    return c;
}

// Auto-merge (R/MNN_tree.R:196-226): stats[i][j] = MNN pairs between remainders i (as left) and j (as right)
using CountMatrix = std::vector<std::vector<int64_t>>;

struct BestMerge {
    int left = 0, right = 0;
    int64_t count = -1;
};

// .pick_best_merge: first maximum in column-major order; left = row, right = column
inline BestMerge pick_best_merge(const CountMatrix& stats) {
    BestMerge b;
    const int R = (int)stats.size();
    for (int j = 0; j < R; ++j)
        for (int i = 0; i < R; ++i)
            if (stats[i][j] > b.count) b = BestMerge{i, j, stats[i][j]};
    return b;
}

// .update_remainders, the matrix part: drop the two chosen, keep the rest in order (their old indices to `keep`), append a
// row for the new node (zeros, for the caller's recount) with a zero column
inline CountMatrix drop_merged(const CountMatrix& stats, int left, int right, std::vector<int>& keep) {
    keep.clear();
    for (int i = 0; i < (int)stats.size(); ++i)
        if (i != left && i != right) keep.push_back(i);
    const int K = (int)keep.size();
    CountMatrix ns((size_t)K + 1, std::vector<int64_t>((size_t)K + 1, 0));
    for (int a = 0; a < K; ++a)
        for (int c = 0; c < K; ++c) ns[a][c] = stats[keep[a]][keep[c]];
    return ns;
}

}  // namespace bmx
