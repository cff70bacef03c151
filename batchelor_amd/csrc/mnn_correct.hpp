// mnnCorrect() on the device (mnn_correct.hip): the arguments of the one-shot call and what it returns, host side.
#pragma once
#include <cstdint>
#include <vector>

namespace bmx {

struct MnnCorrectArgs {
    int B = 0, G = 0;                         // batches, genes of every batch
    const double* const* data = nullptr;      // per batch: G x ncells[b] column-major (R's layout)
    const int32_t* ncells = nullptr;
    // the batches as CSC (bmx_mnn_correct_sparse): indptr is set, `data` holds every batch's stored values
    const int64_t* const* indptr = nullptr;   // per batch: [ncells[b] + 1], from 0 to the batch's number of stored entries
    const int32_t* const* indices = nullptr;  // per batch: 0-based rows, ascending within a column; null without an entry
    bool sparse() const { return indptr != nullptr; }
    const int32_t* const* restrict_idx = nullptr;  // per batch: 1-based cells, or null (nullable as a whole)
    const int32_t* n_restrict = nullptr;           // per batch: their number, < 0: none
    int k = 20;
    double prop_k = 0.0;                      // NaN: NULL
    double sigma = 0.1;
    int cos_in = 1, cos_out = 1, var_adj = 1, correct_all = 0, svd_dim = 0, auto_merge = 0;
    int var_adj_strict = 0;                   // with var_adj: adjust_shift_variance in strict mode (bmx_ops.hpp)
    const int32_t* subset = nullptr;          // 1-based genes (subset.row), or null
    int nsubset = 0;
    const int32_t* tree = nullptr;            // post-order code: leaf = batch id, 0 = merge
    int tree_len = 0;
};

struct MnnCorrectResult {
    int Gout = 0;
    std::vector<double> corrected;            // [N][Gout] (= Gout x N column-major), cells in input order
    std::vector<int32_t> batch;               // 1-based, per cell
    std::vector<std::vector<int>> left, right;  // batch ids of every merge
    std::vector<std::vector<int32_t>> pairs_left, pairs_right;  // per merge, 1-based rows of the output
    std::vector<int64_t> strict_cells;        // [merges][2]: cells the strict pass recomputed in the merge's call on the input genes / on the output genes (-1: none ran)
    double stage_ms[5] = {0, 0, 0, 0, 0};     // HIP-event time over all merges: search + pairs, averaging, smoothing, asv, apply
};

// argument checks of mnn_correct_run, without a device (throws bmx::Error with the reference's messages)
void mnn_correct_check(const MnnCorrectArgs& a);
void mnn_correct_run(const MnnCorrectArgs& a, MnnCorrectResult& res);

}  // namespace bmx
