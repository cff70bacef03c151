// What the units of the merge engine share (engine.hip: lifetime, upload, searches, the run; engine_exchange.hip: ranks and
// their exchange; engine_merge.hip: one merge; engine_results.hip: what a finished run hands out).
#pragma once
#include <algorithm>
#include <cmath>

#include "engine.hpp"

namespace bmx {

// .choose_k (R/MNN_tree.R:140-146); R's round() is half-to-even = nearbyint in the default rounding mode
inline int choose_k(int k, double prop_k, int N) {
    if (std::isnan(prop_k)) return k;
    const double r = std::nearbyint(prop_k * (double)N);
    const double m = std::max((double)k, r);
    return (int)std::min((double)N, m);
}

// a then b: a merged node's index / origin / stat_slot / extras, a merge's slots of both sides
template <class T>
std::vector<T> concat(const std::vector<T>& a, const std::vector<T>& b) {
    std::vector<T> out = a;
    out.insert(out.end(), b.begin(), b.end());
    return out;
}

// What the phases of one merge hand each other (Engine::merge_step)
struct Engine::MergeCtx {
    int mdx;
    Node& left;
    Node& right;
    const bmx_params_t& p;
    MergeRecord& rec;
    // .restricted_mnn (R/MNN_tree.R:113-133) works on the restricted rows only
    int nLs, nRs;
    const int32_t *lrows, *rrows;  // null: all rows
    const int32_t* rnext;          // the right side's chains of repeated cells, null without
    double *mu_l = nullptr, *mu_r = nullptr;  // the restrict-row column means of both sides
    MnnOut mo;
    int vid = 0;                 // slot of this merge's overall.batch in the pool
    double* averaged = nullptr;  // [mo.U][d] the averaged correction vectors
    std::unique_ptr<Section> sec;  // the streaming section that is open

    MergeCtx(int m, Node& l, Node& r, const bmx_params_t& prm, MergeRecord& rc)
        : mdx(m), left(l), right(r), p(prm), rec(rc), nLs(l.has_restrict ? l.n_restrict : l.n),
          nRs(r.has_restrict ? r.n_restrict : r.n), lrows(l.has_restrict ? l.restrict_rows.p : nullptr),
          rrows(r.has_restrict ? r.restrict_rows.p : nullptr), rnext(r.restrict_dups ? r.dup_next.p : nullptr) {}
};

}  // namespace bmx
