// What the units of the exact kNN call of one another.  Included by knn.hip, knn_refine.hip, knn_exact.hip, knn_large_k.hip
// and the two candidate tiers (knn_f16.hip, knn_bf16.hip, knn_prep.hip) only: the rest of the library sees knn_device (bmx_common.hpp).
//   knn.hip          candidate_tiers, candidate_pass, search_tiers (the tier cascade), knn_device, read_count
//   knn_plan.hpp     the shape of a candidate pass, host only
//   knn_f16.hip      tier 1: knn_topk_f16 (producer and service roles as functions, the consumer sweep in its body), launcher
//   knn_f16_shape.hpp  ... the shape of its workgroup and its LDS layout (host + device, no HIP header), its tunables
//   knn_bf16.hip     tier 2: knn_topk_bf16 (producer role and final lists as functions, the consumer sweep in its body), launcher
//   knn_bf16_shape.hpp ... the shape of its workgroup and its LDS layout (host + device, no HIP header), its tunables
//   knn_prep.hip     the prep kernels of both tiers: the steps of a tile once, a number format per tier
//   knn_order.hip    tier 1, ordered references: the image's two index arrays from the rows' keys (knn_order.hpp: the pure part)
//   knn_tier.hpp     what the two tiers share on the device: work-item decode, LDS word loads, stamps
//   knn_refine.hip   the FP64 re-rank and certificate behind either tier
//   knn_exact.hip    the bounded FP64 sweep, the full FP64 scan, exact_search
//   knn_large_k.hip  k beyond the tiers' lists: partitions, their merges
#pragma once
#include "bmx_common.hpp"
#include "knn_plan.hpp"
#include "knn_select.hpp"

namespace bmx {

// ---- the candidate tiers ---------------------------------------------------------------------------------------------
// one launch of either tier's top-k kernel
struct PassLaunch {
    const uint16_t* pq;
    const uint16_t* pr;
    int nqb, first_begin, range_len, nranges, r_limit, out_chunk0, out_nchunks;
    uint32_t* tau_g;        // per-query threshold shared by all ranges (orderable image); sample pass writes it
    int sample;             // non-zero: threshold-estimation pass, writes tau_g[q] only
    int32_t* cand;
    float* cand_v;          // approximate values of the candidates
    float* tau;
    int n_full = 0;         // the first n_full query blocks sweep [first_begin, r_limit) as ONE range; the others split it
    // fp16 tier: with margin[q] = twice the pass's error bound for query q (its own units) a list is cut at
    // (k-th best value + margin) instead of at its KS-th best -- what lies beyond cannot be among the k nearest
    const float* margin = nullptr;
    int k = 0;
    const uint32_t* tau_seed = nullptr;  // fp16 tier, sample pass of a seeded search: tau_g = min(sampled, tau_seed)
    int shape = 0;          // fp16 tier: MFMA shape of the sweep (f16_pick_shape), the one pr was prepared for
};
// split-bf16 candidate pass (knn_bf16.hip; bf16_prep: knn_prep.hip)
int bf16_pick_ns(int d);         // MFMA k-steps (16 bf16 each) for 3 d + 3 columns; 0 = unsupported
int bf16_ncons(int NS, int KS);  // consumer waves (32 queries each) per workgroup
void bf16_prep(hipStream_t stream, const double* X, const int32_t* rows, int n, int n_pad, int d, int NS,
               const double* mean, int is_query, uint16_t* P, double* n2, unsigned long long* maxbits,
               unsigned long long* slots);  // slots: 64 x 16 words of scratch for the reference-norm maximum
bool bf16_launch(hipStream_t stream, KnnWorkspace& ws, int NS, int KS, const PassLaunch& L);
// fp16 candidate pass (knn_f16.hip; f16_prep_all: knn_prep.hip)
int f16_pick_ns(int d, int KS);
int f16_rows_per_slot(int NS, int KS);  // reference rows a ring slot of the fp16 tier holds (ranges are multiples of it)
int f16_pick_shape(int NS, int KS);     // MFMA shape of the sweep: 0 = 32x32x16, 1 = 16x16x32 (table, or the "mfma_shape" hook)
// ordered references of one search (knn_order.hpp): what goes in, the scratch, the two index arrays that come out
struct RefOrder {
    const double* qcentre;  // [d] a point near the middle of the queries
    float* key;             // [nr] |r - qcentre|^2 per reference position (knn_prep_f16_norms)
    uint32_t* scratch;      // [ref_order_scratch_words(nr)]
    int32_t* img_src;       // [nr] row of X behind image row i
    int32_t* img_pos;       // [nr] reference position behind image row i
};
size_t ref_order_scratch_words(int nr);
// img_src / img_pos from the keys and their range (second word of the prep kernels' slots): knn_order.hip
void ref_order_build(hipStream_t stream, const float* key, int nr, const int32_t* ref_rows, const unsigned long long* slots,
                     uint32_t* scratch, int32_t* img_src, int32_t* img_pos);
void f16_prep_all(hipStream_t stream, const double* X, const int32_t* rrows, int nr, int nr_pad, const double* Q,
                  const int32_t* qrows, int nq, int nq_pad, int d, int NS, int shape, const double* mean, uint16_t* Pr, uint16_t* Pq,
                  double* rn2, double* qn2, unsigned long long* maxbits, unsigned long long* slots, int32_t* flagged0,
                  float* margin, const sel::PassEps& pe, const float* seed_d2, uint32_t* tau_seed, uint32_t* tau_init,
                  const RefOrder* ord = nullptr);
bool f16_launch(hipStream_t stream, KnnWorkspace& ws, int NS, int KS, const PassLaunch& L);
void f16_sample_merge(hipStream_t stream, const float* lists, int nranges, int KS, int nq, int k, const float* margin,
                      uint32_t* tau_g);

// ---- knn.hip -----------------------------------------------------------------------------------------------------------
struct Tier {
    int id;  // 1 = fp16 single product, 2 = split bf16
    int NS, KS;
};
// the candidate tiers that take this shape, cheapest first
int candidate_tiers(int d, int k, int nr, Tier out[2]);
// queries (Qs, qrs)[0, nq) through the tiers tiers[t ...], then the exact paths
void search_tiers(hipStream_t stream, KnnWorkspace& ws, const Tier* tiers, int ntiers, int t, const double* X,
                  const int32_t* ref_rows, int nr, const double* Qs, const int32_t* qrs, int nq, int d, int k, int32_t* io,
                  double* dout, const float* seed_d2 = nullptr, const double* centre = nullptr, double* kth_out = nullptr,
                  const double* qcentre = nullptr);
// one device word to the host (a count that decides what is launched next)
int read_count(hipStream_t stream, KnnWorkspace& ws, const int32_t* dev);

// ---- knn_refine.hip ------------------------------------------------------------------------------------------------------
// what a candidate pass left on the device for its re-rank
struct PassLists {
    const int32_t* cand;   // [nq_pad][C * KS] candidate positions (image rows), -1 = empty
    const float* cand_v;   // their approximate values
    const float* tau;      // [nq_pad][C] final thresholds
    const double* qn2;     // squared norms of the centred queries
    const unsigned long long* maxbits;  // largest squared norm of the centred references (bit pattern)
    const int32_t* img_pos = nullptr;   // ordered references: cand holds image rows, img_pos[row] is the position (null: cand holds positions)
};
// FP64 re-rank and certificate of the queries (Qs, qrs)[0, nq): certified rows of io / dout are final; the others are listed
// in `flagged` with their k-th candidate distance in flag_bound.  zero_slots (nullable): left zeroed for the next search.
void refine_launch(hipStream_t stream, KnnWorkspace& ws, const PassPlan& plan, int KS, const sel::PassEps& pe,
                   const PassLists& lists, const double* X, const int32_t* ref_rows, const double* Qs, const int32_t* qrs,
                   int nq, int d, int k, const float* seed_d2, int32_t* io, double* dout, int32_t* flagged,
                   double* flag_bound, unsigned long long* zero_slots, double* kth_out);

// ---- knn_exact.hip -------------------------------------------------------------------------------------------------------
// The bounded FP64 sweep over the queries list[1 + f] with bounds[f] (knn_exact_filter + knn_exact_pick).
//   dev_cap == 0: `count` queries, known to the host; returns the list of those whose kept references overflowed (count in
//                 its word 0, on the device), for the full scan;
//   dev_cap  > 0: the count is list[0] on the device, at most dev_cap are taken; what cannot be handled raises opt[0].
int32_t* launch_bounded_sweep(hipStream_t stream, KnnWorkspace& ws, const double* X, const int32_t* ref_rows, int nr,
                              const double* Qs, const int32_t* qrs, int d, int k, int32_t* io, double* dout,
                              const int32_t* list, const double* bounds, int count, int dev_cap, bool seeded, int32_t* opt);
// The full FP64 scan of queries list[1 + f0 ..] (nullptr: queries f0 ..): knn_exact_dist into drow, then the selection that
// suits k.  dev_cap == 0: nb queries; dev_cap > 0: list[0] on the device, at most dev_cap.  drow: [max(nb, dev_cap)][nr].
void launch_full_scan(hipStream_t stream, KnnWorkspace& ws, const double* X, const int32_t* ref_rows, int nr,
                      const double* Qs, const int32_t* qrs, int d, int k, int32_t* io, double* dout, const int32_t* list,
                      int f0, int nb, int dev_cap, double* drow);
// Exact FP64 search: `count` queries listed in scan-list form (list[1 + f], nullptr = queries 0 .. count-1).  With
// bounds (the k-th candidate distance of each listed query) a bounded filter pass runs first; what overflows it, or
// everything when there are no bounds, takes the full scan.
void exact_search(hipStream_t stream, KnnWorkspace& ws, const double* X, const int32_t* ref_rows, int nr, const double* Qs,
                  const int32_t* qrs, int d, int k, int32_t* io, double* dout, const int32_t* list, const double* bounds,
                  int count, bool seeded = false);

// ---- knn_large_k.hip -----------------------------------------------------------------------------------------------------
// false: the shape does not suit the partitioned search (too few reference cells a partition, too many candidates)
bool large_k_search(hipStream_t stream, KnnWorkspace& ws, const double* X, const int32_t* ref_rows, int nr, const double* Qs,
                    const int32_t* qrs, int nq, int d, int k, int32_t* io, double* dout, const double* centre,
                    double* kth_out);

}  // namespace bmx
