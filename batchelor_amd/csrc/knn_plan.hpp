// The shape of one candidate pass of the kNN (knn.hip: candidate_pass), as a pure function of the sizes and the testing
// knobs: sample size and its split, number and length of the reference ranges, how many query blocks sweep the reference as
// one range.  No HIP call and no device buffer: tests/host/knn_plan_host.cpp pins it on the CPU.  A wrong plan changes no
// result, only the time -- which is why it is pinned.
#pragma once
#include <algorithm>
#include <cmath>

#include "host_basics.hpp"

namespace bmx {

constexpr int MAX_CHUNKS = 8;  // reference ranges a query's lists can hold: a pass plans at most MAX_CHUNKS - 1

#ifndef BMX_SEEDED_SAMPLE
#define BMX_SEEDED_SAMPLE 4096
#endif

#ifndef BMX_ORDERED_SAMPLE
#define BMX_ORDERED_SAMPLE 8192
#endif

struct PassPlan {
    int unit;              // queries per workgroup
    int nq_pad, nqb;       // queries padded to whole workgroups; query blocks
    int S, CS;             // rows of the threshold sample (0: none); ranges asked of it
    int sample_range_len, sample_nranges;  // ... and what the sample pass is launched with
    int C, chunk_len;      // reference ranges of the split query blocks, rows of one
    int nr_pad;            // C * chunk_len
    int n_full;            // with C > 1: the first n_full query blocks still sweep the reference as ONE range
};

// tier_id: 1 = fp16 single product, 2 = split bf16.  rows_per_slot: what a range is a multiple of (the fp16 ring hands two
// or four tiles over at a time: f16_rows_per_slot; 32 for the bf16 tier).
// ordered: the reference image is in key order (knn_order.hpp) -- the sample then consists of the rows nearest the queries'
// centre, and fewer of them do (BMX_ORDERED_SAMPLE: MEASUREMENTS.md has the series per size).
inline PassPlan plan_candidate_pass(int tier_id, int NS, int KS, int unit, int rows_per_slot, int nq, int nr, bool seeded,
                                    const DevKnobs& knobs, bool ordered = false) {
    PassPlan P{};
    P.unit = unit;
    P.nq_pad = (int)round_up(nq, unit);
    P.nqb = P.nq_pad / unit;
    const int nqb = P.nqb;

    // Reference ranges.  A short sample range [0, S) runs first and hands every query a valid starting threshold, so
    // selection is tight from the first tile of the full pass.  One workgroup per CU: the query blocks that fill whole
    // rounds of 256 workgroups sweep the reference as ONE range (tightest thresholds, one list per query); only the
    // remaining b blocks are split into c ranges, chosen so that their b * c short items fill the last round evenly.
    // Measured work per pair evaluation relative to one range (100k x 400k): 3 ranges 1.12, 5: 1.17, 7: 1.21.
    // Sample size: each sampled row costs every query a filter-only tile visit, each row NOT sampled costs KS / row
    // more candidates to append and select (the harmonic tail of the running threshold) -- with the fp16 kernel's
    // cheap tiles the balance is flat between 16k and 32k rows at 50 PCs and lower for longer rows (a sampled tile
    // costs the full matrix work).  The fp16 kernel samples small references too (a quarter of the rows): its sweep
    // hands every survivor to another wave, which makes a start without thresholds expensive
    const bool no_margin_knob = knobs.no_margin != 0;
    int S_auto = nr >= 32768 ? 4096 : 0;
    if (tier_id == 1 && nr >= 4096) S_auto = std::max(1024, std::min(nr / 4, NS <= 4 ? 24576 : 12288));
    if (ordered && tier_id == 1 && nr >= 4096) S_auto = std::min(S_auto, BMX_ORDERED_SAMPLE);
    // (a seeded search samples too, but a sixth of the rows: the odd query whose seed is loose -- a left cell listed by
    // one far-away right cell -- then starts from a sampled threshold instead of none; the tighter of the two counts)
    if (seeded && tier_id == 1) S_auto = std::min(S_auto, BMX_SEEDED_SAMPLE);
    int S = (int)round_up(knobs.sample >= 0 ? knobs.sample : S_auto, tier_id == 1 ? rows_per_slot : 64);
    // A search with few query blocks (a rank's slice of a multi-GPU run: 12 500 queries = 49 blocks for 256 CUs) would sweep
    // the sample with a fifth of the chip, every block over all of it: the sample is split into CS ranges instead, block x
    // range items fill the CUs, each range of at least 24 ring slots (a lane keeps the KS / 2 <= 24 smallest of its per-slot
    // minima) hands its queries a threshold of its own and the tightest one counts (atomicMin on the shared word).
    // Round 6: the ranges leave their lists and the k-th smallest of the union is taken (f16_sample_merge): the threshold of the
    // unsplit sample, so the split is on by default (testing hook "sample_split": 0 never, n that many ranges).
    int CS = 1;
    if (tier_id == 1 && S > 0 && nqb < 128 && knobs.sample_split != 0 && !no_margin_knob) {
        const int rs = rows_per_slot;
        CS = std::max(1, std::min({256 / std::max(nqb, 1), 8, S / (8 * rs)}));
        if (knobs.sample_split > 0) CS = std::max(1, std::min({knobs.sample_split, S / rs, 512 / KS}));
    }
    int C = 1, n_full = 0;
    {
        const int a = nqb / 256, b = nqb % 256;
        n_full = a * 256;
        if (b > 0) {
            double best = 1e30;
            for (int c = 1; c <= MAX_CHUNKS - 1; ++c) {
                if (c > 1 && nr / c < 2048) break;
                const double tailc = std::ceil((double)b * c / 256.0) / c * (1.0 + 0.105 * std::log((double)c));
                if (tailc < best - 1e-9) {
                    best = tailc;
                    C = c;
                }
            }
        }
    }
    if (knobs.split_c > 0) C = std::max(1, knobs.split_c);
    if (knobs.force_c > 0) {
        C = std::max(1, std::min(MAX_CHUNKS - 1, knobs.force_c));
        n_full = 0;
    }
    const int rmul = rows_per_slot;
    const int chunk_len = (int)round_up(cdiv(nr, C), rmul);
    C = std::max(1, cdiv(nr, chunk_len));
    const int nr_pad = chunk_len * C;
    S = std::min(S, nr_pad / rmul * rmul);  // (a forced sample size beyond the reference: the prepared image ends at nr_pad)
    P.S = S;
    P.CS = CS;
    // the sample pass: one range, or block x range items over the sample rows [0, S)
    P.sample_range_len = S;
    P.sample_nranges = 1;
    if (S > 0 && CS > 1) {
        P.sample_range_len = (int)round_up(cdiv(S, CS), rows_per_slot);
        P.sample_nranges = cdiv(S, P.sample_range_len);
    }
    P.C = C;
    P.chunk_len = chunk_len;
    P.nr_pad = nr_pad;
    P.n_full = n_full;
    return P;
}

// The queries whose re-rank takes half a wave (knn_refine_half): those of the whole-range blocks, which hold one list of at
// most 32 candidates each; the others take a wave (knn_refine).
inline int refine_half_queries(const PassPlan& P, int KS, int nq, const DevKnobs& knobs) {
    if (KS != 32 || knobs.refine_wave) return 0;
    return P.C > 1 ? std::min(nq, P.n_full * P.unit) : nq;
}

}  // namespace bmx
