// What host code needs that needs no HIP header: the library's error, the testing knobs and the two integer helpers.
// bmx_common.hpp includes it for every unit of the library; knn_plan.hpp and merge_plan.hpp include it alone, so that the
// plan of a candidate pass and of a run's merges compile with a plain C++ compiler (tests/host/knn_plan_host.cpp,
// tests/host/merge_plan_host.cpp).
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>

#include "../../include/batchelor_mi355x.h"

namespace bmx {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

// Testing hooks (bmx_dev_set in the C ABI): process-wide knobs that tests and developer scripts set by an explicit call.
// Nothing in the ENVIRONMENT of the host process changes what the library computes or which tier / form runs
// (BMX_DEBUG=1 only prints, BMX_HOST_THREADS only sizes the staging thread pool).
struct DevKnobs {
    int knn_tier = 0;         // 1 / 2: that candidate tier only, 3: exact FP64 scan only
    int sample = -1;          // rows of the threshold sample of a candidate pass (-1: automatic)
    int split_c = 0;          // reference ranges of the tail query blocks (0: automatic)
    int force_c = 0;          // reference ranges of EVERY query block (0: off)
    int no_margin = 0;        // fp16 tier: lists cut at their KS-th best only (round 2's rule)
    int asv_fast = 0;         // adjust_shift_variance: the tiled form whatever the size
    int asv_cap = -1;         // tiled form: kept addends per chain of the literal re-run (-1: default, 0: no re-run)
    int asv_modes = 0;        // tiled form: record which way each of the first n cells of a call went (bmx_dev_get_bytes)
    int asv_sync = 0;         // tiled form: 1 = the workgroups start each round of tiles together (measured slower twice: rounds 4 and 6)
    int tau_replay = 0;       // developer experiment: 1 record every search's final thresholds, 2 start the full passes from them
    int lk_seed = 1;          // k beyond the tiers' lists: partitions after the first searched within the first's kp-th distance (0: plainly)
    int sample_split = -1;    // ranges of the threshold sample of a search with few query blocks (-1: automatic, 0: never, n: that many)
    int exchange_always = 0;  // a single rank goes through its exchange transport too (an all-gather of one)
    int refine_wave = 0;      // the exact re-rank takes a whole wave for every query (no half-wave form)
    int asv_wide = 0;         // adjust_shift_variance: the literal wide form (asv_wide_pairs + asv_wide_cells) whatever the size
    int asv_chunk = 0;        // wide form: at most this many cells a chunk (0: as many as 1 GiB of scratch holds); the strict pass's chunks likewise
    int asv_strict = -1;      // adjust_shift_variance: 1 = every call is strict (var_adj_strict), -1: as the call says
    int mfma_shape = -1;      // fp16 tier: MFMA shape of the sweep, 0 = 32x32x16, 1 = 16x16x32 where it exists (-1: the table's)
    int ref_order = -1;       // fp16 tier: reference image in key order (knn_order.hpp): -1 the default rule (knn.hip), 0 never, 1 wherever it is possible
    int snn_lds_candidates = 0; // SNN graph: candidates of a cell one LDS window holds (0: default 2048; at least k + 1, at most 4096)
};

inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

}  // namespace bmx
