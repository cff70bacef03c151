// The exact kNN (knn.hip) for k beyond what the candidate tiers' lists hold: the partitioned search (large_k_search) and
// the three merges of the partitions' lists (lk_merge_wave, lk_merge, lk_merge_big).
#include "knn_fp64.hpp"
#include "knn_internal.hpp"

#include <algorithm>
#include <type_traits>

namespace bmx {
namespace {

// ---------------------------------------------------------------------------------------------------
// k beyond what the candidate tiers' lists hold (k > 36: `prop.k` of R/MNN_tree.R:140-146, or simply k = 50).
// The reference is dealt into P strided partitions (row j of the list goes to partition j mod P: independent of how the
// caller ordered its cells), every partition is searched for its 36 (or 20) nearest with the whole certified cascade above, and
// the P x 36 candidates of a query are merged exactly: squared distances recomputed in the reference's order of operations
// (sum over the dimensions of (q - x)^2, no contraction), sorted by (distance, position) -- the exact search's own order --, the first
// k are the answer PROVIDED no partition's list ends inside them: a partition whose 36th neighbour ranks behind the k-th
// merged candidate cannot hold anything nearer that it did not list.  With P = ceil(k / 16) a partition holds 16 of the k
// on average; a query for which one holds more than 35 fails the test and goes to the exact scan.
// Cost: the matrix work of ONE search at k = 36 (P searches over 1 / P of the reference each) + P preparations.
// ---------------------------------------------------------------------------------------------------
constexpr int LK_MAXE = 2048;  // candidates merged per query

// seed[q] = the first partition's kp-th distance squared, rounded up to f32 (+inf where that row was not certified): sqrt,
// then squared again -- never below the true value
__global__ void lk_seed_kernel(const double* __restrict__ kth, int nq, float* __restrict__ seed) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const double dd = kth[q] * kth[q] * (1.0 + 1e-15);
    float f = (float)dd;
    if ((double)f < dd) f = __uint_as_float(__float_as_uint(f) + 1u);  // dd >= 0: the next float up
    seed[q] = dd < __builtin_inf() ? f : __builtin_inff();
}

// rows[off_p + j] = the (p + j P)-th row of the caller's reference list, partition-major
__global__ void lk_partition_rows(const int32_t* __restrict__ ref_rows, int nr, int P, int32_t* __restrict__ rows) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nr) return;
    const int p = g % P, j = g / P;
    // partitions 0 .. (nr % P) - 1 hold one row more: offset of partition p = p * (nr / P) + min(p, nr % P)
    const int base = nr / P, rem = nr % P;
    rows[(int64_t)p * base + (p < rem ? p : rem) + j] = ref_rows ? ref_rows[g] : g;
}

// ---- what the three merges share --------------------------------------------------------------------------------------
// the partitions' lists of one query: sub_idx [P][nq][kp] positions inside the partitions (-1: an empty place), sub_d2
// (nullable) their squared distances as the partitions' searches left them
struct LkLists {
    const double* X;
    const int32_t* rows;  // partition-major (lk_partition_rows)
    int nr, P, kp;
    const double* qv;     // the query's row
    int q, nq, d;
    const int32_t* sub_idx;
    const double* sub_d2;
};
struct LkCand {
    double d2;  // squared distance in the reference's order of operations; +inf: no candidate
    int pos;    // position in the caller's reference list; 0x7fffffff: no candidate
};
// candidate e = p kp + j of the query: entry j of partition p's list (e >= P kp: none)
__device__ __forceinline__ LkCand lk_fetch(const LkLists& L, int e) {
    LkCand c{__builtin_inf(), 0x7fffffff};
    if (e >= L.P * L.kp) return c;
    const int p = e / L.kp, j = e - p * L.kp;
    const int64_t at = ((int64_t)p * L.nq + L.q) * L.kp + j;
    const int l = L.sub_idx[at];  // position inside partition p
    if (l < 0) return c;          // (no address is formed from an empty place)
    c.pos = l * L.P + p;
    if (L.sub_d2) {  // (the partition's search left the very sum below, squared: nothing to gather)
        c.d2 = L.sub_d2[at];
        return c;
    }
    const int base = L.nr / L.P, rem = L.nr % L.P;
    const double* x = L.X + (int64_t)L.rows[(int64_t)p * base + (p < rem ? p : rem) + l] * L.d;
    // (eight coordinates asked for at a time -- a random row: the round trips are what this costs --, summed in order: over
    // the columns left to right, one subtraction, one product, one addition each, no contraction)
    double s = 0.0;
    int col = 0;
    for (; col + 8 <= L.d; col += 8) {
        double xv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) xv[u] = x[col + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const double t = L.qv[col + u] - xv[u];
            s += t * t;
        }
    }
    for (; col < L.d; ++col) {
        const double t = L.qv[col] - x[col];
        s += t * t;
    }
    c.d2 = s;
    return c;
}

// A query whose merge is not certified: an optimistic run raises its flag (the engine repeats the run with host-checked
// searches); otherwise the query is listed for the exact scan.  One lane per query calls it.
__device__ __forceinline__ void report_uncertified(int q, int32_t* __restrict__ flagged, int32_t* __restrict__ opt) {
    if (opt) atomicOr(opt, 1);
    else flagged[1 + atomicAdd(&flagged[0], 1)] = q;
}

// kp: neighbours asked of every partition (sub_idx [P][nq][kp])
__global__ __launch_bounds__(256) void lk_merge(const double* __restrict__ X, const int32_t* __restrict__ rows, int nr, int P,
                                                int kp, const double* __restrict__ Q, const int32_t* __restrict__ qrs, int nq,
                                                int d, int k, const int32_t* __restrict__ sub_idx, int32_t* __restrict__ idx_out,
                                                double* __restrict__ dist_out, int32_t* __restrict__ flagged,
                                                int32_t* __restrict__ opt, double* __restrict__ kth_out,
                                                const float* __restrict__ seed_d2, const double* __restrict__ sub_d2) {
    __shared__ double kd[LK_MAXE];
    __shared__ int32_t ki[LK_MAXE];
    __shared__ int sh_fail;
    const int q = blockIdx.x, tid = threadIdx.x;
    const int E = P * kp;
    int np2 = 256;
    while (np2 < E) np2 <<= 1;
    const LkLists L{X, rows, nr, P, kp, Q + (int64_t)(qrs ? qrs[q] : q) * d, q, nq, d, sub_idx, sub_d2};
    for (int e = tid; e < np2; e += 256) {
        const LkCand c = lk_fetch(L, e);
        kd[e] = c.d2;
        ki[e] = c.pos;
    }
    if (tid == 0) sh_fail = 0;
    __syncthreads();
    block_bitonic_sort<256>(kd, ki, np2);
    for (int r = tid; r < k; r += 256) {
        idx_out[(int64_t)q * k + r] = ki[r];
        if (dist_out) dist_out[(int64_t)q * k + r] = sqrt(kd[r]);
    }
    // no partition's list may end inside the first k: its last entry is the kp-th of its partition -- found among the sorted
    // candidates by its position (unique) -- and must rank at k or later
    for (int r = tid; r < k; r += 256) {
        const int g = ki[r], p = g % P, l = g / P;
        if (sub_idx[((int64_t)p * nq + q) * kp + kp - 1] == l) sh_fail = 1;
    }
    // partitions searched within the seed distance (large_k_search) are complete up to it only: the k-th must lie inside
    if (tid == 0 && seed_d2 && !(kd[k - 1] < (double)seed_d2[q])) sh_fail = 1;
    __syncthreads();
    // (a row that fails is rewritten by an exact path -- unless an optimistic run has more of them than it takes on the device,
    // and then the kernels queued behind this search still read the row before the engine starts over: every entry a valid
    // position.  Seeded partitions can leave fewer than k candidates, i.e. empty places among the first k.)
    if (sh_fail)
        for (int r = tid; r < k; r += 256) idx_out[(int64_t)q * k + r] = 0;
    // (the intersection's probe skips a row whose k-th distance it knows to be too small: exact here when the merge stands)
    if (tid == 0 && kth_out) kth_out[q] = sh_fail ? __builtin_inf() : sqrt(kd[k - 1]);
    if (tid == 0 && sh_fail) report_uncertified(q, flagged, opt);
}

// The same merge for up to 512 candidates a query (k <= 224 with lists of 36), one WAVE per query and no sort: the partitions'
// lists arrive sorted by (squared distance, position) -- the order the merged list wants --, so a candidate's place in the
// merged list is the number of candidates in front of it: its place in its own list plus, for every other partition, a binary
// search.  (A 256-thread bitonic sort per query took 3 ms a search at config 2, a third of the whole.)
__global__ __launch_bounds__(256) void lk_merge_wave(const double* __restrict__ X, const int32_t* __restrict__ rows, int nr, int P,
                                                     int kp, const double* __restrict__ Q, const int32_t* __restrict__ qrs,
                                                     int nq, int d, int k, const int32_t* __restrict__ sub_idx,
                                                     int32_t* __restrict__ idx_out, double* __restrict__ dist_out,
                                                     int32_t* __restrict__ flagged, int32_t* __restrict__ opt,
                                                     double* __restrict__ kth_out, const float* __restrict__ seed_d2,
                                                     const double* __restrict__ sub_d2) {
    __shared__ double kd_[4][512];
    __shared__ int32_t ki_[4][512];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + w;
    if (q >= nq) return;  // (whole waves: nothing below synchronises the block)
    double* kd = kd_[w];
    int32_t* ki = ki_[w];
    const int E = P * kp;
    const LkLists L{X, rows, nr, P, kp, Q + (int64_t)(qrs ? qrs[q] : q) * d, q, nq, d, sub_idx, sub_d2};
    for (int e = lane; e < E; e += 64) {
        const LkCand c = lk_fetch(L, e);
        kd[e] = c.d2;
        ki[e] = c.pos;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    // (every entry of the row a valid position whatever the lists hold: lists spoilt by a search that an optimistic run has
    // already given up on must not leave an entry unwritten for the kernels queued behind it)
    for (int r = lane; r < k; r += 64) idx_out[(int64_t)q * k + r] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    bool fail = false;
    double kthv = -1.0;  // the k-th merged candidate's squared distance, on the lane that ranks it
    for (int e = lane; e < E; e += 64) {
        const int p = e / kp, j = e - p * kp;
        const double de = kd[e];
        const int ge = ki[e];
        int rank = j;
        for (int p2 = 0; p2 < P; ++p2) {
            if (p2 == p) continue;
            int lo = 0, hi = kp;  // entries of list p2 in front of (de, ge)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                const double dm = kd[p2 * kp + mid];
                const int gm = ki[p2 * kp + mid];
                if (dm < de || (dm == de && gm < ge)) lo = mid + 1;
                else hi = mid;
            }
            rank += lo;
        }
        if (rank < k) {
            idx_out[(int64_t)q * k + rank] = ge;
            if (dist_out) dist_out[(int64_t)q * k + rank] = sqrt(de);
            fail |= j == kp - 1;  // a partition's list ends inside the first k
            if (rank == k - 1) kthv = de;
        }
    }
    bool any_fail = __builtin_amdgcn_ballot_w64(fail) != 0;
    for (int o = 32; o > 0; o >>= 1) kthv = fmax(kthv, __shfl_xor(kthv, o));
    // partitions searched within the seed distance (large_k_search) are complete up to it only: the k-th must lie inside
    if (seed_d2 && !(kthv >= 0.0 && kthv < (double)seed_d2[q])) any_fail = true;
    if (any_fail)  // (see lk_merge: every entry of a failed row a valid position; later in the wave's program order than the ranks' stores)
        for (int r = lane; r < k; r += 64) idx_out[(int64_t)q * k + r] = 0;
    if (kth_out && lane == 0) kth_out[q] = any_fail || kthv < 0.0 ? __builtin_inf() : sqrt(kthv);
    if (any_fail && lane == 0) report_uncertified(q, flagged, opt);
}

// The merge for k beyond ~900 (`prop.k` = 0.05 of 100 000 cells is k = 5 000, R/MNN_tree.R:140-146): up to LKB_MAXE candidates a
// query, one workgroup per query (LKB_T threads: 256 up to 3 584 candidates, 512 up to 7 168, 1 024 beyond).  No rank counting (E x P binary searches would be 2e7 steps a query at
// P = 358) and no sort of all E: every thread keeps its <= 14 candidates in registers; the k-th smallest (squared distance,
// position) is found by bisection on the distances' bit patterns -- non-negative doubles order like unsigned integers; a round is
// a count and a block reduction --, the k selected candidates are compacted into the LDS and only THEY are sorted (bitonic
// network over the next power of two: 12 bytes an entry, 96 KB at k = 5 000).  The certificate is the partitioned search's: no
// partition's last entry may be among the selected.
constexpr int LKB_PER = 14;                    // candidates a thread holds
constexpr int LKB_MAXE = 1024 * LKB_PER;       // 14 336 (1 024 threads; up to 3 584 candidates: 256 threads -- a block-wide
                                               // barrier of 4 waves instead of 16, ~200 of them a query, and eight queries a CU)
constexpr int LKB_MAXK = 8192;                 // the sort's entries: 12 B x 8 192 = 96 KB of LDS

template <int LKB_T>
__global__ __launch_bounds__(LKB_T) void lk_merge_big(const double* __restrict__ X, const int32_t* __restrict__ rows, int nr, int P,
                                                      int kp, const double* __restrict__ Q, const int32_t* __restrict__ qrs,
                                                      int nq, int d, int k, const int32_t* __restrict__ sub_idx,
                                                      int32_t* __restrict__ idx_out, double* __restrict__ dist_out,
                                                      int32_t* __restrict__ flagged, int32_t* __restrict__ opt,
                                                      double* __restrict__ kth_out, const float* __restrict__ seed_d2,
                                                      const double* __restrict__ sub_d2) {
    extern __shared__ __attribute__((aligned(16))) char lkb_smem[];
    __shared__ int sh_cnt[LKB_T / 64], sh_cb[2][LKB_T / 64];
    __shared__ int sh_fail, sh_base;
    const int E = P * kp, q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int np2 = 1;
    while (np2 < k) np2 <<= 1;
    double* kd = reinterpret_cast<double*>(lkb_smem);    // [np2] the selected candidates, then sorted
    int32_t* ki = reinterpret_cast<int32_t*>(kd + np2);  // [np2]
    const LkLists L{X, rows, nr, P, kp, Q + (int64_t)(qrs ? qrs[q] : q) * d, q, nq, d, sub_idx, sub_d2};
    // ---- exact squared distances in the reference's order of operations; this thread's candidates stay in registers
    unsigned long long mine[LKB_PER];  // (+inf: beyond E, or an empty place of a list)
    int gmine[LKB_PER];
#pragma unroll
    for (int u = 0; u < LKB_PER; ++u) {
        const LkCand c = lk_fetch(L, tid + u * LKB_T);
        mine[u] = (unsigned long long)__double_as_longlong(c.d2);
        gmine[u] = c.pos;
    }
    // block-wide count of this thread's candidates that satisfy pred
    // (a wave's count: one ballot per candidate place, counted on the scalar side; the waves' counts meet in one of two LDS rows
    // in turn -- one barrier a round: a row is written again two rounds later, behind the barrier of the round in between)
    int cb_par = 0;
    auto count_block = [&](auto pred) -> int {
        int c = 0;
#pragma unroll
        for (int u = 0; u < LKB_PER; ++u) c += __popcll(__builtin_amdgcn_ballot_w64(pred(mine[u], gmine[u])));
        if (lane == 0) sh_cb[cb_par][w] = c;
        __syncthreads();
        int t = 0;
        for (int ww = 0; ww < LKB_T / 64; ++ww) t += sh_cb[cb_par][ww];
        cb_par ^= 1;
        return t;
    };
    // ---- the k-th smallest distance: the smallest bit pattern with at least k candidates at or below it
    unsigned long long vk = 0;
    for (int b = 62; b >= 0; --b) {  // (bit 63 is the sign: never set)
        const unsigned long long trial = vk | ((1ull << b) - 1ull);  // the largest value with the bits decided so far and this bit clear
        const int c = count_block([&](unsigned long long v, int) { return v <= trial; });
        if (c < k) vk |= 1ull << b;
    }
    // partitions searched within the seed distance (large_k_search) are complete up to it only: the k-th must lie inside.
    // (Fewer than k candidates in all -- seeded lists may be short -- leaves vk beyond +inf: nothing to select, the query goes
    // to the exact scan.)  vk is the same on every thread.
    if (vk >= 0x7FF0000000000000ull || (seed_d2 && !(__longlong_as_double((long long)vk) < (double)seed_d2[q]))) {
        for (int r = tid; r < k; r += LKB_T) idx_out[(int64_t)q * k + r] = 0;  // (see lk_merge: every entry a valid position)
        if (tid == 0) {
            if (kth_out) kth_out[q] = __builtin_inf();
            report_uncertified(q, flagged, opt);
        }
        return;
    }
    // ... and among the candidates AT that distance the m with the smallest positions (exact duplicates: rare)
    const int below = count_block([&](unsigned long long v, int) { return v < vk; });
    const int ties = count_block([&](unsigned long long v, int) { return v == vk; });
    int gk = 0x7fffffff;
    if (ties > k - below) {
        int lo = 0;  // the smallest position bound with at least k - below ties at or below it
        for (int b = 30; b >= 0; --b) {
            const int trial = lo | ((1 << b) - 1);
            const int c = count_block([&](unsigned long long v, int g) { return v == vk && g <= trial; });
            if (c < k - below) lo |= 1 << b;
        }
        gk = lo;
    }
    auto selected = [&](unsigned long long v, int g) { return v < vk || (v == vk && g <= gk); };
    // ---- the certificate: no partition's last entry among the selected (it sits at e = p kp + kp - 1)
    if (tid == 0) sh_fail = 0;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < LKB_PER; ++u) {
        const int e = tid + u * LKB_T;
        if (e < E && (e % kp) == kp - 1 && selected(mine[u], gmine[u])) sh_fail = 1;
    }
    // ---- the selected to the front (k of them: vk is finite whenever k <= the candidates there are), sorted
    if (tid == 0) sh_base = 0;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < LKB_PER; ++u) {
        const bool s1 = selected(mine[u], gmine[u]);
        const unsigned long long m = __builtin_amdgcn_ballot_w64(s1);
        if (lane == 0) sh_cnt[w] = __popcll(m);
        __syncthreads();
        int off = sh_base;
        for (int ww = 0; ww < w; ++ww) off += sh_cnt[ww];
        if (s1) {
            const int pos = off + __popcll(m & ((1ull << lane) - 1ull));
            kd[pos] = __longlong_as_double((long long)mine[u]);
            ki[pos] = gmine[u];
        }
        __syncthreads();
        if (tid == 0) {
            int t = 0;
            for (int ww = 0; ww < LKB_T / 64; ++ww) t += sh_cnt[ww];
            sh_base += t;
        }
        __syncthreads();
    }
    for (int i = k + tid; i < np2; i += LKB_T) {
        kd[i] = __builtin_inf();
        ki[i] = 0x7fffffff;
    }
    __syncthreads();
    block_bitonic_sort<LKB_T>(kd, ki, np2);
    for (int r = tid; r < k; r += LKB_T) {
        idx_out[(int64_t)q * k + r] = ki[r];
        if (dist_out) dist_out[(int64_t)q * k + r] = sqrt(kd[r]);
    }
    if (tid == 0) {
        if (kth_out) kth_out[q] = sh_fail ? __builtin_inf() : sqrt(kd[k - 1]);
        if (sh_fail) report_uncertified(q, flagged, opt);
    }
}

// optimistic run: the queries a merge could not certify are on the device (flagged[0] of them).  Up to LK_OPT_CAP take the full
// FP64 scan there and then (launched whatever the count: with none flagged its workgroups end at once); more raise the run's
// flag (opt[0]) and the engine repeats the run with host-checked searches.  opt[1] counts the queries that took an exact path.
constexpr int LK_OPT_CAP = 32;
__global__ void lk_opt_overflow(const int32_t* __restrict__ flagged, int32_t* __restrict__ opt) {
    const int c = flagged[0];
    if (c > LK_OPT_CAP) atomicOr(&opt[0], 1);
    if (c > 0) atomicAdd(&opt[1], c < LK_OPT_CAP ? c : LK_OPT_CAP);
}

}  // namespace

bool large_k_search(hipStream_t stream, KnnWorkspace& ws, const double* X, const int32_t* ref_rows, int nr, const double* Qs,
                    const int32_t* qrs, int nq, int d, int k, int32_t* io, double* dout, const double* centre,
                    double* kth_out) {
    // neighbours asked of a partition: 36 where a tier holds that many (rows of up to 61 columns), else 20 (up to 125); a
    // partition holds 0.45 of that of a query's k on average, so that one holding all of it is rare
    Tier tiers[2];
    int kp = 36;
    if (candidate_tiers(d, kp, std::max(nr / cdiv(k, 16), 1), tiers) == 0) kp = 20;
    int P = std::max(2, cdiv(k, kp == 36 ? 16 : 9));
    // beyond what the rank-counting merges take (2 048 candidates): the big merge, with partitions dealt a little finer -- 14
    // (8) of a query's k each on average -- so that a partition holding all kp of them is rarer still (one such query would
    // send an optimistic engine run back to its start)
    if ((int64_t)P * kp > LK_MAXE) P = cdiv(k, kp == 36 ? 14 : 8);
    if ((int64_t)P * kp > LKB_MAXE || k > LKB_MAXK || nr / P < 4 * kp) return false;
    if (candidate_tiers(d, kp, nr / P, tiers) == 0) return false;
    int32_t* rows = ws.lk_rows.reserve((size_t)nr);
    int32_t* sub = ws.lk_idx.reserve((size_t)P * nq * kp);
    hipLaunchKernelGGL(lk_partition_rows, dim3(cdiv(nr, 256)), dim3(256), 0, stream, ref_rows, nr, P, rows);
    BMX_LAUNCH_CHECK();
    const int base = nr / P, rem = nr % P;
    // The partitions are strided samples of one reference: a query's kp-th distance in the first is about its kp-th distance in
    // every other.  So the first is searched plainly and its (certified) kp-th distance seeds the rest: their thresholds start
    // there instead of at +inf -- a partition of ~1 400 cells is otherwise one long warm-up, every early value a survivor for the
    // service waves (1.34 ms a launch at k = 1 000 against 13 us of matrix work).  A seeded list is complete up to the seed only;
    // the merges' certificate asks the k-th merged distance to lie inside it.
    // The partitions' searches leave their exact SQUARED distances (the reference's sum, left to right -- what the merges used to
    // gather every candidate's row for: 2 592 rows of 400 bytes a query at k = 1 000, 49 ms of a 100 ms search).
    const size_t n_sub = (size_t)P * nq * kp;
    double* sub_d2 = n_sub * sizeof(double) <= ((size_t)16 << 30) ? ws.lk_d2.reserve(n_sub) : nullptr;
    struct SquaredScope {
        KnnWorkspace& w;
        ~SquaredScope() { w.dist_squared = false; }
    } squared_scope{ws};
    ws.dist_squared = sub_d2 != nullptr;
    const bool seeded = dev_knobs().lk_seed != 0 && P >= 3;
    double* kth0 = seeded ? ws.lk_kth.reserve((size_t)nq) : nullptr;
    float* seed = seeded ? ws.lk_seed.reserve((size_t)nq) : nullptr;
    for (int p = 0; p < P; ++p) {
        const int n_p = base + (p < rem ? 1 : 0);
        const int nt = candidate_tiers(d, kp, n_p, tiers);
        search_tiers(stream, ws, tiers, nt, 0, X, rows + (int64_t)p * base + std::min(p, rem), n_p, Qs, qrs, nq, d, kp,
                     sub + (int64_t)p * nq * kp, sub_d2 ? sub_d2 + (int64_t)p * nq * kp : nullptr, p > 0 ? seed : nullptr, centre,
                     p == 0 ? kth0 : nullptr);
        if (p == 0 && seeded) {
            hipLaunchKernelGGL(lk_seed_kernel, dim3(cdiv(nq, 256)), dim3(256), 0, stream, (const double*)kth0, nq, seed);
            BMX_LAUNCH_CHECK();
        }
    }
    ws.dist_squared = false;  // (what follows writes the caller's distances)
    int32_t* flagged = ws.flagged_t[0].reserve((size_t)nq + 1);
    int32_t* opt = ws.optimistic ? ws.opt_state_ptr(stream) : nullptr;
    BMX_HIP(hipMemsetAsync(flagged, 0, sizeof(int32_t), stream));
    int32_t* const no_opt = nullptr;  // (the merges list what they cannot certify in either kind of run)
    if (P * kp > 1024) {  // (the bisection merge sorts the k selected, lk_merge all the candidates: measured equal at 684 candidates
                          // a query (k = 300), 88 against 100 ms a config-2 step at 1 152 (k = 500))
        size_t np2 = 1;
        while (np2 < (size_t)k) np2 <<= 1;
        const size_t lds = np2 * 12;
        auto big = [&](auto threads) {
            constexpr int T = decltype(threads)::value;
            ensure_dynamic_lds(reinterpret_cast<const void*>(&lk_merge_big<T>), lds);
            hipLaunchKernelGGL(lk_merge_big<T>, dim3(nq), dim3(T), lds, stream, X, (const int32_t*)rows, nr, P, kp, Qs, qrs, nq, d, k,
                               (const int32_t*)sub, io, dout, flagged, no_opt, kth_out, (const float*)seed, (const double*)sub_d2);
        };
        if (P * kp <= 256 * LKB_PER) big(std::integral_constant<int, 256>{});
        else if (P * kp <= 512 * LKB_PER) big(std::integral_constant<int, 512>{});
        else big(std::integral_constant<int, 1024>{});
    } else if (P * kp <= 512)
        hipLaunchKernelGGL(lk_merge_wave, dim3(cdiv(nq, 4)), dim3(256), 0, stream, X, (const int32_t*)rows, nr, P, kp, Qs, qrs, nq,
                           d, k, (const int32_t*)sub, io, dout, flagged, no_opt, kth_out, (const float*)seed, (const double*)sub_d2);
    else
        hipLaunchKernelGGL(lk_merge, dim3(nq), dim3(256), 0, stream, X, (const int32_t*)rows, nr, P, kp, Qs, qrs, nq, d, k,
                           (const int32_t*)sub, io, dout, flagged, no_opt, kth_out, (const float*)seed, (const double*)sub_d2);
    BMX_LAUNCH_CHECK();
    if (!opt) {
        const int count = read_count(stream, ws, flagged);
        if (count > 0) exact_search(stream, ws, X, ref_rows, nr, Qs, qrs, d, k, io, dout, flagged, nullptr, count);
    } else {
        // (one query whose first partition holds 36 of its k used to send the whole run back to its start: 7 of 300 000 queries a
        // step did at k = 1 000, every step ran twice)
        hipLaunchKernelGGL(lk_opt_overflow, dim3(1), dim3(1), 0, stream, (const int32_t*)flagged, opt);
        BMX_LAUNCH_CHECK();
        double* drow = ws.drow.reserve((size_t)LK_OPT_CAP * nr);
        launch_full_scan(stream, ws, X, ref_rows, nr, Qs, qrs, d, k, io, dout, flagged, 0, 0, LK_OPT_CAP, drow);
    }
    return true;
}

}  // namespace bmx
