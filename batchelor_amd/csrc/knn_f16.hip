// Tier 1 of the exact kNN: a single-product fp16 candidate pass (MI355X / gfx950).
//
// The candidate pass only has to be accurate enough for the FP64 certificate of knn_refine to hold for almost every
// query; the few it cannot certify go on to the split-bf16 pass (knn_bf16.hip) and, failing that, to the exact
// FP64 scan.  So here every operand is ONE fp16 value: with the centred coordinates scaled by a power of two s so
// that the largest reference norm lands in (24, 48] (no overflow, no underflow that matters),
//     v' = |r'|^2 - 2 q'.r'   comes out of one chain of K/16 v_mfma_f32_32x32x16_f16 over
//     refs    [ r'_1 .. r'_d | n1 n2 n3 | 0 .. ],   n1 + n2 + n3 = f32(|r'|^2) exactly (three fp16 pieces)
//     queries [ -2 q'_1 .. -2 q'_d | 1 1 1 | 0 .. ]
// with |v' - exact| <= 2^-9 (1 + 2^-12) |q'||r'| + f32 accumulation terms: 4 MFMAs per 32 x 32 tile at 50 PCs
// (K = 64) against 10 for the split-bf16 pass (K = 160).  At 50 PCs on 100 000 reference cells the bound is about
// 0.05 against a gap of 0.35 between the 20th and the 32nd neighbour, so with KS = 32 kept candidates practically
// every query is certified.  (The prepared images: knn_prep.hip.  The same tile as four 16 x 16 blocks of
// v_mfma_f32_16x16x32_f16, the kernel's MS = 1: at knn_topk_f16 below; what follows describes MS = 0.)
//
// With the matrix work that cheap, what happens around it sets the pace, so a workgroup (one per CU) splits it over
// three kinds of waves.  knn_topk_f16 decodes the work item, carves the LDS and dispatches; producers and service waves
// are a function each, the consumers' sweep stays in the kernel's body (its steps lambdas on the kernel's locals):
//   * producers (2 waves, producer_role) stream the prepared reference image into an LDS ring whose slots hold TP PAIRS of
//     tiles: four tiles (TP = 2) where three such slots fit beside the lists (KS = 32, NS <= 4), else two (F16Shape);
//   * consumers (8 waves x 32 queries, `sweep`) sweep the ring.  Per pair of tiles (tile_pair): the two tiles' MFMA chains
//     interleaved on independent accumulators with the fragment reads of the next pair in their gaps, then the filter (sift)
//     -- the 32 x 32 accumulator puts a query on each lane; min over its 16 values (v_min3 tree), one compare, one scalar
//     branch: most tiles end here -- and the spill: a lane whose group of 4 consecutive references holds a survivor dumps the
//     group's four raw values (one ds_write_b128) and a tag (tile, group, lane) into its wave's queue in the LDS.  Nothing
//     else: no list handling, no threshold bookkeeping in the sweep; ready check, polls and hand-back come once per slot;
//   * service waves (4, lowest issue priority, service_role) work the queues off while the consumers sweep (drain_pass):
//     32 records = 128 values per pass with all 64 lanes busy, each lane re-tests values against their query's current
//     threshold and appends survivors to the query's list with an LDS atomic; a list (KS kept + pending, <= 64 entries,
//     unsorted) is cut back to about its KS smallest by pivot trials / quickselect over the wave (compact_list, select_rank)
//     and the threshold, an LDS word the consumer re-reads once per slot, drops to the cut.  They also write the final
//     lists out (write_final_lists; the consumers help: consumer_epilogue).
// Hand-over everywhere through LDS words and counters, no barrier in the loop.  Shared thresholds across reference
// ranges and the register-only sample pass (sample_epilogue) follow knn_bf16.hip.  What the LDS holds and where:
// knn_f16_shape.hpp (F16Shape, F16Lds), which also has the kernel's tunables.
//
// Every function and lambda of the kernel is force-inlined: left to its own devices the compiler turned the compaction and the
// drain pass into real calls once they grew -- their context then lives in scratch and every LDS atomic becomes a flat one.
#include "knn_f16_shape.hpp"
#include "knn_tier.hpp"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

namespace bmx {
namespace {

using namespace sel;
using namespace f16;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) int* lds_iptr;
typedef __attribute__((address_space(3))) const char* lds_cptr;
typedef __attribute__((address_space(3))) const f32x4* lds_f4ptr;

// What the roles of one workgroup share: where its LDS regions lie, which work item it is, the kernel's arguments.
template <int NS, int KS>
struct PassCtx {
    using S = F16Shape<NS, KS>;
    F16Lds<S> lds;
    int lane, wave;  // (wave: wave-uniform, branches on it are scalar)
    int qblock, rng, nrng, r_begin;  // the work item (knn_tier.hpp)
    int ntiles, nslots;              // reference tiles of its range (even), ring slots of them
    int out_chunk, out_nchunks;      // the list column this item writes, of how many
    bool shared_tau;                 // the ranges of a query block tighten one another's thresholds through tau_g
    const uint16_t* Pq;
    const uint16_t* PrF;
    uint32_t* tau_g;
    int32_t* cand;
    float* cand_v;
    float* tau_out;
    const float* margin_g;
    int kq;
    const uint32_t* tau_seed;
};

// ---- the cycle stamps of the developer build leave the kernel here (make STAMPS=1; launch() prints them)
#ifdef BMX_STAMPS
__device__ unsigned long long bmx_dbg16[48];
__device__ __forceinline__ void stamps_out_service(const Stamps& st, const int lane) {
    if (lane == 0) {
        atomicAdd(&bmx_dbg16[2], st.get(Stamps::DRAIN));
        atomicAdd(&bmx_dbg16[3], st.get(Stamps::NDRAIN));
        atomicAdd(&bmx_dbg16[4], st.get(Stamps::NCOMP));
        atomicAdd(&bmx_dbg16[5], st.get(Stamps::COMP));
        atomicAdd(&bmx_dbg16[11], st.get(Stamps::ROUNDS));
        atomicAdd(&bmx_dbg16[13], st.elapsed());
        atomicAdd(&bmx_dbg16[14], 1ull);
        atomicAdd(&bmx_dbg16[15], st.get(Stamps::IDLE));
    }
}
// the sweep of the first consumer of every workgroup in cycles and in 100 MHz ticks: launch() prints the median clock
constexpr int CLK_WGS = 4096;
__device__ unsigned long long bmx_clk16[2 * CLK_WGS];
template <bool SAMPLE>
__device__ __forceinline__ void stamps_out_consumer(const Stamps& st, const int lane, const int wave, const int ntiles) {
    if (lane == 0 && wave == 0 && blockIdx.x < CLK_WGS) {
        bmx_clk16[2 * blockIdx.x] = st.sweep_cycles;
        bmx_clk16[2 * blockIdx.x + 1] = st.sweep_ticks;
    }
    if (lane == 0) {
        atomicAdd(&bmx_dbg16[0], st.elapsed());
        atomicAdd(&bmx_dbg16[1], st.get(Stamps::SPIN));
        atomicAdd(&bmx_dbg16[8], (unsigned long long)ntiles);
        atomicAdd(&bmx_dbg16[9], 1ull);
        if constexpr (!SAMPLE) {
            atomicAdd(&bmx_dbg16[6], st.get(Stamps::EVT));
            atomicAdd(&bmx_dbg16[7], st.get(Stamps::GRP));
            atomicAdd(&bmx_dbg16[10], st.get(Stamps::EVC));
            atomicAdd(&bmx_dbg16[12], st.get(Stamps::QWAIT));
        }
    }
}
#else
__device__ __forceinline__ void stamps_out_service(const Stamps&, const int) {}
template <bool SAMPLE>
__device__ __forceinline__ void stamps_out_consumer(const Stamps&, const int, const int, const int) {}
#endif

// =====================================================================================================================
// shared by service and consumer waves: compaction of a list, the final lists
// =====================================================================================================================
// quickselect: the key with exactly `target` smaller keys among the lanes of B; leaves it in (pl, pk, M)
__device__ __forceinline__ void select_rank(const uint32_t key, const int jj, unsigned long long B, const int target, int& pl,
                                            uint32_t& pk, unsigned long long& M, Stamps& st) {
    int it = 0;
    for (;;) {
        const int rot = (it * 29 + jj * 7) & 63;  // pivots from changing places
        ++it;
        const unsigned long long Br = B >> rot;
        pl = Br ? rot + __builtin_ctzll(Br) : __builtin_ctzll(B);
        pk = (uint32_t)__builtin_amdgcn_readlane((int)key, pl);
        M = __builtin_amdgcn_ballot_w64(key < pk);
        const int cc = __builtin_popcountll(M);
        if (cc == target) break;
        if (cc > target)
            B &= M;
        else
            B &= ~M & ~(1ull << pl);
    }
    st.add(Stamps::ROUNDS, (unsigned long long)it);
}

// ---- compaction of query jj's list (jj wave-uniform) of consumer c: cut it back to about KS entries,
// tighten the threshold.  The cut need not sit exactly at rank KS: any entry with at least KS - 1 smaller
// ones is a valid new threshold (everything above it is dropped, at least KS stay).  BMX_NPIV entries from
// fixed, evenly spread places of the (unordered) list are tried at once -- independent readlane / compare /
// popcount chains instead of a dependent chain of quickselect rounds -- and the one that keeps the fewest,
// at least KS, wins.  Only when none qualifies or the best would free too little does the exact quickselect
// run.
template <int NS, int KS>
__device__ __forceinline__ void compact_list(const PassCtx<NS, KS>& cx, Stamps& st, const int c, const int jj, const bool exact) {
    using S = F16Shape<NS, KS>;
    constexpr int LCAP = S::LCAP, KEEP_MAX = S::KEEP_MAX;
    const int lane = cx.lane, kq = cx.kq;
    float* const tauL = cx.lds.tauL;
    unsigned long long* mylists = cx.lds.lists + c * 32 * LCAP;
    int* mycnt = cx.lds.cnt + c * 32;
    const int n_raw = __builtin_amdgcn_readfirstlane(lds_load_volatile(&mycnt[jj]));
    const int n = n_raw < LCAP ? n_raw : LCAP;
    if (n <= KS && (n < kq || cx.margin_g == nullptr)) return;
    const unsigned long long c0 = st.now();
    st.count(Stamps::NCOMP);
    const unsigned long long raw = lane < n ? mylists[jj * LCAP + lane] : 0ull;
    // 31-bit rank key: order-preserving image of the value with its low bits replaced by the lane number
    // (unique keys; values closer than 2^-17 relative may swap places at the cut, see below)
    const uint32_t key =
        lane < n ? (((f32_orderable(__uint_as_float((uint32_t)(raw >> 32))) >> 1) & ~63u) | (uint32_t)lane)
                 : 0x7FFFFFFFu;
    unsigned long long M = 0, keep = 0;
    int pl = 0, kept = 0x7FFFFFFF, nkeep = 0;
    uint32_t pk = 0;
    float newtau = 0.f;
    bool cut_done = false;
    const unsigned long long all_lanes = n == 64 ? ~0ull : ((1ull << n) - 1ull);
    // The margin cut: everything above (k-th best value + twice the error bound) is farther, exactly, than k others
    // of the list whatever the rounding did, so it can go -- typically a handful of entries beyond the k-th stay
    // instead of KS - k, and the threshold (what the consumers filter with) sits that much lower.  It applies when
    // the list has k entries and what it keeps fits; otherwise the rank cut below.
    const float mg = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(cx.lds.mgL[c * 32 + jj])));
    if (mg > 0.f && n >= kq) {
        select_rank(key, jj, all_lanes, kq - 1, pl, pk, M, st);
        const float vk = orderable_f32((pk & ~63u) << 1);  // the k-th best value, low bits cleared (within 2^-17 of it)
        const float tm = vk + mg + fabsf(vk) * 6.103515625e-05f;  // (+ 2^-14: the cleared bits of vk and of the cut)
        const uint32_t ck = (f32_orderable(tm) >> 1) & ~63u;  // as a key with its lane bits cleared: <= tm
        const unsigned long long Mm = __builtin_amdgcn_ballot_w64(key < ck);
        const int cc = __builtin_popcountll(Mm);
        if (cc >= kq && cc <= (exact ? KS : KEEP_MAX)) {
            keep = Mm;
            nkeep = cc;
            newtau = orderable_f32(ck << 1);  // <= the value of everything dropped
            cut_done = true;
        }
    }
    if (!cut_done) {
        if (n <= KS) return;
        M = 0;
        pl = 0;
        pk = 0;
#pragma unroll
        for (int i = 0; i < BMX_NPIV; ++i) {
            const int pv = ((2 * i + 1) * n) / (2 * BMX_NPIV);  // < n
            const uint32_t k_i = (uint32_t)__builtin_amdgcn_readlane((int)key, pv);
            const unsigned long long m_i = __builtin_amdgcn_ballot_w64(key < k_i);
            const int c_i = __builtin_popcountll(m_i);
            if (c_i >= KS - 1 && c_i < kept) {
                kept = c_i;
                M = m_i;
                pl = pv;
                pk = k_i;
            }
        }
        if (exact ? kept != KS - 1 : kept + 1 > KEEP_MAX) {
            // quickselect for the key with exactly KS - 1 smaller keys; B = lanes that can still be it
            unsigned long long B = all_lanes;
            if (kept != 0x7FFFFFFF) B &= M;  // below the best pivot found
            select_rank(key, jj, B, KS - 1, pl, pk, M, st);
            kept = KS - 1;
        }
        keep = M | (1ull << pl);  // kept + 1 lanes, at least KS
        nkeep = kept + 1;
        // the new threshold: the cut key with its lane bits cleared, which is <= the value of everything
        // dropped, so "rejected => value >= threshold" holds exactly
        newtau = orderable_f32((pk & ~63u) << 1);
    }
    const int pos = mbcnt64(keep);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // every lane holds its entry before slots are rewritten
    if ((keep >> lane) & 1ull) mylists[jj * LCAP + pos] = raw;
    if (lane == 0) mycnt[jj] = nkeep;
    if (lane == jj) {
        const float told = tauL[c * 32 + jj];
        tauL[c * 32 + jj] = newtau < told ? newtau : told;  // the consumer picks it up at its next slot
        if (cx.shared_tau) atomicMin(&cx.tau_g[cx.qblock * NQ + c * 32 + jj], f32_orderable(newtau));
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    st.since(Stamps::COMP, c0);
}

// ---- final lists [j0, j1) of consumer c out (its queue is empty, nothing appends any more)
template <int NS, int KS>
__device__ __forceinline__ void write_final_lists(const PassCtx<NS, KS>& cx, Stamps& st, const int c, const int j0, const int j1) {
    constexpr int LCAP = F16Shape<NS, KS>::LCAP;
    const int lane = cx.lane, nrng = cx.nrng, out_nchunks = cx.out_nchunks, out_chunk = cx.out_chunk;
    int32_t* const cand = cx.cand;
    float* const cand_v = cx.cand_v;
    float* const tau_out = cx.tau_out;
    unsigned long long* mylists = cx.lds.lists + c * 32 * LCAP;
    int* mycnt = cx.lds.cnt + c * 32;
    for (int jj = j0; jj < j1; ++jj) compact_list(cx, st, c, jj, true);  // the output holds exactly KS entries per list
    for (int jj = j0; jj < j1; ++jj) {
        const int qq = cx.qblock * NQ + c * 32 + jj;
        const int n = __builtin_amdgcn_readfirstlane(lds_load_volatile(&mycnt[jj]));  // <= KS now
        // what this range rejected was rejected against thresholds >= the final working threshold (the consumer
        // filters with a copy of its service wave's threshold, never a tighter one); kept entries at or above it
        // are as good as rejected (another range holds KS better ones): dropped here
        const float eff = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane(
            (int)__float_as_uint(__hip_atomic_load(&cx.lds.tauL[c * 32 + jj], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))));
        if (lane < KS) {
            const unsigned long long e = lane < n ? mylists[jj * LCAP + lane] : 0ull;
            const float val = __uint_as_float((uint32_t)(e >> 32));
            const bool keep = lane < n && (val < eff || nrng == 1);
            const int64_t o = ((int64_t)qq * out_nchunks + out_chunk) * KS + lane;
            cand[o] = keep ? (int32_t)(uint32_t)e : -1;
            cand_v[o] = lane < n ? val : __builtin_inff();
        }
        if (lane == 0) tau_out[(int64_t)qq * out_nchunks + out_chunk] = eff;
        if (nrng == 1) {  // a whole-reference item owns every list column of its queries: the others stay empty
            for (int cc = 1; cc < out_nchunks; ++cc) {
                if (lane < KS) cand[((int64_t)qq * out_nchunks + out_chunk + cc) * KS + lane] = -1;
                if (lane == 0) tau_out[(int64_t)qq * out_nchunks + out_chunk + cc] = __builtin_inff();
            }
        }
    }
}

// =====================================================================================================================
// producer (as in knn_bf16.hip)
// =====================================================================================================================
template <int NS, int KS>
__device__ __forceinline__ void producer_role(const PassCtx<NS, KS>& cx) {
    using S = F16Shape<NS, KS>;
    constexpr int NSLOT = S::NSLOT, TP = S::TP, SLOT_BYTES = S::SLOT_BYTES, TILE_BYTES = S::TILE_BYTES;
    const int lane = cx.lane, nslots = cx.nslots;
    int* const ready = cx.lds.ready;
    int* const done = cx.lds.done;
    const int p = cx.wave - NCONS;
    f32x4 ra[2 * NS], rb[2 * NS];
    const f32x4* src = reinterpret_cast<const f32x4*>(cx.PrF) + ((int64_t)(cx.r_begin >> 5) * NS) * 64 + lane;
    f32x4* ring_l = reinterpret_cast<f32x4*>(cx.lds.ring) + lane;
    auto load = [&](f32x4(&r)[2 * NS], int sl) {  // both tiles of slot sl: 2 NS contiguous 1 KiB pieces
#pragma unroll
        for (int s = 0; s < 2 * NS; ++s) r[s] = src[((int64_t)sl * 2 * NS + s) * 64];
    };
    // slot sl goes to ring position sl % NSLOT once every consumer has read the slots staged there before it:
    // done[pos] counts the hand-backs of the position, NCONS per slot
    auto wait_free = [&](int sl, int pos) __attribute__((always_inline)) {
        if (sl < NSLOT) return;
        const int need = (sl / NSLOT) * NCONS;
        while (__builtin_amdgcn_readfirstlane(lds_load_volatile(&done[pos])) < need)
            __builtin_amdgcn_s_sleep(BMX_PSLEEP);
    };
    auto publish = [&](const f32x4(&r)[2 * NS], int sl) {
        const int pos = sl % NSLOT;
        wait_free(sl, pos);
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        f32x4* dst = ring_l + pos * (SLOT_BYTES / 16);
#pragma unroll
        for (int s = 0; s < 2 * NS; ++s) dst[s * 64] = r[s];
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        // same wave, in-order LDS queue: the flag lands after the tiles
        if (lane == 0) __hip_atomic_store(&ready[pos], sl + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    // two register sets: the loads of slot sl + NPROD stay in flight while slot sl is handed over.  Every load below is
    // unconditional (past the end: the last slot again, never published): with conditional loads the compiler has to
    // wait for ALL outstanding loads before it touches a register set -- the set just asked for included -- because
    // it cannot tell how many are in flight
    if constexpr (TP == 1) {
        if (nslots > 0) {
            const int last = nslots - 1;
            int sl = p;
            load(ra, sl < last ? sl : last);
            load(rb, sl + NPROD < last ? sl + NPROD : last);
            for (; sl < nslots; sl += 2 * NPROD) {
                publish(ra, sl);
                load(ra, sl + 2 * NPROD < last ? sl + 2 * NPROD : last);
                if (sl + NPROD < nslots) publish(rb, sl + NPROD);
                load(rb, sl + 3 * NPROD < last ? sl + 3 * NPROD : last);
            }
        }
    } else {
        // slots of four tiles: a producer stages whole slots, its two register sets hold the two halves of one; the
        // ready word goes out after the second half
        auto load_half = [&](f32x4(&r)[2 * NS], int sl, int half) {
#pragma unroll
            for (int s = 0; s < 2 * NS; ++s) r[s] = src[(((int64_t)sl * TP + half) * 2 * NS + s) * 64];
        };
        auto store_half = [&](const f32x4(&r)[2 * NS], int pos, int half) {
            f32x4* dst = ring_l + pos * (SLOT_BYTES / 16) + half * (2 * TILE_BYTES / 16);
#pragma unroll
            for (int s = 0; s < 2 * NS; ++s) dst[s * 64] = r[s];
        };
        if (nslots > 0) {
            const int last = nslots - 1;
            int sl = p;
            load_half(ra, sl < last ? sl : last, 0);
            load_half(rb, sl < last ? sl : last, 1);
            for (; sl < nslots; sl += NPROD) {
                const int pos = sl % NSLOT;
                const int nx = sl + NPROD < last ? sl + NPROD : last;
                wait_free(sl, pos);
                __atomic_signal_fence(__ATOMIC_SEQ_CST);
                store_half(ra, pos, 0);
                load_half(ra, nx, 0);
                store_half(rb, pos, 1);
                load_half(rb, nx, 1);
                __atomic_signal_fence(__ATOMIC_SEQ_CST);
                if (lane == 0) __hip_atomic_store(&ready[pos], sl + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }
    // two empty slots past the end: the consumers' loop runs one step longer than the data and always refills from
    // "slot sl + 1"
    for (int e = nslots; e < nslots + 2; ++e) {
        if (nslots > 0 && e % NPROD == p) {
            const int pos = e % NSLOT;
            wait_free(e, pos);
            if (lane == 0) __hip_atomic_store(&ready[pos], e + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
}

// =====================================================================================================================
// service wave: works off the spill queues of CPS consumer waves while they sweep -- re-test, append to the lists,
// compact, publish the thresholds -- so that a consumer's own instruction stream holds the filter and the spill only
// =====================================================================================================================
// ---- one drain pass: up to 32 records (128 values) of consumer c's queue, from position r0.  Every lane
// takes one value of a record of the first half and one of the second (two independent chains of LDS read ->
// the query's threshold -> LDS atomic slot -> store, issued together).
template <int MS, int NS, int KS>
__device__ __forceinline__ void drain_pass(const PassCtx<NS, KS>& cx, Stamps& st, const int c, const int r0, const int n) {
    constexpr int LCAP = F16Shape<NS, KS>::LCAP;
    const int lane = cx.lane;
    const unsigned long long d0 = st.now();
    st.count(Stamps::NDRAIN);
    unsigned long long* mylists = cx.lds.lists + c * 32 * LCAP;
    int* mycnt = cx.lds.cnt + c * 32;
    const float* qv = cx.lds.qvals + c * QCAP * 4;
    const uint32_t* qt = cx.lds.qtags + c * QCAP;
    const float* mytau = cx.lds.tauL + c * 32;
    bool pend[2];
    uint32_t tag[2];
    float v[2];
#pragma unroll
    for (int x = 0; x < 2; ++x) {
        const int rec = 16 * x + (lane >> 2);
        const int at = (r0 + rec) & (QCAP - 1);
        pend[x] = rec < n;
        tag[x] = qt[at];
        v[x] = qv[(at << 2) + (lane & 3)];
    }
    // the records are on their way into registers: their queue positions are free again (the store queues
    // up behind the reads in this wave's in-order LDS queue)
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    if (lane == 0) __hip_atomic_store(&cx.lds.rdL[c], r0 + n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    int jq[2], ref[2];
#pragma unroll
    for (int x = 0; x < 2; ++x) {
        const int srcl = tag[x] & 63, u = (int)((tag[x] >> 6) & 3u);  // the lane that spilled the record, its group
        if constexpr (MS == 0) {
            // query srcl & 31, row half srcl >> 5; group u: rows 8 u ...
            jq[x] = srcl & 31;
            ref[x] = cx.r_begin + ((int)(tag[x] >> 8) << 5) + u * 8 + (srcl >> 5) * 4 + (lane & 3);
        } else {
            // 16 x 16 blocks: group u = 2 a + b is the block of reference half a and query half b, the lane's column is
            // query srcl & 15 of that half, its rows 4 (srcl >> 4) ... of the block
            jq[x] = 16 * (u & 1) + (srcl & 15);
            ref[x] = cx.r_begin + ((int)(tag[x] >> 8) << 5) + 16 * (u >> 1) + 4 * (srcl >> 4) + (lane & 3);
        }
    }
    for (;;) {
        float tq[2];
        int slot[2];
#pragma unroll
        for (int x = 0; x < 2; ++x)
            tq[x] = __hip_atomic_load(&mytau[jq[x]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            pend[x] = pend[x] && v[x] < tq[x];
            slot[x] = LCAP;
            if (pend[x]) slot[x] = atomicAdd(&mycnt[jq[x]], 1);  // ds_add_rtn_u32
        }
#pragma unroll
        for (int x = 0; x < 2; ++x)
            if (slot[x] < LCAP) {
                mylists[jq[x] * LCAP + slot[x]] =
                    ((unsigned long long)__float_as_uint(v[x]) << 32) | (uint32_t)ref[x];
                pend[x] = false;
            }
        unsigned long long ov0 = __builtin_amdgcn_ballot_w64(pend[0]);
        unsigned long long ov1 = __builtin_amdgcn_ballot_w64(pend[1]);
        if ((ov0 | ov1) == 0) break;
        // full lists: cut them back (the threshold drops), then the lanes left over try again
        while (ov0 | ov1) {
            const int qq = ov0 ? __builtin_amdgcn_readlane(jq[0], __builtin_ctzll(ov0))
                               : __builtin_amdgcn_readlane(jq[1], __builtin_ctzll(ov1));
            compact_list(cx, st, c, qq, false);
            ov0 &= ~__builtin_amdgcn_ballot_w64(jq[0] == qq);
            ov1 &= ~__builtin_amdgcn_ballot_w64(jq[1] == qq);
        }
    }
    // lists about to fill are cut back now, so that the appends of the next pass rarely find one full
    const int cn = lane < 32 ? lds_load_volatile(&mycnt[lane]) : 0;
    unsigned long long need = __builtin_amdgcn_ballot_w64(cn > LCAP - HEAD);
    while (need) {
        const int jj = __builtin_ctzll(need);
        need &= need - 1;
        compact_list(cx, st, c, jj, false);
    }
    st.since(Stamps::DRAIN, d0);
}

template <int MS, int NS, int KS>
__device__ __forceinline__ void service_role(const PassCtx<NS, KS>& cx) {
    constexpr int CPS = F16Shape<NS, KS>::CPS;
    const int lane = cx.lane;
    int* const wrL = cx.lds.wrL;
    int* const rdL = cx.lds.rdL;
    int* const stL = cx.lds.stL;
    float* const tauL = cx.lds.tauL;
    __builtin_amdgcn_s_setprio(BMX_SPRIO);
    const int c0 = (cx.wave - NCONS - NPROD) * CPS;
    Stamps st;
    st.begin();
    uint32_t finmask = 0;  // bit s: consumer c0 + s is through and its final lists are out
    uint32_t tau_fetch[(CPS * 32 + 63) / 64];
#pragma unroll
    for (int x = 0; x < (CPS * 32 + 63) / 64; ++x) tau_fetch[x] = 0xFFFFFFFFu;
    int iter = 0;
    for (;;) {
        bool worked = false;
#pragma nounroll
        for (int s = 0; s < CPS; ++s) {
            if ((finmask >> s) & 1u) continue;
            const int c = c0 + s;
            // the consumer writes its last record count before the "through" state: read in the opposite order
            const int state = __builtin_amdgcn_readfirstlane(lds_load_volatile(&stL[c]));
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            const int w = __builtin_amdgcn_readfirstlane(lds_load_volatile(&wrL[c]));
            const int r = __builtin_amdgcn_readfirstlane(lds_load_volatile(&rdL[c]));  // this wave's own word
            const int avail = w - r;
            // a short queue is left to grow (a pass costs the same for 1 record as for 32) unless its consumer
            // waits for room or is through
            if (avail >= DRAIN_MIN || (state != 0 && avail > 0)) {
                drain_pass<MS>(cx, st, c, r, avail < 32 ? avail : 32);
                worked = true;
            } else if (state == 2) {
                // nothing will be appended any more: the consumer wave writes the first EPI_CONS final lists out
                // itself, this wave the rest
                __atomic_signal_fence(__ATOMIC_SEQ_CST);
                if (lane == 0) __hip_atomic_store(&stL[c], 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                write_final_lists(cx, st, c, EPI_CONS, 32);
                finmask |= 1u << s;
                worked = true;
            }
        }
        if (finmask == (1u << CPS) - 1u) break;
        if (cx.shared_tau) {
            // thresholds other ranges have reached: the (L1-bypassing) loads are issued in one round of the loop
            // and looked at in the next, so nobody waits for the round trip
            ++iter;
#pragma unroll
            for (int x = 0; x < (CPS * 32 + 63) / 64; ++x) {
                const int qi = c0 * 32 + x * 64 + lane;  // query of the block (CPS * 32 is a multiple of 64)
                if ((iter & 15) == 1) {
                    const float t = orderable_f32(tau_fetch[x]);
                    if (t < tauL[qi]) tauL[qi] = t;
                }
                if ((iter & 15) == 0)
                    tau_fetch[x] = __hip_atomic_load(&cx.tau_g[cx.qblock * NQ + qi], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (!worked) {
            __builtin_amdgcn_s_sleep(BMX_PSLEEP);
            st.count(Stamps::IDLE);
        }
    }
    stamps_out_service(st, lane);
}

// =====================================================================================================================
// consumer
// =====================================================================================================================
__device__ __forceinline__ void lane0_store(int* word, const int val) {
    // EXEC is all ones here (uniform control flow), so it is narrowed and restored with two scalar moves instead of
    // a compare / saveexec / branch sequence
    const lds_iptr dp = (lds_iptr)word;
    asm volatile("s_mov_b64 exec, 1\n\tds_write_b32 %0, %1\n\ts_mov_b64 exec, -1" ::"v"(dp), "v"(val) : "memory");
}

// The sample pass ends in registers: the query's starting threshold from the 2 x KS / 2 candidates its two lanes hold.
template <int NS, int KS>
__device__ __forceinline__ void sample_epilogue(const PassCtx<NS, KS>& cx, const float (&best)[KS / 2]) {
    const int lane = cx.lane, h = lane >> 5, nrng = cx.nrng, kq = cx.kq;
    const int q = cx.qblock * NQ + cx.wave * 32 + (lane & 31);
    const float* const margin_g = cx.margin_g;
    uint32_t* const tau_g = cx.tau_g;
    const uint32_t mine = f32_orderable(best[KS / 2 - 1]), other = __shfl_xor(mine, 32);
    uint32_t start = max(mine, other);
    if constexpr (KS / 2 <= 24) {
        if (margin_g && kq >= 1 && kq <= KS) {
            // the margin form (see compact_list): the k-th smallest of the 2 x KS / 2 values the query's two lanes hold --
            // distinct references, so k references lie at or below it -- plus twice the error bound.  Each entry's
            // rank in the union = its place in its own (sorted) list + the partner's entries in front of it.
            float part[KS / 2];
#pragma unroll
            for (int e = 0; e < KS / 2; ++e) part[e] = __shfl_xor(best[e], 32);
            float uk = __builtin_inff();
#pragma unroll
            for (int i = 0; i < KS / 2; ++i) {
                int r = i;
#pragma unroll
                for (int e = 0; e < KS / 2; ++e) r += (part[e] < best[i] || (part[e] == best[i] && h == 1)) ? 1 : 0;
                uk = r == kq - 1 ? best[i] : uk;
            }
            uk = fminf(uk, __shfl_xor(uk, 32));
            const float tm = uk + margin_g[q] + fabsf(uk) * 2.384185791015625e-07f;  // (the f32 sum rounded up)
            if (tm == tm) start = min(start, f32_orderable(tm));  // (no k-th value yet: inf, nothing changes)
        }
    }
    // (a seeded search: the tighter of the sampled threshold and the seed's, prep wrote the latter's image)
    // A sample split into ranges (few query blocks, see knn_plan.hpp): every range's threshold is valid by itself -- k of ITS
    // references lie at or below it -- so the tightest of them is; prep has written the seed (or +inf) there.
    // Round 6: the ranges also leave their lists (cand_v is free in a sample pass: [query][range][2 x KS / 2] values, all
    // of distinct references), and sample_merge_kernel takes the k-th smallest of their UNION -- what the unsplit sample
    // arrives at, so that splitting costs the full pass nothing (the tightest single range, round 5, left it 10 % looser).
    if (h == 0) {
        if (nrng > 1) atomicMin(&tau_g[q], start);
        else tau_g[q] = cx.tau_seed ? min(start, cx.tau_seed[q]) : start;
    }
    if (nrng > 1 && cx.cand_v) {
        float* dst = cx.cand_v + ((int64_t)q * nrng + cx.rng) * KS + h * (KS / 2);
#pragma unroll
        for (int e = 0; e < KS / 2; e += 4)
            *reinterpret_cast<f32x4*>(dst + e) = f32x4{best[e], best[e + 1], best[e + 2], best[e + 3]};
    }
}

// The same for the 16 x 16 blocks: a lane holds KS / 4 candidates of each of its two queries (query half b: best[b KS / 4 ...]),
// the four lanes 16 apart those of one query -- again 4 x KS / 4 distinct references, the same statistic.
template <int NS, int KS>
__device__ __forceinline__ void sample_epilogue_16(const PassCtx<NS, KS>& cx, const float (&best)[KS / 2]) {
    constexpr int KL = KS / 4;
    const int lane = cx.lane, g = lane >> 4, nrng = cx.nrng, kq = cx.kq;
    const float* const margin_g = cx.margin_g;
    uint32_t* const tau_g = cx.tau_g;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int q = cx.qblock * NQ + cx.wave * 32 + 16 * b + (lane & 15);
        uint32_t start = f32_orderable(best[b * KL + KL - 1]);
        start = max(start, __shfl_xor(start, 16));
        start = max(start, __shfl_xor(start, 32));
        if (margin_g && kq >= 1 && kq <= KS) {
            // rank in the union = place in the lane's own (sorted) list + the entries of the three other lanes in front of it
            // (equal values: the lower lane's first)
            int r[KL];
#pragma unroll
            for (int i = 0; i < KL; ++i) r[i] = i;
#pragma unroll
            for (int x = 1; x < 4; ++x) {
                const bool first = (g ^ x) < g;
#pragma unroll
                for (int e = 0; e < KL; ++e) {
                    const float pe = __shfl_xor(best[b * KL + e], 16 * x);
#pragma unroll
                    for (int i = 0; i < KL; ++i) r[i] += (pe < best[b * KL + i] || (pe == best[b * KL + i] && first)) ? 1 : 0;
                }
            }
            float uk = __builtin_inff();
#pragma unroll
            for (int i = 0; i < KL; ++i) uk = r[i] == kq - 1 ? best[b * KL + i] : uk;
            uk = fminf(uk, __shfl_xor(uk, 16));
            uk = fminf(uk, __shfl_xor(uk, 32));
            const float tm = uk + margin_g[q] + fabsf(uk) * 2.384185791015625e-07f;  // (the f32 sum rounded up)
            if (tm == tm) start = min(start, f32_orderable(tm));  // (no k-th value yet: inf, nothing changes)
        }
        if (g == 0) {
            if (nrng > 1) atomicMin(&tau_g[q], start);
            else tau_g[q] = cx.tau_seed ? min(start, cx.tau_seed[q]) : start;
        }
        if (nrng > 1 && cx.cand_v) {
            float* dst = cx.cand_v + ((int64_t)q * nrng + cx.rng) * KS + g * KL;
#pragma unroll
            for (int e = 0; e < KL; e += 4)
                *reinterpret_cast<f32x4*>(dst + e) =
                    f32x4{best[b * KL + e], best[b * KL + e + 1], best[b * KL + e + 2], best[b * KL + e + 3]};
        }
    }
}

// The full pass: everything is in the queue; once the service wave has worked it off, both write final lists out.
template <int NS, int KS>
__device__ __forceinline__ void consumer_epilogue(const PassCtx<NS, KS>& cx, Stamps& st, const int wr) {
    const int wave = cx.wave;
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    lane0_store(&cx.lds.wrL[wave], wr);
    lane0_store(&cx.lds.stL[wave], 2);
    while (__builtin_amdgcn_readfirstlane(lds_load_volatile(&cx.lds.stL[wave])) != 3) __builtin_amdgcn_s_sleep(2);
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    write_final_lists(cx, st, wave, 0, EPI_CONS);
}

// LCAP restates F16Shape<NS, KS>::LCAP: profiles, bmx_engine_knn_kernel and the bench's roofline key on the kernel's name.
//
// MS, the MFMA shape of the consumers' sweep: 0 = v_mfma_f32_32x32x16_f16, one 32 x 32 accumulator per tile, a lane holds 16
// values of ONE query (lane & 31; references 8 u + 4 (lane >> 5) + i of the tile in group u); 1 = v_mfma_f32_16x16x32_f16
// (even NS), four 16 x 16 blocks per tile -- reference half a, query half b, NS / 2 MFMAs each: the same pipe time and as many
// accumulator registers -- and a lane holds values of TWO queries, 16 b + (lane & 15), of each the references
// 16 a + 4 (lane >> 4) + i of both a.  The prepared reference image comes in the fragment order of the shape
// (knn_prep.hip); ring, hand-over, queues, service waves and lists are the same for both.  knn_f16_shape.hpp
// (mfma_shape_for) has which shape runs where.
template <int NS, int KS, int LCAP, bool SAMPLE, int MS>
__global__ __launch_bounds__((F16Shape<NS, KS>::NWAVES * 64)) void knn_topk_f16(
    const uint16_t* __restrict__ Pq, const uint16_t* __restrict__ PrF, int first_begin, int range_len, int r_limit,
    int n_full, int nranges, int out_chunk0, int out_nchunks, uint32_t* __restrict__ tau_g, int32_t* __restrict__ cand,
    float* __restrict__ cand_v, float* __restrict__ tau_out, const float* __restrict__ margin_g, int kq,
    const uint32_t* __restrict__ tau_seed) {
    using S = F16Shape<NS, KS>;
    using Lds = F16Lds<S>;
    constexpr int NSLOT = S::NSLOT, TP = S::TP, SLOT_BYTES = S::SLOT_BYTES, TILE_BYTES = S::TILE_BYTES;
    static_assert(LCAP == list_cap(NS, KS), "LCAP is a restatement of the shape, not an input");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Lds lds = Lds::carve(smem);
    char* const ring = lds.ring;
    float* const qvals = lds.qvals;
    uint32_t* const qtags = lds.qtags;
    float* const tauL = lds.tauL;
    int *const ready = lds.ready, *const done = lds.done, *const wrL = lds.wrL, *const rdL = lds.rdL, *const stL = lds.stL;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: branches on it are scalar
    const WorkItem wi = decode_work_item(first_begin, range_len, r_limit, n_full, nranges);
    const int qblock = wi.qblock, nrng = wi.nrng;
    const int ntiles = (wi.r_end - wi.r_begin) >> 5;  // even: ranges are multiples of 64 rows
    const int nslots = ntiles / (2 * TP);             // (ranges are multiples of 64 TP rows)
    if (tid < Lds::HANDOVER_WORDS) lds.handover()[tid] = 0;
    if (tid < NQ) {
        lds.cnt[tid] = 0;
        tauL[tid] = (!SAMPLE && tau_g) ? orderable_f32(tau_g[qblock * NQ + tid]) : __builtin_inff();
        lds.mgL[tid] = (!SAMPLE && margin_g) ? margin_g[qblock * NQ + tid] : 0.f;
    }
    __syncthreads();
    const bool shared_tau = !SAMPLE && tau_g != nullptr && nrng > 1;
    // what the roles that are functions of their own see of all this
    const PassCtx<NS, KS> cx{lds, lane, wave, qblock, wi.rng, nrng, wi.r_begin, ntiles, nslots, out_chunk0 + wi.rng, out_nchunks,
                             shared_tau, Pq, PrF, tau_g, cand, cand_v, tau_out, margin_g, kq, tau_seed};

    if (wave >= NCONS && wave < NCONS + NPROD) {
        producer_role(cx);
        return;
    }
    if (wave >= NCONS + NPROD) {
        if constexpr (!SAMPLE) service_role<MS>(cx);  // (the sample pass appends to no list: its service waves end here)
        return;
    }

    // ---------------------------------------------------------------------- consumer: one wave's sweep of the ring.  It stays
    // in the kernel's body, its steps always-inline lambdas on the kernel's own locals, as the parent of this split had it: as a
    // function of its own (or a struct of member functions) behind PassCtx the NS = 4 full pass compiled to another block layout
    // and measured 0.8 % slower (MEASUREMENTS.md).
    static_assert(MS == 0 || (MS == 1 && NS % 2 == 0), "the K of 32 of the 16 x 16 blocks: whole pairs of k-steps");
    Stamps st;
    constexpr int QL = MS == 0 ? 1 : 2;   // queries a lane holds values of: j, and with the 16 x 16 blocks 16 + j too
    constexpr int QW = MS == 0 ? 32 : 16;  // lanes that share a set of columns
    const int j = lane & (QW - 1), h = lane >> (MS == 0 ? 5 : 4);
    const int q = qblock * NQ + wave * 32 + j;

    float tau[QL];
#pragma unroll
    for (int b = 0; b < QL; ++b) tau[b] = tauL[wave * 32 + 16 * b + j];

    // the query image is row-major: lane part h holds the h-th of a row's 64 / QW stretches of columns, the fragment of k-step
    // s is 8 columns of it (the reference image follows the same column order).  MS = 1: bq[b NS / 2 + ks] of query half b
    f16x8 bq[NS];
#pragma unroll
    for (int b = 0; b < QL; ++b) {
        const f32x4* src =
            reinterpret_cast<const f32x4*>(Pq + (int64_t)(q + 16 * b) * (16 * NS) + h * (8 * NS / QL));
#pragma unroll
        for (int s = 0; s < NS / QL; ++s) bq[b * (NS / QL) + s] = __builtin_bit_cast(f16x8, src[s]);
    }

    float* qv = qvals + wave * QCAP * 4;
    uint32_t* qt = qtags + wave * QCAP;
    int wr = 0;       // records pushed so far (wave-uniform)
    int rd_seen = 0;  // what the service wave had worked off when last looked at
    st.begin();

    // Hand-over, once per slot (two tiles).  While the tiles of slot sl compute, their fragment registers are refilled
    // from slot sl + 1 (each register right after the MFMA that consumed it); the ready word of slot sl + 1 is checked
    // before the first refill (it was polled a slot earlier: no LDS round trip in steady state), and after the last
    // refill the wave adds one to the position's hand-back counter -- queued behind the reads in the wave's in-order
    // LDS queue, so the producers cannot overwrite them early -- and polls the ready word of slot sl + 2 and its
    // queries' thresholds as the service wave has them now.  The slot loop is unrolled over the ring positions, so
    // every address below is a register set up once plus a constant.
    lds_iptr done_p[NSLOT], ready_p[NSLOT];
#pragma unroll
    for (int k = 0; k < NSLOT; ++k) {
        done_p[k] = (lds_iptr)&done[k];
        ready_p[k] = (lds_iptr)&ready[k];
        asm volatile("" : "+v"(done_p[k]), "+v"(ready_p[k]));
    }
    lds_iptr wr_p = (lds_iptr)&wrL[wave];
    int one = 1;
    asm volatile("" : "+v"(wr_p), "+v"(one));
    float tau_next[QL];
#pragma unroll
    for (int b = 0; b < QL; ++b) tau_next[b] = tau[b];
    int seen = 0;
    f32x4 a[NS], b[NS];  // fragments of the even / odd tile of the current slot
    // SAMPLE: the lane's KS / 2 smallest candidates, ascending.  Insertion of x into a sorted list is one median per
    // entry, best'[i] = med3(best[i - 1], best[i], x), all of them independent when taken from the top down
    float best[SAMPLE ? KS / 2 : 1];
#pragma unroll
    for (int i = 0; i < (SAMPLE ? KS / 2 : 1); ++i) best[i] = __builtin_inff();

    auto spin_until_staged = [&](const int slot, const int k) __attribute__((always_inline)) {  // slot, at position k
        if (__builtin_amdgcn_readfirstlane(seen) < slot + 1) {
            const unsigned long long s0 = st.now();
            do {
                __builtin_amdgcn_s_sleep(1);
                seen = *(volatile lds_iptr)ready_p[k];
            } while (seen < slot + 1);
            st.since(Stamps::SPIN, s0);
        }
    };
    auto hand_back = [&](const int k) __attribute__((always_inline)) {  // the slot at position k has been read
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        if constexpr (SAMPLE) {
            asm volatile("s_mov_b64 exec, 1\n\tds_add_u32 %0, %1\n\ts_mov_b64 exec, -1" ::"v"(done_p[k]), "v"(one) : "memory");
        } else {
            // ... and, in the same breath, the number of records pushed so far (they sit behind the records in the wave's
            // in-order LDS queue): one store per slot instead of one per spill
            asm volatile("s_mov_b64 exec, 1\n\tds_add_u32 %0, %1\n\tds_write_b32 %2, %3\n\ts_mov_b64 exec, -1" ::"v"(done_p[k]),
                         "v"(one), "v"(wr_p), "v"(wr)
                         : "memory");
        }
    };
    // the ready word of the slot after next and the thresholds: polled ahead of the slot's fragment reads, looked at
    // one slot later (they are back long before the reads the wave has to wait for anyway)
    auto poll = [&](const int k) __attribute__((always_inline)) {
        seen = *(volatile lds_iptr)ready_p[k];
        if constexpr (!SAMPLE) {
#pragma unroll
            for (int b = 0; b < QL; ++b)
                tau_next[b] = __hip_atomic_load(&tauL[wave * 32 + 16 * b + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    };
    // (the list of query half b: best[b KL ...], KL = KS / 2 / QL entries)
    auto sample_insert = [&](const int b, const float x) __attribute__((always_inline)) {
        constexpr int KL = SAMPLE ? KS / 2 / QL : 1;
#pragma unroll
        for (int i = KL - 1; i > 0; --i) best[b * KL + i] = __builtin_amdgcn_fmed3f(best[b * KL + i - 1], best[b * KL + i], x);
        best[b * KL] = fminf(fminf(best[b * KL], x), x);
    };

    // room for `need` (<= QCAP) more records: the service wave's progress is looked at only when the last known state
    // does not leave enough
    auto wait_room = [&](const int need) __attribute__((always_inline)) {
        const unsigned long long w0 = st.now();
        rd_seen = __builtin_amdgcn_readfirstlane(lds_load_volatile(&rdL[wave]));
        if (wr + need - rd_seen > QCAP) {
            lane0_store(&wrL[wave], wr);
            lane0_store(&stL[wave], 1);  // "waiting": the service wave works the queue off whatever its length
            do {
                __builtin_amdgcn_s_sleep(1);
                rd_seen = __builtin_amdgcn_readfirstlane(lds_load_volatile(&rdL[wave]));
            } while (wr + need - rd_seen > QCAP);
            lane0_store(&stL[wave], 0);
        }
        st.since(Stamps::QWAIT, w0);
    };

    // ---- filter of one tile (products in `acc`, tile number t) and, where a value is below its query's threshold, the
    // spill.  Leaves the lane minimum of each of the lane's queries in mn (SAMPLE uses nothing else).  The tile's values come
    // as four groups of four consecutive references: MS = 0, one 32 x 32 accumulator, group u = its registers 4 u ..., all of
    // one query; MS = 1, four 16 x 16 blocks, group u = 2 a + b = the block of reference half a and query half b.
    auto sift = [&](const auto& acc, const int t, float(&mn)[QL]) __attribute__((always_inline)) {
        auto at = [&](const int u, const int i) __attribute__((always_inline)) {
            if constexpr (MS == 0)
                return acc[4 * u + i];
            else
                return acc[u][i];
        };
        // group minima, then the lane minimum of a query.  Every fminf below is half of a
        // three-way minimum: the compiler forms v_min3_f32 from such pairs and, unlike for a lone v_min_f32, does not put
        // a v_max x, x (signalling-NaN quieting) in front of its inputs.  The threshold rides along as the sixth operand
        // of a group: min(group, tau) < tau iff min(group) < tau (SAMPLE: tau = +inf, the plain minimum)
        float g[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float m3 = fminf(fminf(at(u, 0), at(u, 1)), at(u, 2));
            g[u] = fminf(fminf(m3, at(u, 3)), tau[u & (QL - 1)]);
        }
        if constexpr (MS == 0) {
            mn[0] = fminf(fminf(fminf(fminf(g[0], g[1]), g[2]), g[3]), tau[0]);
        } else {
#pragma unroll
            for (int b = 0; b < QL; ++b) mn[b] = fminf(fminf(g[b], g[2 + b]), tau[b]);
        }
        if constexpr (SAMPLE) {
            return;
        } else {
            bool below = mn[0] < tau[0];
            if constexpr (QL == 2) below |= mn[1] < tau[1];
            const unsigned long long any = __builtin_amdgcn_ballot_w64(below);
            if (any == 0) return;
            st.count(Stamps::EVT);
            const unsigned long long e0 = st.now();
            // ---- spill the groups with survivors: four raw values and a tag per (lane, group) into the wave's queue;
            // the service wave takes it from there.  (A lambda: it lives on sift's g[] and on the wave's tau and wr.)
            const uint32_t tagbase = ((uint32_t)t << 8) | (uint32_t)lane;
            auto spill = [&](const int u, const unsigned long long m) __attribute__((always_inline)) {
                if (g[u] < tau[u & (QL - 1)]) {  // the lanes of m
                    const int slot = (wr + mbcnt64(m)) & (QCAP - 1);
                    f32x4 rec;
                    rec[0] = at(u, 0);
                    rec[1] = at(u, 1);
                    rec[2] = at(u, 2);
                    rec[3] = at(u, 3);
                    *reinterpret_cast<f32x4*>(qv + slot * 4) = rec;
                    qt[slot] = tagbase | ((uint32_t)u << 6);
                }
                wr += __builtin_popcountll(m);
                st.count(Stamps::GRP);
            };
            unsigned long long m[4];
            int tot = 0;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                m[u] = __builtin_amdgcn_ballot_w64(g[u] < tau[u & (QL - 1)]);
                tot += __builtin_popcountll(m[u]);
            }
            if (wr + tot - rd_seen > QCAP) {
                if (tot > QCAP) {
                    // the first tiles of a sweep that starts without a threshold: one group (<= 64 records) at a time,
                    // each against the threshold as it stands once there is room for it
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        // (taken again: an earlier group of this tile may have waited and come back with a lower threshold)
                        unsigned long long mu = __builtin_amdgcn_ballot_w64(g[u] < tau[u & (QL - 1)]);
                        if (mu == 0) continue;
                        const int c = __builtin_popcountll(mu);
                        if (wr + c - rd_seen > QCAP) {
                            wait_room(c);
#pragma unroll
                            for (int b = 0; b < QL; ++b) {
                                const float tl = __hip_atomic_load(&tauL[wave * 32 + 16 * b + j], __ATOMIC_RELAXED,
                                                                   __HIP_MEMORY_SCOPE_WORKGROUP);
                                tau[b] = tl < tau[b] ? tl : tau[b];
                            }
                            mu = __builtin_amdgcn_ballot_w64(g[u] < tau[u & (QL - 1)]);
                        }
                        if (mu) {
                            spill(u, mu);
                            __atomic_signal_fence(__ATOMIC_SEQ_CST);
                            lane0_store(&wrL[wave], wr);
                        }
                    }
                    st.since(Stamps::EVC, e0);
                    return;
                }
                wait_room(tot);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) spill(u, m[u]);  // (the count goes out with the next done word)
            st.since(Stamps::EVC, e0);
        }
    };

    // One iteration = one pair of tiles.  Matrix phase: the two tiles' MFMA chains interleaved (independent
    // accumulators: the wave issues its 2 NS MFMAs back to back without waiting on its own results), each fragment
    // register refilled from the next pair right after the MFMA that consumed it.  Vector phase: filter and spill of
    // both tiles.  The two consumer waves of a SIMD fall into opposite phases: one's vector phase runs under the
    // other's MFMAs.  With slots of four tiles (TP = 2) only every other pair crosses a slot boundary: the ready
    // check, the polls and the hand-back happen once per four tiles.
    // MS = 1: fragment f = 2 ks + a of a tile is reference half a in k-step ks (of 32); it feeds the blocks of both query
    // halves and is refilled after the second; the eight blocks of the pair are eight independent chains.
    auto tile_pair = [&](const lds_f4ptr tp, const int t0, const int hand_back_pos) __attribute__((always_inline)) {
        float mnA[QL], mnB[QL];
        if constexpr (MS == 0) {
            f32x16 accA, accB;
#pragma unroll
            for (int e = 0; e < 16; ++e) accA[e] = accB[e] = 0.f;
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                accA = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a[s]), bq[s], accA, 0, 0, 0);
                a[s] = tp[s * 64];
                accB = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, b[s]), bq[s], accB, 0, 0, 0);
                b[s] = tp[(NS + s) * 64];
            }
#pragma unroll
            for (int s = 0; s < 2 * NS; ++s) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // one MFMA
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // one LDS read
            }
            __builtin_amdgcn_sched_barrier(0);
            if (hand_back_pos >= 0) hand_back(hand_back_pos);  // that slot's tiles are all on their way into registers
            sift(accA, t0, mnA);
            sift(accB, t0 + 1, mnB);
        } else {
            f32x4 cA[4], cB[4];  // block 2 a + b
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e) cA[u][e] = cB[u][e] = 0.f;
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int f = 0; f < NS; ++f) {
                const int ks = f >> 1, u0 = 2 * (f & 1);
                const f16x8 fa = __builtin_bit_cast(f16x8, a[f]), fb = __builtin_bit_cast(f16x8, b[f]);
                cA[u0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa, bq[ks], cA[u0], 0, 0, 0);
                cA[u0 + 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa, bq[NS / 2 + ks], cA[u0 + 1], 0, 0, 0);
                a[f] = tp[f * 64];
                cB[u0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb, bq[ks], cB[u0], 0, 0, 0);
                cB[u0 + 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb, bq[NS / 2 + ks], cB[u0 + 1], 0, 0, 0);
                b[f] = tp[(NS + f) * 64];
            }
#pragma unroll
            for (int s = 0; s < 2 * NS; ++s) {
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);  // two MFMAs: a fragment's two blocks
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // one LDS read
            }
            __builtin_amdgcn_sched_barrier(0);
            if (hand_back_pos >= 0) hand_back(hand_back_pos);
            sift(cA, t0, mnA);
            sift(cB, t0 + 1, mnB);
        }
        if constexpr (SAMPLE) {
            // sorted insertion of ONE candidate per pair and query: the lane's minimum over both tiles (32 references of the
            // query, 16 with the 16 x 16 blocks; still one distinct reference per candidate, half the insertions)
#pragma unroll
            for (int qb = 0; qb < QL; ++qb) sample_insert(qb, fminf(fminf(mnA[qb], mnB[qb]), mnB[qb]));
        }
    };

    auto sweep = [&]() __attribute__((always_inline)) {
        // at equal priority the second-dispatched half of the consumers (waves 4..7, one per SIMD) loses every contested
        // issue slot to its older partner: it gets the higher static priority (MI355X_MICROARCH.md, two waves per SIMD)
        if (wave >= NCONS / 2)
            __builtin_amdgcn_s_setprio(BMX_CPRIO_HI);
        else
            __builtin_amdgcn_s_setprio(BMX_CPRIO_LO);
        // the query fragments have arrived: said here once, so that the compiler keeps no vmcnt wait for them in the loop
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
        if (nslots > 0) {
            lds_cptr ring_lane = (lds_cptr)ring + lane * 16;
            asm volatile("" : "+v"(ring_lane));
            spin_until_staged(0, 0);
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            {
                const lds_f4ptr tp = (lds_f4ptr)ring_lane;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    a[s] = tp[s * 64];
                    b[s] = tp[(NS + s) * 64];
                }
            }
            if constexpr (TP == 1) hand_back(0);  // (a slot of four tiles is handed back once its second half has been read)
            poll(1 % NSLOT);
            for (int sl0 = 0; sl0 < nslots; sl0 += NSLOT) {
#pragma unroll
                for (int k = 0; k < NSLOT; ++k) {
                    const int sl = sl0 + k;  // its (first) fragments are in a[], b[]; slot sl + 1 sits at position kn
                    if (sl >= nslots) break;
                    const int kn = (k + 1) % NSLOT;
                    if constexpr (TP == 2) {
                        // first pair of the slot: refill from the slot's own second half, then the slot is read
                        __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this pair's fragments
                        tile_pair((lds_f4ptr)(ring_lane + k * SLOT_BYTES + 2 * TILE_BYTES), 4 * sl, k);
                    }
                    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this pair's fragments, the next slot's ready word, tau
                    if constexpr (!SAMPLE) {
#pragma unroll
                        for (int b = 0; b < QL; ++b) asm("v_min_f32 %0, %0, %1" : "+v"(tau[b]) : "v"(tau_next[b]));
                    }
                    spin_until_staged(sl + 1, kn);
                    __atomic_signal_fence(__ATOMIC_SEQ_CST);
                    poll((kn + 1) % NSLOT);
                    tile_pair((lds_f4ptr)(ring_lane + kn * SLOT_BYTES), 2 * TP * sl + 2 * (TP - 1), TP == 1 ? kn : -1);
                }
            }
        }
        __builtin_amdgcn_s_setprio(0);
    };
    sweep();
    st.sweep_end();
    if constexpr (!SAMPLE)
        consumer_epilogue(cx, st, wr);
    else if constexpr (MS == 0)
        sample_epilogue(cx, best);
    else
        sample_epilogue_16(cx, best);
    stamps_out_consumer<SAMPLE>(st, lane, wave, ntiles);
}

template <int NS, int KS, int MS>
void launch(hipStream_t stream, KnnWorkspace& ws, const PassLaunch& L) {
    using S = F16Shape<NS, KS>;
    constexpr size_t lds = S::lds_bytes;
    static_assert(lds <= LDS_TOTAL, "LDS budget");
    const auto full = &knn_topk_f16<NS, KS, S::LCAP, false, MS>, sample = &knn_topk_f16<NS, KS, S::LCAP, true, MS>;
    ensure_dynamic_lds(reinterpret_cast<const void*>(full), lds);
    ensure_dynamic_lds(reinterpret_cast<const void*>(sample), lds);
    std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
    if (ws.profile) {
        ev = ws.next_events(L.sample ? 0 : 1);
        BMX_HIP(hipEventRecord(ev.first, stream));
    }
    if (!L.sample) ws.last_mfma_shape = MS;
    if (!L.sample)
        ws.last_kernel = "knn_topk_f16<" + std::to_string(NS) + ", " + std::to_string(KS) + ", " + std::to_string(S::LCAP) +
                         ", false, " + std::to_string(MS) + ">";
    const int items = L.n_full + (L.nqb - L.n_full) * L.nranges;
    const auto pass = L.sample ? sample : full;
    hipLaunchKernelGGL(pass, dim3(items), dim3(S::NWAVES * 64), lds, stream, L.pq, L.pr, L.first_begin, L.range_len, L.r_limit,
                       L.n_full, L.nranges, L.out_chunk0, L.out_nchunks, L.tau_g, L.cand, L.cand_v, L.tau, L.margin, L.k,
                       L.sample ? L.tau_seed : (const uint32_t*)nullptr);
    BMX_LAUNCH_CHECK();
    if (ws.profile) BMX_HIP(hipEventRecord(ev.second, stream));
#ifdef BMX_STAMPS
    {
        if (L.sample) fprintf(stderr, "(sample pass) ");
        unsigned long long hh[48];
        BMX_HIP(hipStreamSynchronize(stream));
        BMX_HIP(hipMemcpyFromSymbol(hh, HIP_SYMBOL(bmx_dbg16), sizeof(hh)));
        const double nt = (double)hh[8];
        const double sw = hh[14] ? (double)hh[14] : 1.0;
        fprintf(stderr,
                "[stamps f16] consumers=%.0f tiles/wave=%.0f cyc/tile=%.0f spin/tile=%.0f evpath/tile=%.0f qwait/tile=%.0f "
                "event tiles=%.3f groups/tile=%.3f | service waves=%.0f cyc=%.0f drain=%.0f (%.0f passes, %.0f cyc each) "
                "compact=%.0f (%.0f calls, %.1f rounds each) idle polls=%.0f\n",
                (double)hh[9], nt / hh[9], hh[0] / nt, hh[1] / nt, hh[10] / nt, hh[12] / nt, hh[6] / nt, hh[7] / nt,
                (double)hh[14], hh[13] / sw, hh[2] / sw, hh[3] / sw, hh[3] ? (double)hh[2] / hh[3] : 0.0, hh[5] / sw,
                hh[4] / sw, hh[4] ? (double)hh[11] / hh[4] : 0.0, hh[15] / sw);
        unsigned long long z[48] = {0};
        BMX_HIP(hipMemcpyToSymbol(HIP_SYMBOL(bmx_dbg16), z, sizeof(z)));
        // the clock the sweeps ran at: cycles / 100 MHz ticks of the first consumer of every workgroup, the median of them
        std::vector<unsigned long long> ck(2 * CLK_WGS);
        BMX_HIP(hipMemcpyFromSymbol(ck.data(), HIP_SYMBOL(bmx_clk16), ck.size() * sizeof(unsigned long long)));
        std::vector<double> ghz;
        for (int w = 0; w < std::min(items, CLK_WGS); ++w)
            if (ck[2 * w + 1] > 0) ghz.push_back((double)ck[2 * w] / (double)ck[2 * w + 1] * 0.1);
        if (!ghz.empty()) {
            std::sort(ghz.begin(), ghz.end());
            fprintf(stderr, "[stamps f16] shape %d in-kernel clock: median %.3f GHz (min %.3f, max %.3f) over %zu workgroups\n", MS,
                    ghz[ghz.size() / 2], ghz.front(), ghz.back(), ghz.size());
        }
    }
#endif
}

// The split sample's thresholds (see sample_epilogue): one wave per query, n = nranges x KS values of
// distinct references; the k-th smallest of them -- every value's rank by counting, ties by position -- plus twice the pass's
// error bound is a valid starting threshold (the margin form of the unsplit sample), taken if tighter than what stands there.
__global__ __launch_bounds__(256) void sample_merge_kernel(const float* __restrict__ lists, int n, int nq, int k,
                                                           const float* __restrict__ margin_g, uint32_t* __restrict__ tau_g) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + w;
    if (q >= nq) return;  // (whole waves: nothing below synchronises the block)
    // the k-th smallest of the n <= 512 values (the ranges' lists, in any order): a lane holds up to eight of them as orderable
    // bit patterns, a bisection over the 32 bits counts with ballots -- no LDS, no dependent look-ups.  (Until late in round 6:
    // every entry's rank by a binary search in every other list, 36 dependent LDS reads an entry: 44 us a launch at 12 500 queries.)
    uint32_t val[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int i = lane + 64 * u;
        val[u] = i < n ? f32_orderable(lists[(int64_t)q * n + i]) : 0xFFFFFFFFu;
    }
    uint32_t t = 0;  // the smallest pattern with at least k values at or below it
    for (int b = 31; b >= 0; --b) {
        const uint32_t trial = t | ((1u << b) - 1u);  // the largest pattern with the bits decided so far and this bit clear
        int c = 0;
#pragma unroll
        for (int u = 0; u < 8; ++u) c += __popcll(__builtin_amdgcn_ballot_w64(val[u] <= trial));
        if (c < k) t |= 1u << b;
    }
    if (lane == 0) {
        const float uk = orderable_f32(t);
        const float tm = uk + margin_g[q] + fabsf(uk) * 2.384185791015625e-07f;  // (the f32 sum rounded up)
        if (tm == tm && tm < __builtin_inff()) atomicMin(&tau_g[q], f32_orderable(tm));
    }
}
}  // namespace

void f16_sample_merge(hipStream_t stream, const float* lists, int nranges, int KS, int nq, int k, const float* margin,
                      uint32_t* tau_g) {
    const int n = nranges * KS;
    if (n > 512 || nq <= 0 || k < 1 || k > n || !margin) return;  // (the ranges' own thresholds stand)
    hipLaunchKernelGGL(sample_merge_kernel, dim3(cdiv(nq, 4)), dim3(256), 0, stream, lists, n, nq, k, margin, tau_g);
    BMX_LAUNCH_CHECK();
}

// MFMA k-steps (16 fp16 each) for d + 3 columns; 0 = this tier does not take the shape
int f16_pick_ns(int d, int KS) {
    const int ns = (d + 3 + 15) / 16;
    if (KS == BMX_KS1) return ns <= 8 ? ns : 0;
    if (KS == 48) return ns <= 4 ? ns : 0;
    return 0;
}

// The MFMA shape of a search's sweeps (knn_topk_f16's MS): the table of knn_f16_shape.hpp, or what the testing hook forces;
// the 16 x 16 blocks exist for even NS only.  The prepared reference image is written for the shape (f16_prep_all).
int f16_pick_shape(int NS, int KS) {
    if (NS % 2 != 0) return 0;
    const int forced = dev_knobs().mfma_shape;
    return forced == 0 || forced == 1 ? forced : mfma_shape_for(NS, KS);
}

namespace {
template <int NS, int KS>
void launch_shape(hipStream_t stream, KnnWorkspace& ws, const PassLaunch& L) {
    if constexpr (NS % 2 == 0) {
        if (L.shape == 1) {
            launch<NS, KS, 1>(stream, ws, L);
            return;
        }
    }
    launch<NS, KS, 0>(stream, ws, L);
}
}  // namespace

bool f16_launch(hipStream_t stream, KnnWorkspace& ws, int NS, int KS, const PassLaunch& L) {
    if (L.shape != 0 && (L.shape != 1 || NS % 2 != 0)) return false;
#define BMX_CASE(N)                       \
    case N:                               \
        if (KS == BMX_KS1)                \
            launch_shape<N, BMX_KS1>(stream, ws, L); \
        else if constexpr (N <= 4)        \
            launch_shape<N, 48>(stream, ws, L); \
        else                              \
            return false;                 \
        return true;
    switch (NS) {
        BMX_CASE(1)
        BMX_CASE(2)
        BMX_CASE(3)
        BMX_CASE(4)
        BMX_CASE(5)
        BMX_CASE(6)
        BMX_CASE(7)
        BMX_CASE(8)
        default:
            return false;
    }
#undef BMX_CASE
}

int f16_rows_per_slot(int NS, int KS) { return 64 * tile_pairs_for(NS, KS); }

}  // namespace bmx
