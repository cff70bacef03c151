// Split-bf16 candidate pass for the exact kNN (MI355X / gfx950).
//
// The f32-input MFMA runs at 1/16 of the bf16 rate, and the candidate pass only has to be accurate enough for the
// FP64 certificate of knn_refine to hold.  So the f32 operands are split into bf16 pieces,
//     r = rh + rl (+ 2^-16),   q' = -2q = qh + ql (+ 2^-16),
// and ONE v_mfma_f32_32x32x16_bf16 chain over the concatenated K = [qh|qh|ql|1 1 1] . [rh|rl|rh|n1 n2 n3] yields
//     v = |r|^2 + qh.rh + qh.rl + ql.rh        (|r|^2 as three bf16 pieces: exact to 2^-24)
// with |v - (|r|^2 - 2 q.r)| <= 3.03 * 2^-16 * 2 |q||r| + f32 accumulation error -- the bound knn_refine certifies
// against.  10 MFMAs of 32 cycles per 32x32 tile at 50 PCs instead of 28 of 64 cycles.  (The prepared images: knn_prep.hip.)
//
// At that rate the matrix pipe is no longer the limit; staging and selection are.  Structure of a workgroup
// (knn_bf16_shape.hpp has its numbers and its LDS layout):
//   * NCONS consumer waves, 32 queries each: query fragments resident in VGPRs; per query a sorted kept list and two
//     lane-private pending lists in the LDS, their lengths and the working threshold in registers (knn_select.hpp);
//   * NPROD producer waves stream the reference tiles (fragment-major, 1 KiB coalesced reads, two or three tiles in
//     flight per producer) into an LDS ring (as many slots as the LDS left by the lists holds) shared by all
//     consumers -- one read of the reference set per 32*NCONS queries;
//   * no s_barrier in the main loop: slots are handed over through LDS words (ready[slot] = tile number + 1, one
//     done word per slot and consumer), which the in-order LDS queue of each wave makes safe without extra waits.
//     A consumer that is busy merging a candidate list therefore delays nobody until the ring runs dry;
//   * the consumer loop is software-pipelined: under the dependent MFMA chain of tile t the wave refills its
//     fragment registers with tile t + 1 and filters tile t - 1; appends and list merges of tile t - 1 follow.
// The kernel by role: producer_role and write_final_lists are functions of the pass's context; the consumers' sweep is the
// kernel's body, as lambdas on its locals (MEASUREMENTS.md, "What stayed inline", has why).
#include "knn_bf16_shape.hpp"
#include "knn_tier.hpp"

#include <cmath>

namespace bmx {
namespace {

using namespace sel;
using namespace bf16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) const char* lds_cptr;
typedef __attribute__((address_space(3))) const f32x4* lds_f4ptr;

// What the roles of a workgroup share: where its LDS regions lie, who the wave is, the work item.  The roles take it BY VALUE:
// taken by reference the producers' tile addresses compile to other code than they do in the kernel's body (one base and
// immediate offsets instead of an address a fragment; up to two registers more at NS = 13 and 19), by value to the same.  The
// pass's buffers go to the roles as parameters of their own, __restrict__ as the kernel's.
template <int NS, int KS>
struct PassCtx {
    using S = Bf16Shape<NS, KS>;
    Bf16Lds<S> lds;
    int lane, wave;           // (wave: wave-uniform, branches on it are scalar)
    int qblock, nrng;         // the work item (knn_tier.hpp): its query block, the ranges the block is split into
    int r_begin, ntiles;      // ... its reference range: first row, 32-row tiles
    int out_chunk, out_nchunks;  // the list column this item writes, of how many
};

// ---- the cycle stamps of the developer build leave the kernel here (make STAMPS=1; launch() prints them)
#ifdef BMX_STAMPS
__device__ unsigned long long bmx_dbg[48];
__device__ __forceinline__ void stamps_out_producer(const Stamps& st, const int lane, const int p) {
    if (lane == 0) {
        atomicAdd(&bmx_dbg[32 + p], st.get(Stamps::PWAIT));
        atomicAdd(&bmx_dbg[36 + p], st.elapsed());
    }
}
__device__ __forceinline__ void stamps_out_consumer(const Stamps& st, const int lane, const int wave, const int ntiles) {
    if (lane == 0) {
        atomicAdd(&bmx_dbg[0], st.elapsed());
        atomicAdd(&bmx_dbg[1], st.get(Stamps::SPIN));
        atomicAdd(&bmx_dbg[2], st.get(Stamps::COMP));
        atomicAdd(&bmx_dbg[3], st.get(Stamps::NSPIN));
        atomicAdd(&bmx_dbg[4], st.get(Stamps::NFLUSH));
        atomicAdd(&bmx_dbg[5], st.get(Stamps::NCOMP));
        atomicAdd(&bmx_dbg[6], st.get(Stamps::EVT));
        atomicAdd(&bmx_dbg[7], st.get(Stamps::GRP));
        atomicAdd(&bmx_dbg[8], (unsigned long long)ntiles);
        atomicAdd(&bmx_dbg[9], 1ull);
        atomicAdd(&bmx_dbg[10], st.get(Stamps::EVC));
        atomicAdd(&bmx_dbg[16 + wave], st.get(Stamps::SPIN));
        atomicAdd(&bmx_dbg[24 + wave], st.get(Stamps::COMP));
    }
}
#else
__device__ __forceinline__ void stamps_out_producer(const Stamps&, const int, const int) {}
__device__ __forceinline__ void stamps_out_consumer(const Stamps&, const int, const int, const int) {}
#endif

// =====================================================================================================================
// producer waves: reference tiles from global memory into the ring
// =====================================================================================================================
template <int NS, int KS, bool SAMPLE>
__device__ __forceinline__ void producer_role(const PassCtx<NS, KS> cx, const uint16_t* __restrict__ PrF) {
    using S = Bf16Shape<NS, KS>;
    constexpr int NCONS = S::NCONS, NPROD = S::NPROD, NSLOT = S::NSLOT, TILE_BYTES = S::TILE_BYTES;
    const int lane = cx.lane, ntiles = cx.ntiles;
    int* const ready = cx.lds.ready;
    int* const done = cx.lds.done;
    const int p = cx.wave - NCONS;
    Stamps st;
    st.begin();
    f32x4 ra[NS], rb[NS];
    const f32x4* src = reinterpret_cast<const f32x4*>(PrF) + ((int64_t)(cx.r_begin >> 5) * NS) * 64 + lane;
    f32x4* ring_l = reinterpret_cast<f32x4*>(cx.lds.ring) + lane;
    auto load = [&](f32x4(&r)[NS], int t) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < NS; ++s) r[s] = src[((int64_t)t * NS + s) * 64];
    };
    // tile t goes to slot t % NSLOT once every consumer has read the tile staged there NSLOT tiles earlier (that
    // tile may have come from another producer: the consumers' done words order the two).  done[slot][c] is the
    // number of the last tile consumer c has read from the slot, plus one.
    auto wait_free = [&](int t, int slot) __attribute__((always_inline)) {
        if (t < NSLOT) return;
        const int need = t - NSLOT + 1;
        const auto s0 = st.now();
        for (;;) {
            const int v = lane < NCONS ? lds_load_volatile(&done[slot * NCONS + lane]) : need;
            if (__builtin_amdgcn_ballot_w64(v < need) == 0) break;
            __builtin_amdgcn_s_sleep(1);
        }
        st.since(Stamps::PWAIT, s0);
    };
    auto publish = [&](const f32x4(&r)[NS], int t) __attribute__((always_inline)) {
        const int slot = t % NSLOT;
        wait_free(t, slot);
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        f32x4* dst = ring_l + slot * (TILE_BYTES / 16);
#pragma unroll
        for (int s = 0; s < NS; ++s) dst[s * 64] = r[s];
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        // same wave, in-order LDS queue: the flag lands after the tile
        if (lane == 0) __hip_atomic_store(&ready[slot], t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    // three register sets: the loads of tiles t + 4 and t + 8 are in flight while tile t is handed over
    f32x4 rc[NS];
    int t = p;
    if (t < ntiles) load(ra, t);
    if (t + NPROD < ntiles) load(rb, t + NPROD);
    for (; t < ntiles; t += 3 * NPROD) {
        if (t + 2 * NPROD < ntiles) load(rc, t + 2 * NPROD);
        publish(ra, t);
        if (t + NPROD < ntiles) {
            if (t + 3 * NPROD < ntiles) load(ra, t + 3 * NPROD);
            publish(rb, t + NPROD);
        }
        if (t + 2 * NPROD < ntiles) {
            if (t + 4 * NPROD < ntiles) load(rb, t + 4 * NPROD);
            publish(rc, t + 2 * NPROD);
        }
    }
    // two empty tiles past the end: the consumers' loop runs one tile longer than the data (the selection of a
    // tile happens under the MFMAs of the next one) and always prefetches "tile t + 1", with no last-tile case
    for (int e = ntiles; e < ntiles + 2; ++e) {
        if (ntiles > 0 && e % NPROD == p) {
            const int slot = e % NSLOT;
            wait_free(e, slot);
            if (lane == 0) __hip_atomic_store(&ready[slot], e + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    if constexpr (!SAMPLE) stamps_out_producer(st, lane, p);
}

// =====================================================================================================================
// the end of a consumer's full pass: its 32 lists, compacted, to global memory
// =====================================================================================================================
template <int NS, int KS>
__device__ __forceinline__ void write_final_lists(const PassCtx<NS, KS> cx, int& mycnt, int& nk, float& tau,
                                                  int32_t* __restrict__ cand, float* __restrict__ cand_v,
                                                  float* __restrict__ tau_out) {
    using S = Bf16Shape<NS, KS>;
    const int lane = cx.lane, wave = cx.wave, nrng = cx.nrng, out_chunk = cx.out_chunk, out_nchunks = cx.out_nchunks;
    unsigned long long* const buf = cx.lds.lists;
    for (int jj = 0; jj < 32; ++jj) compact_regs<KS, S::PLN>(buf, wave * 32 + jj, jj, lane, mycnt, nk, tau);
    for (int jj = 0; jj < 32; ++jj) {
        const int s = wave * 32 + jj;
        const int qq = cx.qblock * S::NQ + s;
        const int n = __builtin_amdgcn_readlane(nk, jj);
        // what this range rejected was rejected against thresholds >= the final working threshold of its lane pair;
        // kept entries at or above that threshold are as good as rejected (another range holds KS better ones), so
        // they are dropped here and the refine kernel only sees the few that matter
        const float w0 = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(tau), jj));
        const float w1 = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(tau), jj + 32));
        const float eff = w0 < w1 ? w0 : w1;
        if (lane < KS) {
            const unsigned long long key = buf[s * S::PITCH + lane];
            const float val = __uint_as_float((uint32_t)(key >> 32));
            const bool keep = lane < n && (val < eff || nrng == 1);
            cand[((int64_t)qq * out_nchunks + out_chunk) * KS + lane] = keep ? (int32_t)(uint32_t)key : -1;
            if (cand_v) cand_v[((int64_t)qq * out_nchunks + out_chunk) * KS + lane] = val;
        }
        if (lane == 0) tau_out[(int64_t)qq * out_nchunks + out_chunk] = eff;
        if (nrng == 1) {  // a whole-reference item owns every list column of its queries: the others stay empty
            for (int c = 1; c < out_nchunks; ++c) {
                if (lane < KS) cand[((int64_t)qq * out_nchunks + out_chunk + c) * KS + lane] = -1;
                if (lane == 0) tau_out[(int64_t)qq * out_nchunks + out_chunk + c] = __builtin_inff();
            }
        }
    }
}

// =====================================================================================================================
// the kernel; its body is the consumer waves' sweep
// =====================================================================================================================
// SAMPLE = true: threshold estimation only, entirely in registers and branch-free.  Each (tile, lane) contributes the
// minimum of its 16 values as ONE candidate; a lane keeps the KS/2 smallest of its candidates in a sorted register
// list (one min/max pair per entry and tile, issued in the gaps of the MFMA chain).  The two lanes of a query thus
// hold KS distinct references, so the larger of their two last entries bounds the KS-th nearest reference from
// above: a valid starting threshold for the full pass.  Nothing else is kept (the full pass rescans the sample
// rows), no list in the LDS is touched.  Output: tau_g[q] (order-preserving integer image of the threshold).
// SAMPLE = false: the full pass.  tau_g[q] is SHARED by all reference ranges of query q: every workgroup folds its
// own list's threshold into it (atomicMin) whenever it compacts, and refreshes its working threshold from it, so a
// range benefits from what the others have already found and extra ranges cost no extra selection work.  Each
// range's threshold is an upper bound of the KS-th nearest reference overall, hence so is their minimum; a stale
// read only leaves the filter looser, never wrong.
template <int NS, int KS, bool SAMPLE>
__global__ __launch_bounds__((Bf16Shape<NS, KS>::NWAVES * 64)) void knn_topk_bf16(
    const uint16_t* __restrict__ Pq, const uint16_t* __restrict__ PrF, int first_begin, int range_len, int r_limit,
    int n_full, int nranges, int out_chunk0, int out_nchunks, uint32_t* __restrict__ tau_g, int32_t* __restrict__ cand,
    float* __restrict__ cand_v, float* __restrict__ tau_out) {
    using S = Bf16Shape<NS, KS>;
    constexpr int NCONS = S::NCONS, PL = S::PLN, PITCH = S::PITCH, NQ = S::NQ, TILE_BYTES = S::TILE_BYTES, NSLOT = S::NSLOT;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Bf16Lds<S> lds = Bf16Lds<S>::carve(smem);
    char* const ring = lds.ring;
    unsigned long long* const buf = lds.lists;
    int* const ready = lds.ready;
    int* const done = lds.done;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: branches on it are scalar
    // the work item: a query block and its reference range (whole-reference blocks first, then the split ones, range-major)
    const WorkItem wi = decode_work_item(first_begin, range_len, r_limit, n_full, nranges);
    const int qblock = wi.qblock, rng = wi.rng, nrng = wi.nrng, r_begin = wi.r_begin, r_end = wi.r_end;
    const int ntiles = (r_end - r_begin) >> 5;
    const int out_chunk = out_chunk0 + rng;
    if (tid < Bf16Lds<S>::HANDOVER_WORDS) lds.handover()[tid] = 0;
    __syncthreads();

    const PassCtx<NS, KS> cx{lds, lane, wave, qblock, nrng, r_begin, ntiles, out_chunk, out_nchunks};
    if (wave >= NCONS) {
        producer_role<NS, KS, SAMPLE>(cx, PrF);
        return;
    }

    // ---------------------------------------------------------------------- consumer
    const int j = lane & 31, h = lane >> 5;
    const int qs = wave * 32 + j;
    const int q = qblock * NQ + qs;

    float tau = (!SAMPLE && tau_g) ? orderable_f32(tau_g[q]) : __builtin_inff();
    int nk = 0;  // entries in this query's kept list (the same in both of its lanes, like tau)

    bf16x8 bq[NS];
    {
        const f32x4* src = reinterpret_cast<const f32x4*>(Pq + (int64_t)q * (16 * NS) + h * (8 * NS));
#pragma unroll
        for (int s = 0; s < NS; ++s) bq[s] = __builtin_bit_cast(bf16x8, src[s]);
    }

    unsigned long long* pend = buf + qs * PITCH + KS + h * PL;
    int mycnt = 0;
    Stamps st;
    st.begin();

    // Tile hand-over.  Tile t + 1 (the producers stage two empty tiles past the end, so there always is one) is read
    // into the fragment registers while tile t computes, each register right after the MFMA that consumed it.  Its
    // ready word was polled one tile earlier (`seen`), so in steady state no LDS round trip is waited for.  After the
    // fragment reads the wave stores "read up to t + 1" in its done word of the slot -- queued behind the reads in
    // the wave's in-order LDS queue, so the producer cannot overwrite them early -- and polls the ready word of
    // tile t + 2.
    // The explicit lgkmcnt(0) at the top of every tile is free (everything queued is a tile old, the fragments of
    // tile t included) and leaves the compiler's wait-count pass with nothing pending: without it the pass makes the
    // MFMAs of tile t wait for the reads of tile t + 1 issued between them.
    const bool shared_tau = !SAMPLE && tau_g != nullptr && nrng > 1;
    uint32_t tau_fetch = 0xFFFFFFFFu;
    int seen = 0;
    int slot_n = 0;  // slot of the tile to read next
    int yield_tiles = 0;
    auto spin_until_staged = [&](int tile) __attribute__((always_inline)) {
        if (__builtin_amdgcn_readfirstlane(seen) < tile + 1) {
            yield_tiles = YIELD_TILES;
            const auto s0 = st.now();
            st.count(Stamps::NSPIN);
            do {
                __builtin_amdgcn_s_sleep(1);
                seen = lds_load_volatile(&ready[slot_n]);
            } while (seen < tile + 1);
            st.since(Stamps::SPIN, s0);
        }
    };
    auto read_tile = [&](f32x4(&a)[NS]) __attribute__((always_inline)) {
        const f32x4* tp = reinterpret_cast<const f32x4*>(ring + slot_n * TILE_BYTES) + lane;
#pragma unroll
        for (int s = 0; s < NS; ++s) a[s] = tp[s * 64];
    };
    auto hand_back = [&](int tile) __attribute__((always_inline)) {
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        if (lane == 0)
            __hip_atomic_store(&done[slot_n * NCONS + wave], tile + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        slot_n = slot_n + 1 == NSLOT ? 0 : slot_n + 1;
        seen = lds_load_volatile(&ready[slot_n]);
    };

    // One step = the MFMA chain of tile t into `cur`, with three other things issued in the gaps of the chain (the
    // wave cannot issue the next, dependent MFMA before the previous one is through the pipe): the refill of each
    // fragment register with tile t + 1 right after the MFMA that read it (a single fragment set: a refill lands a
    // whole tile period before its use), and the clean-tile filter of tile t - 1, whose products sit in `prev`.
    f32x4 a[NS];
    uint32_t best[SAMPLE ? KS / 2 : 1];
#pragma unroll
    for (int i = 0; i < (SAMPLE ? KS / 2 : 1); ++i) best[i] = 0xFF800000u;  // image of +inf
    auto step = [&](f32x16& cur, const f32x16& prev, const int t) __attribute__((always_inline)) {
        // Each SIMD hosts consumers w and w + 4; instruction arbitration goes by priority, then age, so at equal
        // priority the younger half (w >= 4) loses every contested slot, falls behind, and the older half waits for
        // it at the ring (measured: 290 vs 50 cycles of ring wait per tile).  A consumer that had to wait for the
        // ring is ahead of the others: it yields (priority 0) for the next few tiles, everybody else runs at 1.
        if (yield_tiles > 0) {
            __builtin_amdgcn_s_setprio(0);
            --yield_tiles;
        } else {
            __builtin_amdgcn_s_setprio(1);
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0)
        spin_until_staged(t + 1);
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        lds_cptr tbase = (lds_cptr)ring + (slot_n * TILE_BYTES + lane * 16);
        asm volatile("" : "+v"(tbase));     // the address is formed here, ...
        __builtin_amdgcn_sched_barrier(0);  // ... outside the interleaved block below
        const lds_f4ptr tp = (lds_f4ptr)tbase;
#pragma unroll
        for (int e = 0; e < 16; ++e) cur[e] = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            cur = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[s]), bq[s], cur, 0, 0, 0);
            a[s] = tp[s * 64];
        }
        // group minima (4 registers each), then the lane minimum, of the previous tile
        float g[4];
        unsigned long long gmask[4] = {0, 0, 0, 0};
#pragma unroll
        for (int u = 0; u < 4; ++u)
            g[u] = fminf(fminf(prev[4 * u], prev[4 * u + 1]), fminf(prev[4 * u + 2], prev[4 * u + 3]));
        const float mn = fminf(fminf(g[0], g[1]), fminf(g[2], g[3]));
        if constexpr (SAMPLE) {
            // sorted insertion on the order-preserving integer images (integer min/max need no NaN canonicalisation);
            // at step 0 `prev` is +inf and changes nothing
            uint32_t x = f32_orderable(mn);
#pragma unroll
            for (int i = 0; i < KS / 2; ++i) {
                const uint32_t lo = min(best[i], x);
                x = max(best[i], x);
                best[i] = lo;
            }
            asm volatile("" ::"v"(best[KS / 2 - 1]));  // keep it in this block
        } else {
            // the four group tests are evaluated here, under the MFMA chain, and leave scalar masks: the branches after
            // the chain then hang on scalar registers only (a mask that a later merge of this tile makes stale is
            // merely looser: every value is still compared with the current threshold)
#pragma unroll
            for (int u = 0; u < 4; ++u) gmask[u] = __builtin_amdgcn_ballot_w64(g[u] < tau);
            asm volatile("" ::"s"(gmask[0]), "s"(gmask[1]), "s"(gmask[2]), "s"(gmask[3]));  // keep the filter in this block
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // one MFMA
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // one LDS read
            __builtin_amdgcn_sched_group_barrier(0x002, SAMPLE ? 2 + (KS + NS - 1) / NS : 2, 0);  // a share of the VALU
        }
        hand_back(t + 1);
        if constexpr (SAMPLE) return;

        const int r0 = r_begin + ((t - 1) << 5);  // the tile whose products are in `prev`
        if ((gmask[0] | gmask[1] | gmask[2] | gmask[3]) == 0) return;
        st.count(Stamps::EVT);
        const auto e0 = st.now();
        auto flush_full = [&]() __attribute__((always_inline)) {
            unsigned long long fm = __builtin_amdgcn_ballot_w64(mycnt > PL - 4);  // keep 4 slots free
            if (fm) {
                const auto s0 = st.now();
                st.count(Stamps::NFLUSH);
                fm = (fm | (fm >> 32)) & 0xFFFFFFFFull;
                st.add(Stamps::NCOMP, (unsigned long long)__builtin_popcountll(fm));
                while (fm) {
                    const int jj = __builtin_ctzll(fm);
                    fm &= fm - 1;
                    compact_regs<KS, PL>(buf, wave * 32 + jj, jj, lane, mycnt, nk, tau);
                }
                if constexpr (!SAMPLE) {
                    // publish this list's threshold (fire and forget; what the other ranges publish is picked up by
                    // the periodic refresh above)
                    if (shared_tau && h == 0) atomicMin(&tau_g[q], f32_orderable(tau));
                }
                st.since(Stamps::COMP, s0);
            }
        };
        {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (gmask[u] == 0) continue;
                st.count(Stamps::GRP);
                // a pending list keeps 4 free slots at this point, so the group's four values are appended in straight
                // line code: a lane whose value does not pass writes it to the list's last slot instead, which stays
                // unused as long as anything fails (at most 3 real entries land in the 4 free slots then)
                const int rbase = r0 + 8 * u + 4 * h;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = prev[4 * u + e];
                    const bool pass = v < tau;
                    uint32_t* dst = reinterpret_cast<uint32_t*>(pend + (pass ? mycnt : PL - 1));
                    dst[0] = (uint32_t)(rbase + e);
                    dst[1] = __float_as_uint(v);
                    mycnt += pass ? 1 : 0;
                }
                flush_full();
            }
        }
        st.since(Stamps::EVC, e0);
    };

    f32x16 accA, accB;
#pragma unroll
    for (int e = 0; e < 16; ++e) accA[e] = accB[e] = __builtin_inff();  // "previous tile" of step 0: nothing passes
    if (ntiles > 0) {
        spin_until_staged(0);
        __atomic_signal_fence(__ATOMIC_SEQ_CST);
        read_tile(a);
        hand_back(0);
        // steps 0 .. ntiles: step t multiplies tile t (step ntiles: an empty tile, product unused) and filters tile
        // t - 1; two steps per iteration so that the two accumulators alternate statically
        for (int t2 = 0; t2 <= ntiles; t2 += 2) {
            if constexpr (!SAMPLE) {
                // periodic refresh of the shared threshold: the (L1-bypassing) load is issued here and looked at one
                // iteration later, so nobody waits for the round trip
                if (shared_tau) {
                    if ((t2 & 15) == 2) tau = fminf(tau, orderable_f32(tau_fetch));
                    if ((t2 & 15) == 0)
                        tau_fetch = __hip_atomic_load(&tau_g[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            step(accA, accB, t2);
            if (t2 + 1 <= ntiles) step(accB, accA, t2 + 1);
        }
    }

    if constexpr (SAMPLE) {
        const uint32_t mine = best[KS / 2 - 1], other = __shfl_xor(mine, 32);
        if (h == 0) tau_g[q] = max(mine, other);
        return;
    }
    stamps_out_consumer(st, lane, wave, ntiles);
    write_final_lists(cx, mycnt, nk, tau, cand, cand_v, tau_out);
}

template <int NS, int KS>
void launch(hipStream_t stream, KnnWorkspace& ws, const PassLaunch& L) {
    using S = Bf16Shape<NS, KS>;
    constexpr size_t lds = S::lds_bytes;
    const auto full = &knn_topk_bf16<NS, KS, false>, sample = &knn_topk_bf16<NS, KS, true>;
    ensure_dynamic_lds(reinterpret_cast<const void*>(full), lds);
    ensure_dynamic_lds(reinterpret_cast<const void*>(sample), lds);
    std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
    if (ws.profile) {
        ev = ws.next_events(L.sample ? 0 : 2);
        BMX_HIP(hipEventRecord(ev.first, stream));
    }
    const int items = L.n_full + (L.nqb - L.n_full) * L.nranges;
    const auto pass = L.sample ? sample : full;
    hipLaunchKernelGGL(pass, dim3(items), dim3(S::NWAVES * 64), lds, stream, L.pq, L.pr, L.first_begin, L.range_len, L.r_limit,
                       L.n_full, L.nranges, L.out_chunk0, L.out_nchunks, L.tau_g, L.cand, L.cand_v, L.tau);
    BMX_LAUNCH_CHECK();
    if (ws.profile) BMX_HIP(hipEventRecord(ev.second, stream));
#ifdef BMX_STAMPS
    if (!L.sample) {
        unsigned long long h[48];
        BMX_HIP(hipStreamSynchronize(stream));
        BMX_HIP(hipMemcpyFromSymbol(h, HIP_SYMBOL(bmx_dbg), sizeof(h)));
        const double w = (double)h[9], nt = (double)h[8];
        fprintf(stderr, "[stamps] waves=%.0f tiles/wave=%.0f cyc/tile=%.0f spin/tile=%.0f flush/tile=%.0f nspin/tile=%.3f nflush/tile=%.3f ncomp/tile=%.3f evt/tile=%.3f grp/tile=%.3f cyc/flush=%.0f evpath/tile=%.0f\n",
                w, nt / w, h[0] / nt, h[1] / nt, h[2] / nt, h[3] / nt, h[4] / nt, h[5] / nt, h[6] / nt, h[7] / nt, h[4] ? (double)h[2] / h[4] : 0.0, h[10] / nt);
        fprintf(stderr, "[stamps] spin/tile by consumer:");
        for (int i = 0; i < S::NCONS; ++i) fprintf(stderr, " %.0f", h[16 + i] / (nt / S::NCONS));
        fprintf(stderr, "  flush/tile:");
        for (int i = 0; i < S::NCONS; ++i) fprintf(stderr, " %.0f", h[24 + i] / (nt / S::NCONS));
        fprintf(stderr, "  producer waiting fraction:");
        for (int i = 0; i < S::NPROD; ++i) fprintf(stderr, " %.2f", h[36 + i] ? (double)h[32 + i] / h[36 + i] : 0.0);
        fprintf(stderr, "\n");
        unsigned long long z[48] = {0};
        BMX_HIP(hipMemcpyToSymbol(HIP_SYMBOL(bmx_dbg), z, sizeof(z)));
    }
#endif
}

}  // namespace

int bf16_pick_ns(int d) {
    static const int opts[] = {1, 2, 3, 4, 6, 8, 10, 13, 16, 19, 24};
    for (int o : opts)
        if (3 * d + 3 <= 16 * o) return o;
    return 0;
}

int bf16_ncons(int NS, int KS) { return ring_shape(NS, KS).ncons; }

bool bf16_launch(hipStream_t stream, KnnWorkspace& ws, int NS, int KS, const PassLaunch& L) {
#define BMX_CASE(N)                        \
    case N:                                \
        if (KS == 24)                      \
            launch<N, 24>(stream, ws, L);  \
        else if constexpr (N <= 16)        \
            launch<N, 40>(stream, ws, L);  \
        else                               \
            return false;                  \
        return true;
    switch (NS) {
        BMX_CASE(1)
        BMX_CASE(2)
        BMX_CASE(3)
        BMX_CASE(4)
        BMX_CASE(6)
        BMX_CASE(8)
        BMX_CASE(10)
        BMX_CASE(13)
        BMX_CASE(16)
        BMX_CASE(19)
        BMX_CASE(24)
        default:
            return false;
    }
#undef BMX_CASE
}

}  // namespace bmx
