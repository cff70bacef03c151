// The shape of a workgroup of the fp16 candidate pass (knn_f16.hip: knn_topk_f16): its waves, what its LDS holds and WHERE
// every piece of that lies -- pure functions of the fragment count NS and the list size KS.  No HIP call and no HIP header:
// tests/host/knn_f16_shape_host.cpp pins the shape of every instantiation on the CPU.  The kernel's static_asserts and
// __launch_bounds__, its launcher and f16_rows_per_slot all read F16Shape; the kernel takes its LDS pointers from F16Lds.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define BMX_F16_HD __host__ __device__
#else
#define BMX_F16_HD
#endif

// ---- the tunables of the kernel, overridable for A/B builds (make VARIANT=x EXTRA=-DBMX_...=n) -------------------------
#ifndef BMX_NSERV
#define BMX_NSERV 4  // service waves where the consumers fit 128 registers (NS <= 5): each works off NCONS / n spill queues
#endif
#ifndef BMX_DRAIN_MIN
#define BMX_DRAIN_MIN 16  // records in a queue before its service wave bothers: a pass costs the same for 1 record as for 32
#endif
#ifndef BMX_SPRIO
#define BMX_SPRIO 0  // issue priority of the service waves: the lowest, they work in what the consumers leave
#endif
#ifndef BMX_CPRIO_LO
#define BMX_CPRIO_LO 0  // issue priority of the first-dispatched half of the consumers (waves 0..3)
#endif
#ifndef BMX_CPRIO_HI
#define BMX_CPRIO_HI 1  // ... and of the second half (waves 4..7), which at equal priority loses every contested issue slot
#endif
#ifndef BMX_HEAD
#define BMX_HEAD 4  // a list is compacted ahead of time once fewer than this many slots are free
#endif
#ifndef BMX_RING_MAX
#define BMX_RING_MAX 4  // ring slots at most (config 3, slots of four tiles: three gain 5 %, two nothing, four no more than three)
#endif
#ifndef BMX_NPIV
#define BMX_NPIV 4  // pivots a compaction tries at once before it falls back to the exact quickselect
#endif
#ifndef BMX_PSLEEP
#define BMX_PSLEEP 1  // s_sleep argument of a producer that waits for a ring position, and of an idle service wave
#endif
#ifndef BMX_LCAP_MAX
#define BMX_LCAP_MAX 56  // longest list (kept + pending entries) a query gets
#endif
#ifndef BMX_TP_MAX
#define BMX_TP_MAX 2  // tile pairs per ring slot at most: 2 = slots of four tiles where they fit (config 3: passes -5 %)
#endif

namespace bmx {
namespace f16 {

constexpr int NCONS = 8;   // consumer waves (32 queries each): two per SIMD
constexpr int NPROD = 2;   // producer waves
// service waves (each works off the spill queues of NCONS / n consumers).  Fourteen waves on a CU leave a wave 128
// registers, twelve 168: the long-K consumers (fragments of two tiles + query fragments + two accumulators) need the latter
BMX_F16_HD constexpr int serv_waves(int NS) { return NS <= 5 ? BMX_NSERV : 2; }
constexpr int NQ = NCONS * 32;
constexpr int QCAP = 64;   // spill records per consumer wave (one group of one tile can fill all 64)
constexpr int EPI_CONS = 20;  // of a consumer's 32 final lists, those it writes out itself (its service wave: the rest)
constexpr int DRAIN_MIN = BMX_DRAIN_MIN;  // records in a queue before its service wave bothers (unless the consumer waits)
constexpr int HEAD = BMX_HEAD;    // a list is compacted ahead of time once fewer than HEAD slots are free
constexpr int LDS_TOTAL = 160 * 1024;
constexpr int HANDOVER_BYTES = 512;  // the hand-over words' corner of the LDS (ready, done, wrL, rdL, stL; the rest spare)

// ---------------------------------------------------------------------------------------------------
// LDS budget: ring of reference tiles | per-query lists | per-wave spill queues | list counters | published
// thresholds | hand-over words
// ---------------------------------------------------------------------------------------------------
BMX_F16_HD constexpr int lds_fixed_bytes() { return NCONS * QCAP * 20 + NQ * 4 + NQ * 4 + NQ * 4 + HANDOVER_BYTES; }
// A ring slot holds TP PAIRS of reference tiles (64 TP rows): the consumers wait, hand back and poll once per slot.
BMX_F16_HD constexpr int ring_slots_for(int NS, int LCAP, int TP) {
    const int rest = LDS_TOTAL - lds_fixed_bytes() - NQ * LCAP * 8;
    const int n = rest / (TP * 2 * NS * 1024);
    return n > BMX_RING_MAX ? BMX_RING_MAX : n;
}
// Slots of FOUR tiles (TP = 2) where a ring of three such slots fits beside lists of at least KS + 16 entries (up to 61
// columns at KS = 32): the hand-over -- ready check, polls, hand-back: a quarter of the base loop -- then comes once per
// four tiles (config 3: candidate passes -5 %; with two such slots: no gain, with four: as with three).  Else two tiles.
BMX_F16_HD constexpr int tile_pairs_for(int NS, int KS) {
    return (BMX_TP_MAX >= 2 && KS + 16 <= BMX_LCAP_MAX && ring_slots_for(NS, KS + 16, 2) >= 3) ? 2 : 1;
}
// list capacity: the longest that leaves the ring three slots of four tiles, or at least two slots of two; else as short as
// a useful pending part allows
BMX_F16_HD constexpr int list_cap(int NS, int KS) {
    const int TP = tile_pairs_for(NS, KS);
    for (int c = BMX_LCAP_MAX; c >= KS + 16; c -= 8)
        if (ring_slots_for(NS, c, TP) >= (TP == 2 ? 3 : 2)) return c;
    return KS + 16 <= 64 ? KS + 16 : 64;
}

// The MFMA shape of the consumers' sweep per (NS, KS): 0 = 32x32x16, one accumulator per tile; 1 = 16x16x32, four 16 x 16
// blocks per tile (even NS only; knn_f16.hip has what a lane holds under either).  Same LDS, same pipe time, same registers:
// an entry is 1 only where the step measured faster by wall time with it; unmeasured shapes stay 0.  Measured: NS = 4,
// KS = 32 (config 3): 4 % more cycles a tile at a 9 % higher clock, the step 1.2 - 2.5 % shorter (MEASUREMENTS.md).
BMX_F16_HD constexpr int mfma_shape_for(int NS, int KS) { return NS == 4 && KS == 32 ? 1 : 0; }

// Everything a (NS, KS) instantiation derives from the four functions above, once.
template <int NS_, int KS_>
struct F16Shape {
    static constexpr int NS = NS_, KS = KS_;
    static constexpr int TP = tile_pairs_for(NS, KS);  // tile pairs per ring slot
    static constexpr int LCAP = list_cap(NS, KS);      // entries of a query's list
    static constexpr int NSLOT = ring_slots_for(NS, LCAP, TP);
    static constexpr int TILE_BYTES = NS * 1024;
    static constexpr int SLOT_BYTES = TP * 2 * TILE_BYTES;
    // what a cut in mid-sweep may keep: a full list must come out with room again (the appends that found it full retry
    // until they fit), and a cut that frees next to nothing would be back at once
    static constexpr int KEEP_MAX = KS + 11 < LCAP - 4 ? KS + 11 : LCAP - 4;
    static constexpr int NSERV = serv_waves(NS);
    static constexpr int CPS = NCONS / NSERV;  // consumers a service wave looks after
    static constexpr int NWAVES = NCONS + NPROD + NSERV;
    static constexpr int lds_bytes = NSLOT * SLOT_BYTES + NQ * LCAP * 8 + lds_fixed_bytes();
    static_assert(NSLOT >= 2, "LDS ring");
    static_assert(LCAP <= 64 && LCAP > KS, "one list entry per lane during compaction");
    static_assert(KEEP_MAX >= KS, "list capacity");
    static_assert(NCONS % NSERV == 0 && (NCONS / NSERV) % 2 == 0, "a service wave's consumers: whole groups of 64 queries");
    static_assert((QCAP & (QCAP - 1)) == 0 && QCAP >= 64, "queue positions wrap by masking; one group can hold 64 records");
};

// The region table of the workgroup's LDS, in address order.  carve() is the one place that turns the dynamic LDS into
// typed pointers.
template <class S>
struct F16Lds {
    char* ring;                 // [NSLOT][2 TP][TILE_BYTES] staged reference tiles, fragment-major, written by the producers
    unsigned long long* lists;  // [NQ][LCAP] a query's candidates, unsorted: value bits << 32 | reference row
    float* qvals;               // [NCONS][QCAP][4] spill queue of a consumer: the four raw values of a group of references
    uint32_t* qtags;            // [NCONS][QCAP] ... and the record's tag: tile << 8 | group << 6 | lane that spilled it
    int* cnt;                   // [NQ] entries in each list (appends take their slot from it with an LDS atomic)
    float* tauL;                // [NQ] thresholds as the service waves last published them
    float* mgL;                 // [NQ] twice the pass's error bound of each query (0: the KS-th-best cut only)
    // ---- the hand-over words: contiguous, HANDOVER_WORDS of them, zeroed together when the workgroup starts
    int* ready;                 // [NSLOT] number of the slot staged at the position, plus one
    int* done;                  // [NSLOT] hand-backs of the position so far (every consumer adds one per slot read)
    int* wrL;                   // [NCONS] records pushed so far (written by the consumer)
    int* rdL;                   // [NCONS] records worked off so far (written by its service wave)
    int* stL;                   // [NCONS] consumer state: 0 sweeping, 1 waiting for room in its queue, 2 through, 3 lists out

    static constexpr int RING_BYTES = S::NSLOT * S::SLOT_BYTES;
    static constexpr int LISTS_BYTES = NQ * S::LCAP * 8;
    static constexpr int QVALS_BYTES = NCONS * QCAP * 16;
    static constexpr int QTAGS_BYTES = NCONS * QCAP * 4;
    static constexpr int PER_QUERY_BYTES = NQ * 4;  // cnt, tauL, mgL each
    static constexpr int HANDOVER_WORDS = 2 * S::NSLOT + 3 * NCONS;
    static_assert(HANDOVER_WORDS * 4 <= HANDOVER_BYTES, "hand-over words");
    static_assert(HANDOVER_WORDS <= S::NWAVES * 64, "one thread zeroes one hand-over word");

    BMX_F16_HD static constexpr int bytes() {
        return RING_BYTES + LISTS_BYTES + QVALS_BYTES + QTAGS_BYTES + 3 * PER_QUERY_BYTES + HANDOVER_BYTES;
    }
    static_assert(RING_BYTES + LISTS_BYTES + QVALS_BYTES + QTAGS_BYTES + 3 * PER_QUERY_BYTES + HANDOVER_BYTES == S::lds_bytes,
                  "the region table is the LDS budget");

    BMX_F16_HD static F16Lds carve(char* smem) {
        F16Lds l;
        l.ring = smem;
        l.lists = reinterpret_cast<unsigned long long*>(smem + RING_BYTES);
        l.qvals = reinterpret_cast<float*>(l.lists + NQ * S::LCAP);
        l.qtags = reinterpret_cast<uint32_t*>(l.qvals + NCONS * QCAP * 4);
        l.cnt = reinterpret_cast<int*>(l.qtags + NCONS * QCAP);
        l.tauL = reinterpret_cast<float*>(l.cnt + NQ);
        l.mgL = l.tauL + NQ;
        l.ready = reinterpret_cast<int*>(l.mgL + NQ);
        l.done = l.ready + S::NSLOT;
        l.wrL = l.done + S::NSLOT;
        l.rdL = l.wrL + NCONS;
        l.stL = l.rdL + NCONS;
        return l;
    }
    // the hand-over words as one span (ready[0] is its first word)
    BMX_F16_HD int* handover() const { return ready; }
};

}  // namespace f16
}  // namespace bmx
