// The shape of a workgroup of the split-bf16 candidate pass (knn_bf16.hip: knn_topk_bf16): its waves, what its LDS holds and
// WHERE every piece of that lies -- pure functions of the fragment count NS and the list size KS.  No HIP call and no HIP
// header: tests/host/knn_bf16_shape_host.cpp pins the shape of every instantiation on the CPU.  The kernel's static_asserts
// and __launch_bounds__, its launcher and bf16_ncons all read Bf16Shape; the kernel takes its LDS pointers from Bf16Lds.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define BMX_BF16_HD __host__ __device__
#else
#define BMX_BF16_HD
#endif

// ---- the tunable of the kernel, overridable for A/B builds (make VARIANT=x EXTRA=-DBMX_YIELD_TILES=n) -------------------
#ifndef BMX_YIELD_TILES
#define BMX_YIELD_TILES 8  // tiles a consumer that had to wait for the ring runs at the low issue priority
#endif

namespace bmx {
namespace sel {
// Row pitch of a query's list in 8-byte entries: one more than the capacity (KS kept entries, two pending lists of PLN), so
// that the lists of neighbouring queries start 2 banks apart and the appends of a wave's lanes do not pile up on one bank
// pair.  (Here, not in knn_select.hpp beside compact_regs, which addresses the lists with it: the shape needs it on the host.)
BMX_BF16_HD constexpr int list_pitch(int KS, int PLN) { return KS + 2 * PLN + 1; }
}  // namespace sel
namespace bf16 {

constexpr int LDS_TOTAL = 160 * 1024;
constexpr int HANDOVER_BYTES = 512;  // the hand-over words' corner of the LDS (ready, done; the rest spare)
constexpr int YIELD_TILES = BMX_YIELD_TILES;
constexpr int RING_MAX = 8;  // ring slots at most

// Workgroup shape per (fragment count, list size): NCONS consumer waves of 32 queries, NPROD producer waves (producer p
// stages tiles p, p + NPROD, ... into ring slot tile % NSLOT), PLN entries per lane-private pending list.
// 8 + 4 puts two consumers and one producer on every SIMD.  Measured alternatives at 100k x 100k, d = 50 (cycles per
// tile per consumer wave, 1480 for 8 + 4): 9 + 3 -> 1750, 10 + 2 -> 1940 -- the SIMDs that get a third consumer fall
// behind and the ring makes everybody else wait for them, so more queries per CU did not pay.
struct RingShape {
    int ncons, nprod, pln;
};
BMX_BF16_HD constexpr RingShape ring_shape(int NS, int KS) {
    return (NS <= 13 && KS == 24) ? RingShape{8, 4, 12} : RingShape{4, 4, 12};
}

// Everything a (NS, KS) instantiation derives from ring_shape, once.
template <int NS_, int KS_>
struct Bf16Shape {
    static constexpr int NS = NS_, KS = KS_;
    static constexpr int NCONS = ring_shape(NS, KS).ncons;
    static constexpr int NPROD = ring_shape(NS, KS).nprod;
    static constexpr int PLN = ring_shape(NS, KS).pln;
    static constexpr int NWAVES = NCONS + NPROD;
    static constexpr int CAP = KS + 2 * PLN;  // entries of a query's list: KS kept, two pending lists of PLN
    static constexpr int PITCH = sel::list_pitch(KS, PLN);  // row pitch of a query's list, 8-byte entries
    static constexpr int NQ = NCONS * 32;
    static constexpr int TILE_BYTES = NS * 1024;
    static constexpr int LISTS_BYTES = NQ * PITCH * 8;
    // Ring depth: as many staged tiles as the LDS left over by the candidate lists holds (at most 8).  The consumers of a
    // workgroup stall at different times (a compaction costs a couple of tile times); the deeper the ring, the less one
    // consumer's stall holds up the others.
    static constexpr int NSLOT = (LDS_TOTAL - LISTS_BYTES - HANDOVER_BYTES) / TILE_BYTES > RING_MAX
                                     ? RING_MAX
                                     : (LDS_TOTAL - LISTS_BYTES - HANDOVER_BYTES) / TILE_BYTES;
    static constexpr int lds_bytes = NSLOT * TILE_BYTES + LISTS_BYTES + HANDOVER_BYTES;
    static_assert(NSLOT >= 2, "LDS ring: a tile is staged while another is read");
    static_assert(CAP <= 64, "one candidate per lane during compaction");
    static_assert(lds_bytes <= LDS_TOTAL, "LDS budget");
};

// The region table of the workgroup's LDS, in address order.  carve() is the one place that turns the dynamic LDS into
// typed pointers.
template <class S>
struct Bf16Lds {
    char* ring;                 // [NSLOT][TILE_BYTES] staged reference tiles, fragment-major, written by the producers
    unsigned long long* lists;  // [NQ][PITCH] a query's candidates: raw f32 value bits << 32 | reference row
    // ---- the hand-over words: contiguous, HANDOVER_WORDS of them, zeroed together when the workgroup starts
    int* ready;                 // [NSLOT] number of the tile staged in the slot, plus one
    int* done;                  // [NSLOT][NCONS] number of the last tile the consumer has read from the slot, plus one

    static constexpr int RING_BYTES = S::NSLOT * S::TILE_BYTES;
    static constexpr int LISTS_BYTES = S::LISTS_BYTES;
    static constexpr int HANDOVER_WORDS = S::NSLOT * (1 + S::NCONS);
    static_assert(HANDOVER_WORDS * 4 <= HANDOVER_BYTES, "hand-over words");
    static_assert(HANDOVER_WORDS <= S::NWAVES * 64, "one thread zeroes one hand-over word");

    BMX_BF16_HD static constexpr int bytes() { return RING_BYTES + LISTS_BYTES + HANDOVER_BYTES; }
    static_assert(RING_BYTES + LISTS_BYTES + HANDOVER_BYTES == S::lds_bytes, "the region table is the LDS budget");

    BMX_BF16_HD static Bf16Lds carve(char* smem) {
        Bf16Lds l;
        l.ring = smem;
        l.lists = reinterpret_cast<unsigned long long*>(smem + RING_BYTES);
        l.ready = reinterpret_cast<int*>(l.lists + S::NQ * S::PITCH);
        l.done = l.ready + S::NSLOT;
        return l;
    }
    // the hand-over words as one span (ready[0] is its first word)
    BMX_BF16_HD int* handover() const { return ready; }
};

}  // namespace bf16
}  // namespace bmx
