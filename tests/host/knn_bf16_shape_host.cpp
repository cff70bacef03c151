// Stand-alone host program (no HIP call, no HIP header): prints the workgroup shape of the split-bf16 candidate pass
// (csrc/knn_bf16_shape.hpp: Bf16Shape, Bf16Lds) for every instantiation bf16_launch can reach, one JSON object a line, and
// checks the invariants every shape must keep.  tests/test_cpu_knn_bf16_shape.py builds it with AddressSanitizer and
// UndefinedBehaviorSanitizer and compares the lines with tests/golden/knn_bf16_shape_parent.json.
#include <cstdio>

#include "knn_bf16_shape.hpp"

using namespace bmx::bf16;

static int bad = 0;
alignas(16) static char smem[160 * 1024];  // carve() only forms addresses in it

template <int NS, int KS>
static void row() {
    using S = Bf16Shape<NS, KS>;
    using L = Bf16Lds<S>;
    std::printf("{\"KS\": %d, \"NS\": %d, \"NCONS\": %d, \"NPROD\": %d, \"PLN\": %d, \"NSLOT\": %d, \"PITCH\": %d, "
                "\"lds_bytes\": %d}\n",
                KS, NS, S::NCONS, S::NPROD, S::PLN, S::NSLOT, S::PITCH, S::lds_bytes);
    bool ok = S::lds_bytes <= LDS_TOTAL && S::NSLOT >= 2 && S::CAP == KS + 2 * S::PLN && S::CAP <= 64 && S::PITCH > S::CAP &&
              S::NQ == 32 * S::NCONS && S::TILE_BYTES == 1024 * NS && S::NWAVES == S::NCONS + S::NPROD;
    // the shape as its parts: what ring_shape gives, and the region table against the budget
    ok = ok && S::NCONS == ring_shape(NS, KS).ncons && S::NPROD == ring_shape(NS, KS).nprod && S::PLN == ring_shape(NS, KS).pln &&
         L::bytes() == S::lds_bytes && S::NSLOT <= RING_MAX &&
         (S::NSLOT == RING_MAX || S::lds_bytes + S::TILE_BYTES > LDS_TOTAL) && S::PITCH == bmx::sel::list_pitch(KS, S::PLN);
    // carve(): the regions in address order, each as long as the table says, the last one ending at bytes(); the ring
    // 16-byte aligned (it is read and written in 16-byte pieces), the lists 8-byte aligned; the hand-over words contiguous
    // from handover() on
    const L l = L::carve(smem);
    ok = ok && l.ring == smem && (char*)l.lists == l.ring + L::RING_BYTES && (char*)l.ready == (char*)l.lists + L::LISTS_BYTES &&
         (char*)l.ready + HANDOVER_BYTES == smem + L::bytes() && ((size_t)(l.ring - smem) % 16) == 0 && S::TILE_BYTES % 16 == 0 &&
         ((size_t)((char*)l.lists - smem) % 8) == 0 && L::LISTS_BYTES == S::NQ * S::PITCH * 8 && l.handover() == l.ready &&
         l.done == l.ready + S::NSLOT && l.done + S::NSLOT * S::NCONS == l.handover() + L::HANDOVER_WORDS &&
         L::HANDOVER_WORDS * 4 <= HANDOVER_BYTES;
    if (!ok) {
        std::printf("invariant broken in the line above\n");
        ++bad;
    }
}

int main() {
    row<1, 24>();
    row<2, 24>();
    row<3, 24>();
    row<4, 24>();
    row<6, 24>();
    row<8, 24>();
    row<10, 24>();
    row<13, 24>();
    row<16, 24>();
    row<19, 24>();
    row<24, 24>();
    row<1, 40>();
    row<2, 40>();
    row<3, 40>();
    row<4, 40>();
    row<6, 40>();
    row<8, 40>();
    row<10, 40>();
    row<13, 40>();
    row<16, 40>();
    if (bad) return 1;
    std::printf("shape checks ok\n");
    return 0;
}
