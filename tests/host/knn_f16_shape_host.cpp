// Stand-alone host program (no HIP call, no HIP header): prints the workgroup shape of the fp16 candidate pass
// (csrc/knn_f16_shape.hpp: F16Shape, F16Lds) for every instantiation f16_launch can reach, one JSON object a line, and checks
// the invariants every shape must keep.  tests/test_cpu_knn_f16_shape.py builds it with AddressSanitizer and
// UndefinedBehaviorSanitizer and compares the lines with tests/golden/knn_f16_shape_parent.json.
#include <cstdio>

#include "knn_f16_shape.hpp"

using namespace bmx::f16;

static int bad = 0;
alignas(16) static char smem[160 * 1024];  // carve() only forms addresses in it

template <int NS, int KS>
static void row() {
    using S = F16Shape<NS, KS>;
    using L = F16Lds<S>;
    std::printf("{\"KS\": %d, \"NS\": %d, \"TP\": %d, \"LCAP\": %d, \"NSLOT\": %d, \"KEEP_MAX\": %d, \"NSERV\": %d, "
                "\"lds_bytes\": %d}\n",
                KS, NS, S::TP, S::LCAP, S::NSLOT, S::KEEP_MAX, S::NSERV, S::lds_bytes);
    bool ok = S::lds_bytes <= 160 * 1024 && S::NSLOT >= 2 && KS < S::LCAP && S::LCAP <= 64 && S::KEEP_MAX >= KS &&
              NCONS % S::NSERV == 0 && (NCONS / S::NSERV) % 2 == 0 && (S::TP != 2 || S::NSLOT >= 3);
    // the shape as its parts: what the four functions give, and the region table against the budget
    ok = ok && S::TP == tile_pairs_for(NS, KS) && S::LCAP == list_cap(NS, KS) && S::NSLOT == ring_slots_for(NS, S::LCAP, S::TP) &&
         S::NSERV == serv_waves(NS) && L::bytes() == S::lds_bytes;
    // carve(): the regions in address order, each as long as the table says, the last one ending at bytes(); the hand-over
    // words contiguous from handover() on
    const L l = L::carve(smem);
    const char* at[] = {l.ring, (char*)l.lists, (char*)l.qvals, (char*)l.qtags, (char*)l.cnt, (char*)l.tauL, (char*)l.mgL,
                        (char*)l.ready};
    const int len[] = {L::RING_BYTES, L::LISTS_BYTES, L::QVALS_BYTES, L::QTAGS_BYTES, L::PER_QUERY_BYTES, L::PER_QUERY_BYTES,
                       L::PER_QUERY_BYTES};
    ok = ok && at[0] == smem;
    for (int i = 0; i < 7; ++i) ok = ok && at[i + 1] == at[i] + len[i];
    ok = ok && (char*)l.ready + HANDOVER_BYTES == smem + L::bytes() && l.handover() == l.ready && l.done == l.ready + S::NSLOT &&
         l.wrL == l.done + S::NSLOT && l.rdL == l.wrL + NCONS && l.stL == l.rdL + NCONS &&
         l.stL + NCONS == l.handover() + L::HANDOVER_WORDS && ((size_t)((char*)l.lists - smem) % 16) == 0 &&
         ((size_t)((char*)l.qvals - smem) % 16) == 0;
    if (!ok) {
        std::printf("invariant broken in the line above\n");
        ++bad;
    }
}

int main() {
    row<1, 32>();
    row<2, 32>();
    row<3, 32>();
    row<4, 32>();
    row<5, 32>();
    row<6, 32>();
    row<7, 32>();
    row<8, 32>();
    row<1, 48>();
    row<2, 48>();
    row<3, 48>();
    row<4, 48>();
    if (bad) return 1;
    std::printf("shape checks ok\n");
    return 0;
}
