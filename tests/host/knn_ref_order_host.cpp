// Stand-alone host program (no HIP call): the pure part of the ordered references (csrc/knn_order.hpp) -- the bucket of a
// key, the degenerate case, the offsets, the permutation -- on keys read from a file.
//   knn_ref_order_host KEYS.f32 NR NR_PAD OUT.i32
// reads NR little-endian f32 keys, writes the NR_PAD image positions (int32) and prints the number of buckets in use.  On the
// way it checks the offsets on a known input and the `ordered` flag of the pass plan (csrc/knn_plan.hpp): non-zero exit.
// tests/test_cpu_knn_ref_order.py builds it with AddressSanitizer and UndefinedBehaviorSanitizer and compares with numpy.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "knn_order.hpp"
#include "knn_plan.hpp"

int main(int argc, char** argv) {
    if (argc != 5) {
        fprintf(stderr, "usage: %s KEYS.f32 NR NR_PAD OUT.i32\n", argv[0]);
        return 2;
    }
    const int nr = atoi(argv[2]), nr_pad = atoi(argv[3]);
    if (nr < 1 || nr_pad < nr) return 2;
    std::vector<float> key(nr);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(key.data(), sizeof(float), nr, f) != (size_t)nr) return 3;
    fclose(f);
    std::vector<int32_t> pos(nr_pad, -1);
    const int used = bmx::order::order_positions(key.data(), nr, nr_pad, pos.data());
    // the offsets on their own: sizes 0, 1, 2, ... -> triangular numbers
    uint32_t counts[bmx::order::ORDER_BUCKETS], offs[bmx::order::ORDER_BUCKETS];
    for (int b = 0; b < bmx::order::ORDER_BUCKETS; ++b) counts[b] = (uint32_t)b;
    bmx::order::bucket_offsets(counts, offs);
    for (int b = 0; b < bmx::order::ORDER_BUCKETS; ++b)
        if (offs[b] != (uint32_t)(b * (b - 1) / 2)) return 4;
    // the plan's trailing flag: off, every number is the plan's without it; on, the sample of an unseeded search is capped and
    // nothing else moves; the seeded search keeps its own
    {
        const bmx::DevKnobs knobs;
        const bmx::PassPlan a = bmx::plan_candidate_pass(1, 4, 32, 256, 128, 100000, 400000, false, knobs);
        const bmx::PassPlan b = bmx::plan_candidate_pass(1, 4, 32, 256, 128, 100000, 400000, false, knobs, false);
        const bmx::PassPlan c = bmx::plan_candidate_pass(1, 4, 32, 256, 128, 100000, 400000, false, knobs, true);
        const bmx::PassPlan s0 = bmx::plan_candidate_pass(1, 4, 32, 256, 128, 30000, 100000, true, knobs);
        const bmx::PassPlan s1 = bmx::plan_candidate_pass(1, 4, 32, 256, 128, 30000, 100000, true, knobs, true);
        if (a.S != b.S || a.C != b.C || a.chunk_len != b.chunk_len || a.n_full != b.n_full || a.CS != b.CS) return 5;
        if (a.S != 24576 || c.S != BMX_ORDERED_SAMPLE || c.C != a.C || c.chunk_len != a.chunk_len || c.n_full != a.n_full) return 5;
        if (s0.S != BMX_SEEDED_SAMPLE || s1.S != s0.S) return 5;
    }
    FILE* o = fopen(argv[4], "wb");
    if (!o || fwrite(pos.data(), sizeof(int32_t), nr_pad, o) != (size_t)nr_pad) return 3;
    fclose(o);
    printf("buckets_used %d\n", used);
    return 0;
}
