// Stand-alone host program (no HIP call): prints the plan of a candidate pass (csrc/knn_plan.hpp) for a table of shapes, one
// JSON object a line, and checks the invariants every plan must keep.  tests/test_cpu_knn_plan.py builds it with
// AddressSanitizer and UndefinedBehaviorSanitizer and compares the lines with tests/golden/knn_plan_parent.json.
#include <cstdio>
#include <cstring>

#include "knn_plan.hpp"

using bmx::DevKnobs;
using bmx::PassPlan;

struct Shape {
    int tier, NS, KS, unit, rows_per_slot, nq, nr, seeded;
    const char* knob;  // one testing knob set for the row ("" = none)
    int value;
};

static const Shape kShapes[] = {
    {1, 4, 32, 256, 128, 100000, 400000, 0, "", 0},  // whole-range round plus split tail
    {1, 4, 32, 256, 128, 12500, 100000, 0, "", 0},   // sample split
    {1, 4, 32, 256, 128, 3000, 3000, 0, "", 0},      // no sample, one range
    {1, 4, 32, 256, 128, 500, 5000, 0, "", 0},
    {1, 4, 32, 256, 128, 70000, 20000, 0, "", 0},
    {1, 4, 32, 256, 128, 65536, 9000, 0, "", 0},     // b = 0
    {1, 4, 48, 256, 64, 20000, 100000, 0, "", 0},
    {1, 7, 32, 256, 64, 20000, 100000, 0, "", 0},    // NS > 4 sample cap
    {1, 4, 32, 256, 128, 30000, 100000, 1, "", 0},
    {2, 10, 24, 256, 32, 20000, 100000, 0, "", 0},
    {2, 10, 24, 256, 32, 20000, 20000, 0, "", 0},
    {2, 16, 24, 128, 32, 1200, 2500, 0, "", 0},
    // the first shape with each knob
    {1, 4, 32, 256, 128, 100000, 400000, 0, "sample", 0},
    {1, 4, 32, 256, 128, 100000, 400000, 0, "sample", 1024},
    {1, 4, 32, 256, 128, 100000, 400000, 0, "split_c", 3},
    {1, 4, 32, 256, 128, 100000, 400000, 0, "force_c", 2},
    {1, 4, 32, 256, 128, 100000, 400000, 0, "sample_split", 0},
    {1, 4, 32, 256, 128, 100000, 400000, 0, "sample_split", 4},
    {1, 4, 32, 256, 128, 100000, 400000, 0, "no_margin", 1},
    // the knobs of the sample split where the split is on (49 query blocks)
    {1, 4, 32, 256, 128, 12500, 100000, 0, "sample_split", 0},
    {1, 4, 32, 256, 128, 12500, 100000, 0, "sample_split", 4},
    {1, 4, 32, 256, 128, 12500, 100000, 0, "no_margin", 1},
    // 258 query blocks against a reference that only splits in two; a forced sample beyond the reference; limits of C
    {1, 1, 32, 256, 256, 66000, 4200, 0, "", 0},
    {1, 4, 32, 256, 128, 3000, 3000, 0, "sample", 1000000},
    {1, 4, 32, 256, 128, 100000, 400000, 0, "force_c", 99},
    {1, 4, 32, 256, 128, 300, 400000, 0, "", 0},
    {2, 10, 24, 256, 32, 30000, 100000, 1, "", 0},
    {2, 4, 40, 128, 32, 40000, 50000, 0, "", 0},
};

static bool set_knob(DevKnobs& k, const char* name, int v) {
    if (!*name) return true;
    if (!std::strcmp(name, "sample")) k.sample = v;
    else if (!std::strcmp(name, "split_c")) k.split_c = v;
    else if (!std::strcmp(name, "force_c")) k.force_c = v;
    else if (!std::strcmp(name, "sample_split")) k.sample_split = v;
    else if (!std::strcmp(name, "no_margin")) k.no_margin = v;
    else return false;
    return true;
}

int main() {
    int bad = 0;
    for (const Shape& s : kShapes) {
        DevKnobs knobs;
        if (!set_knob(knobs, s.knob, s.value)) {
            std::printf("unknown knob %s\n", s.knob);
            return 2;
        }
        const PassPlan p = bmx::plan_candidate_pass(s.tier, s.NS, s.KS, s.unit, s.rows_per_slot, s.nq, s.nr, s.seeded != 0, knobs);
        std::printf("{\"tier\": %d, \"NS\": %d, \"KS\": %d, \"unit\": %d, \"rows_per_slot\": %d, \"nq\": %d, \"nr\": %d, "
                    "\"seeded\": %d, \"knob\": \"%s\", \"value\": %d, \"plan\": {\"unit\": %d, \"nq_pad\": %d, \"nqb\": %d, "
                    "\"S\": %d, \"CS\": %d, \"sample_range_len\": %d, \"sample_nranges\": %d, \"C\": %d, \"chunk_len\": %d, "
                    "\"nr_pad\": %d, \"n_full\": %d}}\n",
                    s.tier, s.NS, s.KS, s.unit, s.rows_per_slot, s.nq, s.nr, s.seeded, s.knob, s.value, p.unit, p.nq_pad, p.nqb,
                    p.S, p.CS, p.sample_range_len, p.sample_nranges, p.C, p.chunk_len, p.nr_pad, p.n_full);
        const bool ok = p.chunk_len % s.rows_per_slot == 0 && (long long)p.C * p.chunk_len >= s.nr && p.C >= 1 && p.C <= 7 &&
                        p.S <= p.nr_pad && p.n_full % 256 == 0 && p.n_full <= p.nqb &&
                        (long long)p.sample_nranges * p.sample_range_len >= p.S && p.nr_pad == p.C * p.chunk_len;
        if (!ok) {
            std::printf("invariant broken in the line above\n");
            ++bad;
        }
    }
    if (bad) return 1;
    std::printf("plan checks ok\n");
    return 0;
}
