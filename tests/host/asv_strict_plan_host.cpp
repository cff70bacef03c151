// Stand-alone host program (no HIP call): the scratch plan of adjust_shift_variance's strict mode (plan_asv_strict,
// csrc/asv_plan.hpp) for a table of inputs, one JSON object a line, with the invariants it must keep -- and, beside it, the
// call's own plan for the same inputs, which strict mode must leave as it is.  tests/test_cpu_asv_strict.py builds it with
// AddressSanitizer and UndefinedBehaviorSanitizer and holds the plans against tests/golden/asv_plan_parent.json.
#include <cstdio>
#include <cstring>

#include "asv_plan.hpp"

using bmx::AsvLiteralLayout;
using bmx::AsvPlan;
using bmx::AsvStrictPlan;
using bmx::DevKnobs;

struct Case {
    int g, n2, nr1, nr2, vrm;
    int fast, wide, chunk, cap;  // the testing knobs asv_fast, asv_wide, asv_chunk, asv_cap
};

// rows of tests/host/asv_plan_host.cpp (its tiled, exact and wide calls), and the chunk hook on a tiled call
static const Case kCases[] = {
    {50, 20001, 1000, 1000, 1, 0, 0, 0, -1},
    {256, 50000, 2000, 2000, 1, 0, 0, 0, -1},
    {50, 200, 0, 100, 0, 1, 0, 0, -1},
    {50, 200, 1, 100, 0, 1, 0, 0, -1},
    {50, 200, 129, 100, 0, 1, 0, 0, -1},
    {50, 200, 100, 0, 0, 1, 0, 0, -1},
    {50, 200, 0, 0, 0, 1, 0, 0, -1},
    {50, 1, 28, 101, 1, 1, 0, 0, -1},
    {1, 1237, 1003, 900, 0, 1, 0, 0, -1},
    {200, 1237, 1003, 900, 1, 1, 0, 0, -1},
    {200, 1237, 1003, 900, 0, 1, 0, 0, 64},
    {200, 1237, 1003, 900, 0, 1, 0, 0, 0},
    {100, 5000, 40000, 30000, 1, 0, 0, 0, -1},
    {100, 5000, 40000, 30000, 1, 0, 0, 0, 0},
    {50, 180000, 850000, 180000, 1, 0, 0, 0, -1},
    {50, 180000, 850000, 180000, 1, 0, 0, 0, 0},
    {50, 1000000, 3000000, 1000000, 1, 0, 0, 0, -1},
    {50, 20000, 1000, 1000, 1, 0, 0, 0, -1},      // exact: strict is a no-op, the plan is still defined
    {2000, 300, 100, 120, 0, 0, 1, 7, -1},        // wide by the hook, chunks of 7
    {50, 0, 10, 10, 0, 0, 0, 0, -1},              // no cell at all
};

struct Region {
    long long off, extent;
};

static bool regions_ok(const Region* r, int n, long long total) {
    for (int i = 0; i < n; ++i) {
        if (r[i].off < 0 || r[i].extent < 0 || r[i].off + r[i].extent > total) return false;
        if (i + 1 < n && r[i].off + r[i].extent > r[i + 1].off) return false;
    }
    return true;
}

static bool same(const AsvStrictPlan& a, const AsvStrictPlan& b) {
    return a.chunk == b.chunk && a.npad == b.npad && a.wide == b.wide && a.list == b.list && a.count == b.count &&
           a.modes == b.modes && a.doubles == b.doubles;
}

int main() {
    int bad = 0;
    for (const Case& c : kCases) {
        DevKnobs knobs;
        knobs.asv_fast = c.fast;
        knobs.asv_wide = c.wide;
        knobs.asv_chunk = c.chunk;
        knobs.asv_cap = c.cap;
        const AsvPlan p = bmx::plan_adjust_shift_variance(c.g, c.n2, c.nr1, c.nr2, c.vrm, knobs);
        const AsvStrictPlan s = bmx::plan_asv_strict(c.g, c.n2, c.nr1, c.nr2, knobs);
        std::printf("{\"g\": %d, \"n2\": %d, \"nr1\": %d, \"nr2\": %d, \"vect_row_major\": %d, \"asv_fast\": %d, \"asv_wide\": %d, "
                    "\"asv_chunk\": %d, \"asv_cap\": %d, \"plan\": {\"exact\": %d, \"wide\": %d, \"chunk\": %d, \"blocks\": %d, "
                    "\"npad\": %d, \"lcap\": %d, \"main_doubles\": %llu, \"extra_doubles\": %llu}, "
                    "\"strict\": {\"chunk\": %d, \"npad\": %d, \"wide\": %llu, \"list\": %llu, \"count\": %llu, \"modes\": %llu, "
                    "\"doubles\": %llu}}\n",
                    c.g, c.n2, c.nr1, c.nr2, c.vrm, c.fast, c.wide, c.chunk, c.cap, p.exact, p.wide, p.chunk, p.blocks, p.npad,
                    p.lcap, (unsigned long long)p.main_doubles, (unsigned long long)p.extra_doubles, s.chunk, s.npad,
                    (unsigned long long)s.wide, (unsigned long long)s.list, (unsigned long long)s.count,
                    (unsigned long long)s.modes, (unsigned long long)s.doubles);
        const AsvLiteralLayout L(c.nr2, s.npad);
        const long long per_cell = L.wide_per_cell(c.g);
        const long long cells = c.n2 > 1 ? c.n2 : 1;
        const Region r[] = {{(long long)s.wide, per_cell * s.chunk},
                            {(long long)s.list, (cells + 1) / 2},   // n2 int32
                            {(long long)s.count, 1},                // two uint32
                            {(long long)s.modes, (cells + 7) / 8}}; // n2 bytes
        bool ok = regions_ok(r, 4, (long long)s.doubles);
        // the chunk: at least one cell, at most the call's cells, within the budget unless that is the one cell, under the hook
        ok = ok && s.chunk >= 1 && s.chunk <= cells && s.npad == p.npad && s.npad >= c.nr1 && (s.npad & (s.npad - 1)) == 0;
        ok = ok && (s.chunk == 1 || (unsigned long long)per_cell * s.chunk * sizeof(double) <= bmx::ASV_STRICT_BUDGET_BYTES);
        if (c.chunk > 0) ok = ok && s.chunk <= c.chunk;
        // the wide tail of a chunk lies inside the chunk's part of the scratch
        ok = ok && L.wide_proj(c.g, s.chunk) + s.chunk <= per_cell * s.chunk;
        // a pure function: the same inputs give the same plan, and the knobs that choose the call's FORM do not enter
        DevKnobs other = knobs;
        other.asv_fast = !c.fast;
        other.asv_cap = c.cap == 0 ? -1 : 0;
        other.asv_modes = 12345;
        other.asv_strict = 1;
        ok = ok && same(s, bmx::plan_asv_strict(c.g, c.n2, c.nr1, c.nr2, knobs)) &&
             same(s, bmx::plan_asv_strict(c.g, c.n2, c.nr1, c.nr2, other));
        // ... and the call's own plan does not know about strict mode
        DevKnobs strict_knobs = knobs;
        strict_knobs.asv_strict = 1;
        const AsvPlan q = bmx::plan_adjust_shift_variance(c.g, c.n2, c.nr1, c.nr2, c.vrm, strict_knobs);
        ok = ok && std::memcmp(&p, &q, sizeof(p)) == 0;
        if (!ok) {
            std::printf("invariant broken in the line above\n");
            ++bad;
        }
    }
    // the hook "asv_chunk" is followed exactly wherever it is below what the budget allows
    for (int chunk : {1, 7, 300, 1003}) {
        DevKnobs knobs;
        knobs.asv_chunk = chunk;
        const AsvStrictPlan s = bmx::plan_asv_strict(100, 1003, 1237, 1003, knobs);
        if (s.chunk != chunk) {
            std::printf("asv_chunk = %d gives a chunk of %d\n", chunk, s.chunk);
            ++bad;
        }
    }
    {  // one cell's values beyond the whole budget: still a chunk of one
        const AsvStrictPlan s = bmx::plan_asv_strict(256, 1000, 1 << 30, 1 << 29, DevKnobs());
        if (s.chunk != 1) {
            std::printf("a cell beyond the budget gives a chunk of %d\n", s.chunk);
            ++bad;
        }
    }
    if (bad) return 1;
    std::printf("strict plan checks ok\n");
    return 0;
}
