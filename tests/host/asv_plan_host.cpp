// Stand-alone host program (no HIP call): prints the plan of adjust_shift_variance and the offsets of its two scratch
// layouts (csrc/asv_plan.hpp) for a table of inputs, one JSON object a line, and checks the invariants every layout must
// keep.  tests/test_cpu_asv_plan.py builds it with AddressSanitizer and UndefinedBehaviorSanitizer and compares the lines
// with tests/golden/asv_plan_parent.json.
#include <cstdio>
#include <cstring>

#include "asv_plan.hpp"

using bmx::AsvLiteralLayout;
using bmx::AsvPlan;
using bmx::AsvTileLayout;
using bmx::DevKnobs;

struct Case {
    int g, n2, nr1, nr2, vrm;
    int fast, wide, chunk, cap;  // the testing knobs asv_fast, asv_wide, asv_chunk, asv_cap
};

static const Case kCases[] = {
    // ---- each form and each switch between them
    {50, 20000, 1000, 1000, 1, 0, 0, 0, -1},       // 4e7 pairs exactly: the exact form
    {50, 20001, 1000, 1000, 1, 0, 0, 0, -1},       // one cell more: tiled
    {50, 100, 65536, 65536, 1, 0, 0, 0, -1},       // 131 072 restricted cells: exact
    {50, 100, 65536, 65537, 1, 0, 0, 0, -1},       // one more: tiled
    {256, 50000, 2000, 2000, 1, 0, 0, 0, -1},      // 2e8 pairs at 256 dimensions: tiled (the staged form)
    {257, 50000, 2000, 2000, 1, 0, 0, 0, -1},      // 257: the wide form
    {10240, 100, 50, 50, 0, 0, 0, 0, -1},          // the exact form's two gene vectors fill 160 KB of LDS
    {10241, 100, 50, 50, 0, 0, 0, 0, -1},          // ... and no longer fit: wide
    {2000, 300, 100, 120, 0, 0, 1, 0, -1},         // wide by the hook
    {2000, 300, 100, 120, 0, 0, 1, 7, -1},         // ... in chunks of 7 cells
    {2000, 5, 100, 120, 0, 0, 1, 7, -1},           // ... fewer cells than a chunk
    {20000, 100000, 3000, 3000, 1, 0, 0, 0, -1},   // wide, the chunk set by the 1 GiB budget
    {20000, 100000, 3000, 3000, 1, 0, 0, 7, -1},
    // ---- nr1 = 0, 1 and powers of two +- 1; nr2 = 0 -- the exact form
    {50, 200, 0, 100, 0, 0, 0, 0, -1},
    {50, 200, 1, 100, 0, 0, 0, 0, -1},
    {50, 200, 2, 100, 0, 0, 0, 0, -1},
    {50, 200, 3, 100, 0, 0, 0, 0, -1},
    {50, 200, 127, 100, 0, 0, 0, 0, -1},
    {50, 200, 128, 100, 0, 0, 0, 0, -1},
    {50, 200, 129, 100, 0, 0, 0, 0, -1},
    {50, 200, 1023, 100, 1, 0, 0, 0, -1},
    {50, 200, 1024, 100, 1, 0, 0, 0, -1},
    {50, 200, 1025, 100, 1, 0, 0, 0, -1},
    {50, 200, 100, 0, 0, 0, 0, 0, -1},
    {50, 200, 0, 0, 0, 0, 0, 0, -1},
    {50, 0, 10, 10, 0, 0, 0, 0, -1},
    // ---- the same under asv_fast: the tiled form
    {50, 200, 0, 100, 0, 1, 0, 0, -1},
    {50, 200, 1, 100, 0, 1, 0, 0, -1},
    {50, 200, 2, 100, 0, 1, 0, 0, -1},
    {50, 200, 3, 100, 0, 1, 0, 0, -1},
    {50, 200, 127, 100, 0, 1, 0, 0, -1},
    {50, 200, 128, 100, 0, 1, 0, 0, -1},
    {50, 200, 129, 100, 0, 1, 0, 0, -1},
    {50, 200, 1023, 100, 1, 1, 0, 0, -1},
    {50, 200, 1024, 100, 1, 1, 0, 0, -1},
    {50, 200, 1025, 100, 1, 1, 0, 0, -1},
    {50, 200, 100, 0, 0, 1, 0, 0, -1},
    {50, 200, 0, 0, 0, 1, 0, 0, -1},
    {50, 1, 28, 101, 1, 1, 0, 0, -1},
    // ---- the stream forms: NB8 = 1, 8, 9, 16 and the staged form at its first and last width
    {1, 1237, 1003, 900, 0, 1, 0, 0, -1},
    {62, 1237, 1003, 900, 0, 1, 0, 0, -1},
    {63, 1237, 1003, 900, 0, 1, 0, 0, -1},
    {126, 1237, 1003, 900, 0, 1, 0, 0, -1},
    {127, 1237, 1003, 900, 0, 1, 0, 0, -1},
    {200, 1237, 1003, 900, 1, 1, 0, 0, -1},
    {256, 1237, 1003, 900, 0, 1, 0, 0, -1},
    {256, 1237, 1003, 900, 1, 1, 0, 0, -1},
    // ---- asv_cap
    {100, 5000, 40000, 30000, 1, 0, 0, 0, -1},
    {100, 5000, 40000, 30000, 1, 0, 0, 0, 0},
    {100, 5000, 40000, 30000, 1, 0, 0, 0, 1},
    {100, 5000, 40000, 30000, 1, 0, 0, 0, 64},
    {100, 5000, 40000, 30000, 1, 0, 0, 0, 100},
    {200, 1237, 1003, 900, 0, 1, 0, 0, 64},
    {200, 1237, 1003, 900, 0, 1, 0, 0, 0},
    // ---- config 5's root merge; a call whose workgroups the 96 GiB budget limits, not its tiles
    {50, 180000, 850000, 180000, 1, 0, 0, 0, -1},
    {50, 180000, 850000, 180000, 1, 0, 0, 0, 0},
    {50, 1000000, 3000000, 1000000, 1, 0, 0, 0, -1},
    {50, 1000000, 3000000, 1000000, 0, 0, 0, 0, -1},
};

struct Region {
    const char* name;
    long long off, extent;
};

// every region inside [0, total), in ascending order, none reaching into the next
static bool regions_ok(const Region* r, int n, long long total) {
    for (int i = 0; i < n; ++i) {
        if (r[i].off < 0 || r[i].extent < 0 || r[i].off + r[i].extent > total) return false;
        if (i + 1 < n && r[i].off + r[i].extent > r[i + 1].off) return false;
    }
    return true;
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
        std::printf("{\"g\": %d, \"n2\": %d, \"nr1\": %d, \"nr2\": %d, \"vect_row_major\": %d, \"asv_fast\": %d, \"asv_wide\": %d, "
                    "\"asv_chunk\": %d, \"asv_cap\": %d, \"plan\": {\"exact\": %d, \"wide\": %d, \"chunk\": %d, \"blocks\": %d, "
                    "\"npad\": %d, \"lcap\": %d, \"main_doubles\": %llu, \"extra_doubles\": %llu}, ",
                    c.g, c.n2, c.nr1, c.nr2, c.vrm, c.fast, c.wide, c.chunk, c.cap, p.exact, p.wide, p.chunk, p.blocks, p.npad,
                    p.lcap, (unsigned long long)p.main_doubles, (unsigned long long)p.extra_doubles);
        bool ok = p.blocks >= 1;
        if (p.exact || p.wide) {
            const AsvLiteralLayout L(c.nr2, p.npad);
            const int nc = p.wide ? p.chunk : 0;
            std::printf("\"literal\": {\"lw2\": %lld, \"add2\": %lld, \"kp\": %lld, \"kw\": %lld, \"per_cell\": %lld, "
                        "\"gradn\": %lld, \"l2\": %lld, \"proj\": %lld}}\n",
                        (long long)L.lw2, (long long)L.add2, (long long)L.kp, (long long)L.kw, (long long)L.per_cell,
                        (long long)L.wide_gradn(nc), (long long)L.wide_l2(c.g, nc), (long long)L.wide_proj(c.g, nc));
            const Region cell[] = {{"lw2", L.lw2, c.nr2}, {"add2", L.add2, c.nr2}, {"kp", L.kp, p.npad}, {"kw", L.kw, p.npad}};
            ok = ok && regions_ok(cell, 4, L.per_cell) && p.npad >= c.nr1 && (p.npad & (p.npad - 1)) == 0;
            if (p.wide) {
                const Region tail[] = {{"cells", 0, L.per_cell * nc},
                                       {"gradn", L.wide_gradn(nc), (long long)c.g * nc},
                                       {"l2", L.wide_l2(c.g, nc), nc},
                                       {"proj", L.wide_proj(c.g, nc), nc}};
                ok = ok && regions_ok(tail, 4, (long long)p.main_doubles) && p.chunk >= 1 && p.blocks <= p.chunk;
            } else {
                ok = ok && (long long)p.main_doubles == L.per_cell * p.blocks;
            }
        } else {
            const AsvTileLayout L(c.g, c.nr1, c.nr2, p.lcap, c.n2, c.vrm);
            std::printf("\"tile\": {\"N\": %lld, \"Nown\": %lld, \"SP\": %lld, \"SW\": %lld, \"LO\": %lld, \"LR\": %lld, \"LS\": %lld, "
                        "\"GI\": %lld, \"SO\": %lld, \"per_block\": %lld, \"S\": %lld, \"snrm\": %lld, \"snrm_max\": %lld, "
                        "\"sid\": %lld, \"vect_rm\": %lld, \"tile_ctr\": %lld, \"gbar\": %lld, \"extra_doubles\": %lld, "
                        "\"lds_bytes\": %llu}}\n",
                        (long long)L.N, (long long)L.Nown, (long long)L.SP, (long long)L.SW, (long long)L.LO, (long long)L.LR,
                        (long long)L.LS, (long long)L.GI, (long long)L.SO, (long long)L.per_block, (long long)L.S,
                        (long long)L.snrm, (long long)L.snrm_max, (long long)L.sid, (long long)L.vect_rm, (long long)L.tile_ctr,
                        (long long)L.gbar, (long long)L.extra_doubles, (unsigned long long)bmx::asv_tile_lds_bytes(c.g, p.lcap));
            const long long lc = p.lcap;
            const Region wg[] = {{"SP", L.SP, bmx::AT_C * L.N},  {"SW", L.SW, bmx::AT_C * L.N},
                                 {"LO", L.LO, bmx::AT_C * lc * 2}, {"LR", L.LR, bmx::AT_C * lc},
                                 {"LS", L.LS, bmx::AT_C * lc * 2}, {"GI", L.GI, (3 * lc + 1) / 2},  // 3 lcap int32
                                 {"SO", L.SO, bmx::AT_C * L.Nown / 2}};                               // 16 Nown floats
            const Region ex[] = {{"S", L.S, L.N * bmx::asv_tile_gs(c.g)},
                                 {"snrm", L.snrm, L.N},
                                 {"snrm_max", L.snrm_max, 1},
                                 {"sid", L.sid, (L.N + 1) / 2},  // N int32
                                 {"vect_rm", L.vect_rm, c.vrm ? 0 : (long long)c.n2 * c.g},
                                 {"tile_ctr", L.tile_ctr, 1},
                                 {"gbar", L.gbar, 1}};
            ok = ok && regions_ok(wg, 7, L.per_block) && regions_ok(ex, 7, L.extra_doubles) &&
                 (long long)p.main_doubles == L.per_block * p.blocks && (long long)p.extra_doubles == L.extra_doubles &&
                 L.N >= (long long)c.nr1 + c.nr2 && L.N % bmx::AT_NP == 0 && (p.lcap & (p.lcap - 1)) == 0 && p.blocks <= 256 &&
                 p.main_doubles <= ((size_t)12 << 30) && bmx::asv_tile_lds_bytes(c.g, p.lcap) <= (size_t)160 * 1024;
        }
        if (!ok) {
            std::printf("invariant broken in the line above\n");
            ++bad;
        }
    }
    // the tile kernel's LDS fits a workgroup's 160 KB at every width the tiled form takes
    for (int g = 1; g <= 256; ++g)
        if (bmx::asv_tile_lds_bytes(g, bmx::asv_tile_lcap_default(g)) > (size_t)160 * 1024) {
            std::printf("asv_tile_lds_bytes(%d) beyond 160 KB\n", g);
            ++bad;
        }
    if (bad) return 1;
    std::printf("plan checks ok\n");
    return 0;
}
