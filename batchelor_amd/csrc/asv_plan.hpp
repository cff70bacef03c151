// adjust_shift_variance: which form a call runs, what scratch it needs and WHERE every piece of that scratch lies -- pure
// functions of the sizes and the testing knobs.  No HIP call and no HIP header: tests/host/asv_plan_host.cpp pins the plan and
// both layouts on the CPU.  The two layout structs are the one place that says what a workgroup's scratch holds: the plan
// sizes its allocation from them, the launchers (asv_literal.hip, asv_tile.hip) and the kernels take their pointers from them.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "host_basics.hpp"

#if defined(__HIPCC__)
#define BMX_ASV_HD __host__ __device__ inline
#else
#define BMX_ASV_HD inline
#endif

namespace bmx {

// ---- the literal wide form (asv_literal.hip: asv_wide_pairs) ------------------------------------------
constexpr int AW_C = 32;   // cells per tile
constexpr int AW_S = 64;   // streamed cells per tile
constexpr int AW_KC = 32;  // genes staged per step

// ---- the tiled form (asv_tile.hip) ----------------------------------------------------------------------
constexpr int AT_C = 16;        // cells per tile
constexpr int AT_R = 64;        // streamed cells per step
constexpr int AT_KC = 32;       // dimensions staged per step
constexpr int AT_NB = 2048;     // histogram bins
constexpr int AT_CAP = 2048;    // collected entries of the crossing bin
constexpr int AT_U = 8;         // scratch elements per thread and batch in the per-cell passes (two batches in flight)

constexpr int AT_NP = 2 * AT_R; // the stream is padded to whole pairs of steps (zero rows)
constexpr int AT_SM = 4 * AT_C * 6;  // doubles of the block-reduction area: six values per (wave, cell) after the stream (>= 256 threads)

BMX_ASV_HD int asv_tile_gp(int g) { return (g + AT_KC - 1) / AT_KC * AT_KC + 2; }
// 8-dimension blocks of a streamed row; 0: the staged form.  Round 6: a row carries two more columns behind its g coordinates
// -- 1 and its squared norm -- so that the distance chain's MFMAs deliver -|x_c - x_o|^2 / sigma directly (asv_tile_kernel)
BMX_ASV_HD int asv_tile_nb8(int g) { return g + 2 <= 128 ? (g + 2 + 7) / 8 : 0; }
// row stride of the gathered stream: whole 8-dimension blocks (zero filled) for the register-streamed form
BMX_ASV_HD int asv_tile_gs(int g) { return asv_tile_nb8(g) > 0 ? asv_tile_nb8(g) * 8 : g; }
BMX_ASV_HD size_t asv_tile_npad(size_t N) {
    const size_t p = (N + AT_NP - 1) / AT_NP * AT_NP;
    return p > (size_t)AT_NP ? p : (size_t)AT_NP;
}
// addends a chain of the literal re-run may keep (its sort buffer and two 16 KB bin arrays must fit the LDS beside the tile)
// (a power of two: the lists are padded to one for the sorting networks)
// (BASELINE config 5 at full size, sigma 0.1: 7 % of the root merge's cells keep more than 32 768 addends in a chain, 33 cells of
// the whole tree more than 65 536, none more than 131 072 -- at 4 % of the step's time for the longer lists)
inline int asv_tile_lcap_default(int) { return 131072; }
// ... of which this many are sorted in the LDS (beside the tile); longer lists are sorted where they lie, in global memory
BMX_ASV_HD int asv_tile_lsort(int g) { return g <= 128 ? 4096 : 2048; }
// doubles of the kernel's multi-purpose LDS region (see there)
BMX_ASV_HD int asv_tile_ub_doubles(int g, int lcap) {
    const int nb8 = asv_tile_nb8(g);
    int u = 2 * AT_CAP;
    const int ls = lcap < asv_tile_lsort(g) ? lcap : asv_tile_lsort(g);
    u = u > 2 * ls ? u : 2 * ls;
    const int a = nb8 > 8 ? 2 * nb8 * 2 * 64 : 0;
    return u > a ? u : a;
}
// doubles of a workgroup's lists: per cell (log-weight, flag) of the own batch, log-weight of the reference in restrict order,
// (projection, log-weight) of the reference sorted; three index lists
BMX_ASV_HD int64_t asv_tile_list_doubles(int lcap) { return (int64_t)AT_C * lcap * 5 + (3 * (int64_t)lcap + 1) / 2 + 1; }
inline size_t asv_tile_lds_bytes(int g, int lcap) {
    const int nb8 = asv_tile_nb8(g);
    return ((size_t)2 * AT_C * asv_tile_gp(g) + (size_t)asv_tile_ub_doubles(g, lcap) +
            (nb8 == 0 ? (size_t)AT_R * (AT_KC + 2) : 0) + 8 * AT_C + 32 + AT_SM) * sizeof(double) +
           (size_t)2 * AT_NB * sizeof(unsigned long long);
}

// The scratch of the tiled form.  Every member is an offset in DOUBLES.
//   per workgroup (from the workgroup's base, workgroup b starts at b * per_block):
//     SP  [blocks of 64 streamed cells][16 slots][64]  projections of every (cell, streamed cell) pair; a cell's slot rotates
//     SW  likewise                                     with the block number (at() below)
//     LO  [16][lcap][2]  literal re-run: (log-weight, counted-in-prob2 flag) of the own batch's kept addends, restrict order
//     LR  [16][lcap]     ... log-weights of the reference batch's kept addends in restrict order
//     LS  [16][lcap][2]  ... (projection, log-weight) of the reference batch's, sorted
//     GI  [3][lcap] int32  the index lists of one cell's three chains (own, restrict order, projection order), reused per cell
//     SO  [Nown / 64][4][64][4] float  the own batch's pairs as float codes (lcap > 0 only; Nown = nr2 padded like N)
//   the extra region, once per call (from its base, behind the workgroups' blocks):
//     S        [N][gs]  the streamed cells (own batch's restricted cells, then the reference's), zero rows up to N
//     snrm     [N] their squared norms, snrm_max: the largest of them
//     sid      [N] int32  cell ids of the own batch's rows (-1: reference / padding)
//     vect_rm  [n2][g]  a row-major copy of vect when it came column-major
//     tile_ctr, gbar  one unsigned each: the tile counter and the round barrier's arrival count
struct AsvTileLayout {
    int64_t N, Nown;  // streamed cells / the own batch's part of them, padded to whole pairs of steps (Nown: 0 without the re-run)
    int64_t SP, SW, LO, LR, LS, GI, SO, per_block;
    int64_t S, snrm, snrm_max, sid, vect_rm, tile_ctr, gbar, extra_doubles;

    BMX_ASV_HD AsvTileLayout(int g, int nr1, int nr2, int lcap, int n2, int vect_row_major) {
        N = (int64_t)asv_tile_npad((size_t)nr1 + (size_t)nr2);
        Nown = lcap > 0 ? (int64_t)asv_tile_npad((size_t)nr2) : 0;
        SP = 0;
        SW = SP + (int64_t)AT_C * N;
        LO = SW + (int64_t)AT_C * N;
        LR = LO + (int64_t)AT_C * lcap * 2;
        LS = LR + (int64_t)AT_C * lcap;
        GI = LS + (int64_t)AT_C * lcap * 2;
        SO = LO + asv_tile_list_doubles(lcap);
        per_block = SO + (int64_t)AT_C * Nown / 2;
        S = 0;
        snrm = S + N * asv_tile_gs(g);
        snrm_max = snrm + N;
        sid = snrm_max + 1;
        vect_rm = sid + (N + 1) / 2 + 2;
        const int64_t tail = vect_rm + (vect_row_major ? 0 : (int64_t)n2 * g);  // 16 doubles: the two device words sit at its end
        tile_ctr = tail + 12;
        gbar = tail + 14;
        extra_doubles = tail + 16;
    }
    // The rotated-slot address: element jlow of block jb (64 streamed cells) of the cell whose slot number plus the
    // workgroup's rotation is crot, in SP / SW.  A cell's slot inside a block's piece rotates with the block number: with a
    // fixed slot the per-cell passes walked the scratch at a stride of exactly 8 KB, through a handful of memory channels.
    BMX_ASV_HD static int64_t at(int crot, int jb, int jlow) {
        return (int64_t)jb * (AT_C * 64) + (((crot + jb) & (AT_C - 1)) << 6) + jlow;
    }
    // the float code of (streamed cell jlow of block jb, tile cell c) in SO: [block][c & 3][64][c >> 2], so that the stream
    // stores a lane's four cells c, c + 4, c + 8, c + 12 of one streamed cell as one 16-byte piece
    BMX_ASV_HD static int64_t so_at(int64_t jb, int jlow, int c) { return ((jb * 4 + (c & 3)) * 64 + jlow) * 4 + (c >> 2); }
};

// The scratch of the literal forms, per cell (the exact form: per workgroup), offsets in doubles:
//   lw2 [nr2] log-weights of the own batch's restricted cells, add2 [nr2] 1.0: the cell counts towards prob2,
//   kp / kw [npad] projection and log-weight of the reference batch's (npad = nr1 rounded up to a power of two, padded with
//   +inf so that the padding sorts last).
// The wide form keeps nc cells' values at once and behind them gradn [g][nc], l2 [nc], proj [nc].
struct AsvLiteralLayout {
    int64_t lw2, add2, kp, kw, per_cell;
    BMX_ASV_HD AsvLiteralLayout(int nr2, int npad) {
        lw2 = 0;
        add2 = lw2 + nr2;
        kp = add2 + nr2;
        kw = kp + npad;
        per_cell = kw + npad;
    }
    BMX_ASV_HD int64_t wide_gradn(int nc) const { return per_cell * nc; }
    BMX_ASV_HD int64_t wide_l2(int g, int nc) const { return wide_gradn(nc) + (int64_t)g * nc; }
    BMX_ASV_HD int64_t wide_proj(int g, int nc) const { return wide_l2(g, nc) + nc; }
    BMX_ASV_HD int64_t wide_per_cell(int g) const { return per_cell + g + 2; }  // (a chunk of nc cells: nc times this)
};

// What a call of these sizes runs and needs: the caller reserves main_doubles + extra_doubles of scratch and hands the same
// plan to the launch.
struct AsvPlan {
    int exact = 1;   // 1: asv_exact_kernel (the reference's order of operations literally), 0: the tiled FP64-MFMA form
    int wide = 0;    // 1 (with exact = 0): the literal wide form -- pair values in LDS-tiled passes, then the exact per-cell phase
    int chunk = 0;   // wide form: cells whose pair values sit in scratch at once
    int blocks = 1;  // workgroups
    int npad = 1;    // exact form: nr1 rounded up to a power of two
    int lcap = 0;    // tiled form: addends a chain of the literal re-run of a flagged cell may keep (0: no re-run)
    size_t main_doubles = 0, extra_doubles = 0;
};

// Which form runs and what it needs: a PURE function of the sizes and of the testing hooks "asv_fast", "asv_wide",
// "asv_chunk" and "asv_cap", so that the caller's allocation and the launch agree whatever happens to the free memory in
// between.  exact = 1: asv_exact_kernel (bit-exact walk; up to 131 072 restricted cells and 4e7 pairs); wide = 1: the literal
// wide form; neither: the tiled FP64-MFMA form, `blocks` workgroups of AsvTileLayout::per_block doubles each, behind them
// (`extra_doubles`) the layout's extra region.
inline AsvPlan plan_adjust_shift_variance(int g, int n2, int nr1, int nr2, int vect_row_major, const DevKnobs& knobs) {
    AsvPlan pl;
    // the bit-exact form's sequential log-sum chains cost ~1.6 ns per (cell, restricted cell) pair, the tiled form 0.015:
    // exact up to 4e7 pairs (the reference's own test shapes and anything a test can check against the CPU), tiled beyond
    pl.exact = !knobs.asv_fast && (int64_t)nr1 + nr2 <= 131072 && (double)std::max(n2, 1) * ((double)nr1 + nr2) <= 4e7;
    int p = 1;
    while (p < std::max(nr1, 1)) p <<= 1;
    pl.npad = p;
    const AsvLiteralLayout lit(nr2, p);
    // gene space beyond the exact form's size (the tiled form stops at 256 dimensions), or forced by the testing hook: the
    // literal wide form, the exact form's values chunk by chunk of cells
    // (also where the exact form's two gene vectors would not fit a workgroup's LDS: the wide form's values are its bits)
    if (knobs.asv_wide || (!pl.exact && g > 256) || (pl.exact && (size_t)2 * g * sizeof(double) > (size_t)160 * 1024)) {
        pl.exact = 0;
        pl.wide = 1;
        const size_t per_cell = (size_t)lit.wide_per_cell(g);
        const size_t budget = (size_t)1 << 27;  // doubles: 1 GiB of scratch at most
        pl.chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(n2, 1), budget / per_cell));
        if (knobs.asv_chunk > 0) pl.chunk = std::min(pl.chunk, knobs.asv_chunk);  // (testing hook "asv_chunk")
        pl.blocks = std::min(pl.chunk, 1024);
        pl.main_doubles = per_cell * (size_t)pl.chunk;
        pl.extra_doubles = 16;
        return pl;
    }
    if (pl.exact) {
        const size_t per_block = (size_t)lit.per_cell;
        const size_t budget = (size_t)1 << 27;  // doubles: 1 GiB of scratch at most
        pl.blocks = (int)std::max<size_t>(1, std::min<size_t>({(size_t)std::max(n2, 1), (size_t)1024, budget / std::max<size_t>(per_block, 1)}));
        pl.main_doubles = per_block * (size_t)pl.blocks;
        pl.extra_doubles = 16;
        return pl;
    }
    // the literal re-run of flagged cells keeps at most lcap addends per chain (testing hook "asv_cap": 0 = off, n = at most n)
    pl.lcap = asv_tile_lcap_default(g);
    {
        // a chain keeps addends of ONE batch's restricted cells: lists longer than the larger batch (as a power of two) are
        // never filled, and at 85 MB of list scratch per workgroup a call of a few thousand cells would ask for 22 GB
        int need = 1;
        while (need < std::max({nr1, nr2, 1})) need <<= 1;
        pl.lcap = std::min(pl.lcap, need);
    }
    if (knobs.asv_cap >= 0) {  // (rounded down to a power of two: the lists are padded to one)
        int c2 = 0;
        for (int b = 1; b > 0 && b <= knobs.asv_cap; b <<= 1) c2 = b;
        pl.lcap = std::min(pl.lcap, c2);
    }
    const AsvTileLayout L(g, nr1, nr2, pl.lcap, n2, vect_row_major);
    const size_t per_block = (size_t)L.per_block;
    const size_t budget = (size_t)12 << 30;  // doubles: 96 GiB of the 288 at most
    const size_t tiles = ((size_t)std::max(n2, 1) + AT_C - 1) / AT_C;
    pl.blocks = (int)std::max<size_t>(1, std::min<size_t>({tiles, (size_t)256, budget / per_block}));
    pl.main_doubles = per_block * (size_t)pl.blocks;
    pl.extra_doubles = (size_t)L.extra_doubles;
    return pl;
}

// ---- strict mode (var_adj_strict) ---------------------------------------------------------------------------------
// The tiled form records the way each cell of the call went (0 the histogram way, 1 re-run literally, 2 flagged but beyond
// the re-run), asv_strict_compact turns the record into the ascending list of the mode-2 cells, and the literal wide form
// recomputes exactly those, a chunk of the list at a time.  The scratch of that pass lies BEHIND the plan's own
// (main_doubles + extra_doubles) in the caller's reservation; offsets in doubles from there:
//   wide   [chunk * wide_per_cell]  AsvLiteralLayout per cell of a chunk and the wide tail (asv_literal.hip)
//   list   [n2] int32               the mode-2 cells of the call's cell range, ascending
//   count  2 uint32                 cells in the list, cells re-run literally (mode 1)
//   modes  [n2] uint8               the record, indexed by cell
// A pure function of (g, n2, nr1, nr2), the byte budget below and the testing hook "asv_chunk".
constexpr size_t ASV_STRICT_BUDGET_BYTES = (size_t)32 << 30;  // of pair values in flight (adjust_shift_variance, strict mode)

struct AsvStrictPlan {
    int chunk = 1;  // cells of the list whose pair values sit in scratch at once (>= 1)
    int npad = 1;   // nr1 rounded up to a power of two, as the plan's
    size_t wide = 0, list = 0, count = 0, modes = 0, doubles = 0;
};

inline AsvStrictPlan plan_asv_strict(int g, int n2, int nr1, int nr2, const DevKnobs& knobs) {
    AsvStrictPlan sp;
    int p = 1;
    while (p < std::max(nr1, 1)) p <<= 1;
    sp.npad = p;
    const size_t per_cell = (size_t)AsvLiteralLayout(nr2, p).wide_per_cell(g);
    const size_t cells = (size_t)std::max(n2, 1);
    sp.chunk = (int)std::max<size_t>(1, std::min<size_t>(cells, ASV_STRICT_BUDGET_BYTES / sizeof(double) / per_cell));
    if (knobs.asv_chunk > 0) sp.chunk = std::min(sp.chunk, knobs.asv_chunk);  // (testing hook "asv_chunk")
    sp.wide = 0;
    sp.list = sp.wide + per_cell * (size_t)sp.chunk;
    sp.count = sp.list + (cells + 1) / 2;
    sp.modes = sp.count + 1;
    sp.doubles = sp.modes + (cells + 7) / 8;
    return sp;
}

}  // namespace bmx
