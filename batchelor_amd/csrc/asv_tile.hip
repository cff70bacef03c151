// adjust_shift_variance at scale: the tiled FP64-MFMA form (asv.hip says when it runs).  One kernel, asv_tile_kernel<NB8>,
// a sequence of phases per tile of 16 cells; in front of it the gathered stream (asv_gather_stream, asv_max_norm); behind it
// the per-device tallies and phase ticks that tests and bench.py read.  AsvTileLayout (asv_plan.hpp) says where everything
// in a workgroup's scratch lies.
#include "asv_internal.hpp"

#include <algorithm>
#include <mutex>
#include <type_traits>

namespace bmx {
namespace {

constexpr int T = ASV_T;
typedef double d4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------
// adjust_shift_variance at scale (BASELINE.json configs[4]: every right cell of a merge against every restricted cell of
// both batches -- 5e11 pairs at the root of the 16-batch tree).  A workgroup owns a TILE OF 16 CELLS:
//   1. the restricted cells of both batches, gathered into one zero-padded matrix (asv_gather_stream), stream past it once:
//      every wave loads its 16 rows of a 64-row step straight into MFMA operand registers (LDS-staged beyond 128
//      dimensions); two FP64 MFMA chains (v_mfma_f64_16x16x4_f64) per 16 x 16 sub-tile give  D = x_c . x_o  and
//      P = g^_c . x_o, from which the projection on the cell's line (P) and the squared distance to it
//      |x_c|^2 + |x_o|^2 - 2 D - (g^_c . x_c - P)^2  follow per pair (src/adjust_shift_variance.cpp:9-27 in GEMM form);
//      projection and log-weight go to the tile's scratch, the per-cell maxima / projection range come out of the same pass;
//   2. cell by cell: the own-batch probability (log-sum-exp, :74-112) and the weighted quantile of the reference batch's
//      projections (:117-157) WITHOUT sorting them: linear histogram of the weights over the projection range (2 048
//      bins, integer fixed-point sums: order-independent, so runs are bit-identical), the bin where the cumulative weight
//      crosses the target is collected, sorted and walked; a bin that is still too full is subdivided again.
// Weights are taken relative to the cell's largest one and kept to 2^-40: a reference cell 28 sigma2 further from the line
// than the nearest contributes nothing, as in FP64 it would not either beyond 37.  Cells whose walk is decided on the last
// bits may pick the neighbouring quantile (asv_exact_kernel is the bit-exact form, taken up to 4e7 pairs).
// ---------------------------------------------------------------------------------------------------
// The weighted-quantile walk (src/adjust_shift_variance.cpp:137-157: the first entry at which the cumulative weight reaches
// the target) over up to 8 T integer weights in the LDS, by the whole block instead of one thread going entry by entry:
// every thread sums its eight consecutive entries, a scan over the threads gives each its starting weight, the thread whose
// stretch holds the first crossing reports it.  Integer sums: the result is what the sequential walk finds.
// target_of(total weight of v) -> target.  Returns the index (-1: never reached), *cum_before = base + weight before it.
template <class TargetOf>
__device__ __forceinline__ int asv_first_crossing(const unsigned long long* v, int n, unsigned long long base,
                                                  TargetOf target_of, unsigned long long* smu, int* sh_idx,
                                                  unsigned long long* sh_cum, double* target_out) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i0 = tid * 8;
    unsigned long long mine[8], loc = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        mine[k] = i0 + k < n ? v[i0 + k] : 0ull;
        loc += mine[k];
    }
    unsigned long long inc = loc;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    __syncthreads();  // (smu may still be read as something else)
    if (lane == 63) smu[w] = inc;
    if (tid == 0) *sh_idx = 0x7fffffff;
    __syncthreads();
    unsigned long long woff = 0, total = 0;
    for (int ww = 0; ww < T / 64; ++ww) {
        const unsigned long long t = smu[ww];
        total += t;
        if (ww < w) woff += t;
    }
    const double target = target_of(total);
    unsigned long long cum = base + woff + (inc - loc), cbefore = 0;
    int cand = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const bool hit = cand == 0x7fffffff && i0 + k < n && (double)(cum + mine[k]) >= target;
        cbefore = hit ? cum : cbefore;
        cand = hit ? i0 + k : cand;
        cum += mine[k];
    }
    if (cand != 0x7fffffff) atomicMin(sh_idx, cand);
    __syncthreads();
    if (cand == *sh_idx && cand != 0x7fffffff) *sh_cum = cbefore;
    __syncthreads();
    *target_out = target;
    return *sh_idx == 0x7fffffff ? -1 : *sh_idx;
}

// One cell's scratch row, elements [jstart, jstart + n) of the stream, past the block: thread t visits jstart + t,
// + T, ... in batches of AT_U, the next batch on its way while the current one is consumed (one wave per SIMD: nothing
// else hides the round trip to the scratch).  Straight-line code: every load is issued (block numbers clamped to the
// row's last block) and `proc` gets the element number to tell the ones beyond n -- with the loads or their first use
// under per-element branches the compiler waited for ALL outstanding loads before the first use: no overlap at all.
// So `proc` should select, not branch, on what it was given.
// Layout: AsvTileLayout::at (crot = the cell's slot number plus the workgroup's rotation).
template <bool WITH_W, class Proc>
__device__ __forceinline__ void asv_row_scan(const double* __restrict__ P, const double* __restrict__ W, int64_t jstart,
                                             int n, int crot, int last_block, int tid, Proc proc) {
    const int64_t jt = jstart + tid;
    const int jlow = (int)(jt & 63), jb_t = (int)(jt >> 6);
    double pa[AT_U], wa[AT_U], pb[AT_U], wb[AT_U];
    auto fetch = [&](double (&p)[AT_U], double (&w)[AT_U], int o0) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < AT_U; ++u) {
            const int o = o0 + u * T;  // (o - tid is a multiple of T = 4 blocks)
            int jb = jb_t + ((o - tid) >> 6);
            jb = jb < last_block ? jb : last_block;
            const int64_t off = AsvTileLayout::at(crot, jb, jlow);
            p[u] = P[off];
            w[u] = WITH_W ? W[off] : 0.0;
        }
    };
    auto consume = [&](const double (&p)[AT_U], const double (&w)[AT_U], int o0) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < AT_U; ++u) proc(p[u], w[u], o0 + u * T);
    };
    fetch(pa, wa, tid);
    for (int o0 = tid; o0 < n; o0 += 2 * AT_U * T) {
        fetch(pb, wb, o0 + AT_U * T);
        consume(pa, wa, o0);
        fetch(pa, wa, o0 + 2 * AT_U * T);
        consume(pb, wb, o0 + AT_U * T);
    }
}

// ---------------------------------------------------------------------------------------------------
// The literal re-run of the cells whose quantile walk is decided by rounding (the "flagged" cells of asv_tile_kernel).
//
// The reference sums its weights by sequential R::logspace_add chains (src/adjust_shift_variance.cpp:96-109, :127-131,
// :147-151).  Where the bandwidth is small against the squared distances, a cell's own log-weight (0) dwarfs the rest of
// its batch, prob2 - totalprob2 is below an ulp of totalprob1, the target of the walk IS totalprob1 (or an ulp or two
// below it) and the walk ends where the cumulative chain over the SORTED reference cells first reaches what the chain in
// RESTRICT order ended at: a statement about the rounding of two summation orders, which only the chains themselves
// reproduce.  But in exactly that regime almost every addend of a chain is an exact no-op:
//
//   Lemma.  Let acc be a chain's running value, known to lie in [L, U] with L, U of one sign, and 2^e <= min(|L|, |U|).
//   An addend lw < L + (e - 54) ln 2 - 1/4 leaves it unchanged: logspace_add(acc, lw) = acc + log1p(exp(lw - acc)), the
//   second term is <= exp(lw - L) < 2^(e - 54) e^(-1/4), less than a quarter of the spacing of doubles at |acc| >= 2^e (half
//   of it just below a power of two, towards zero) -- the sum rounds to acc; the few-ulp errors of the portable exp / log1p
//   are inside the factor e^(-1/4).  An addend lw <= acc - 700 is a no-op outright: the portable exp returns 0 there.
//
// acc is bounded from what has gone by: it is >= the largest addend so far (M) and <= M + log(count); once the cell's own
// weight 1 has gone by it is log(1 + sum of the others) in [log1p(e^Mx), log1p(count e^Mx)], Mx the largest other addend.
// A chain restricted to the addends the lemma does not exclude therefore has, by induction over its steps, the SAME bits
// as the full chain -- and keeping more addends than necessary (bounds from an earlier point of the sequence, margins for
// the matrix-core form's rounding of lw) is harmless: every addend that is left out is individually a no-op.
// So, per flagged cell: (i) the kept addends of the three chains are picked from the tile's scratch (values in GEMM form,
// margins `mb` / `tolp` for their rounding) -- in restrict order for totalprob2 / prob2 (:96-109) and totalprob1 (:127-131),
// in projection order for the walk (:147-151), where "what has gone by" is taken per histogram bin, two bins back; (ii)
// for those few the projection and the distance to the line are recomputed in the reference's own order of operations
// (:9-27, :88-89, :120-123), sorted as std::sort sorts the pairs (:134); (iii) one lane per chain repeats the reference's
// sequential sums with the bit-reproducible exp / log1p.  Every such cell is bit-equal to what a CPU following the
// reference's order of operations gets -- whatever the size of the call.  A cell that keeps more than `lcap` addends in
// any chain (bandwidths of the order of the squared distances: nearly every pair carries weight) goes the histogram
// way, which there resolves the quantile to 2^-40 of the total weight.
// ---------------------------------------------------------------------------------------------------
constexpr double AT_LN2 = 0.6931471805599453;


// addends below the returned value cannot change a chain whose running value lies in [L, U] (the lemma above)
__device__ __forceinline__ double asv_noop_below(double L, double U) {
    double t = L - 701.0;  // (portable exp: 0 for arguments <= -700)
    if ((L > 0.0 && U > 0.0) || (L < 0.0 && U < 0.0)) {
        const double amin = fmin(fabs(L), fabs(U));
        t = fmax(t, L + (double)(ilogb(amin) - 54) * AT_LN2 - 0.25);
    }
    return t;
}

// Thresholds of a chain from what has gone by (addends below them are no-ops), for the two regimes of a chain:
//  * running value below zero (a reference chain; an own-batch chain until the cell's own weight 1 arrives): it is >= the
//    largest addend so far (lo) and never exceeds hi + log(count), hi >= every addend the chain can have met by then;
//  * the cell itself has gone by: the chain stands at log(1 + the others' weights) >= log1p(exp(largest other so far)), and
//    only grows -- away from zero, towards coarser spacing.
// mb >= the rounding of the GEMM-form log-weights the bounds are taken from.
__device__ __forceinline__ double asv_thr_neg(double lo, double hi, double cnt, double mb) {
    if (lo == -__builtin_inf()) return lo;  // nothing has gone by: the next addend starts the chain
    return asv_noop_below(lo - mb, fmax(lo, hi) + mb + log(cnt) + 0.01) - mb;
}
__device__ __forceinline__ double asv_thr_self(double others, double mb) {
    // (no other addend yet: the chain stands at 0 exactly, only exp's underflow makes a no-op)
    const double L = others == -__builtin_inf() ? 0.0 : log1p(exp(others - mb)) * (1.0 - 1e-9);
    return asv_noop_below(L, L) - mb;
}

// Bitonic sort of a[0, np2) (np2 a power of two) in GLOBAL memory by the whole block, through an LDS window of B elements
// (B a power of two): every stage whose partners lie inside an aligned window runs there (a window is loaded, taken through
// all such steps, stored), only the steps that reach across windows (j >= B) go to global memory one by one.  A list of
// 32 768 pairs: 4 window rounds + 6 global steps instead of 120 global passes.  less(x, y): x sorts in front of y.
template <class E, class Less>
__device__ __forceinline__ void asv_sort_global(E* a, int np2, E* win, int B, int tid, Less less) {
    auto pass_done = [&]() {  // what the other threads of the block wrote must be what the next step reads
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");
    };
    if (B > np2) B = np2;
    // the steps j = jtop, jtop / 2, ..., 1 of stage k inside every window (jtop < B)
    auto windows = [&](int k_lo, int k_hi, bool all_steps) {
        for (int w0 = 0; w0 < np2; w0 += B) {
            for (int i = tid; i < B; i += T) win[i] = a[w0 + i];
            __syncthreads();
            for (int k = k_lo; k <= k_hi; k <<= 1)
                for (int j = all_steps ? (k >> 1) : (B >> 1); j > 0; j >>= 1) {
                    for (int p = tid; p < B / 2; p += T) {
                        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), q = i | j;
                        const E x = win[i], y = win[q];
                        const bool up = ((w0 + i) & k) == 0;
                        if (up ? less(y, x) : less(x, y)) {
                            win[i] = y;
                            win[q] = x;
                        }
                    }
                    __syncthreads();
                }
            for (int i = tid; i < B; i += T) a[w0 + i] = win[i];
            __syncthreads();
        }
        pass_done();
    };
    pass_done();
    windows(2, B, true);  // every stage k <= B: all its steps stay inside a window
    for (int k = 2 * B; k <= np2; k <<= 1) {
        for (int j = k >> 1; j >= B; j >>= 1) {
#pragma unroll 4
            for (int p = tid; p < np2 / 2; p += T) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), q = i | j;
                const E x = a[i], y = a[q];
                const bool sw = ((i & k) == 0) ? less(y, x) : less(x, y);
                a[i] = sw ? y : x;
                a[q] = sw ? x : y;
            }
            pass_done();
        }
        windows(k, k, false);  // the rest of stage k: steps j < B
    }
}

// asv_row_scan in PIECES with a block-wide step in the middle of each: `pre` sees every element of a piece, then `hook(end)`
// runs -- it may synchronise the block (every thread makes every call, the loop bounds are uniform) and returns true to end
// the scan --, then `test` sees the piece's elements again (they are still in registers).  A piece is a row of T elements
// over the first two batches (the bounds of a chain tighten fastest at its start) and a batch of AT_U rows from then on.
template <class Load, class Pre, class Hook, class Test>
__device__ __forceinline__ void asv_row_scan_pieces(Load load, int64_t jstart, int n, int crot, int last_block, int tid,
                                                    Pre pre, Hook hook, Test test) {
    const int64_t jt = jstart + tid;
    const int jlow = (int)(jt & 63), jb_t = (int)(jt >> 6);
    double pa[AT_U], wa[AT_U], pb[AT_U], wb[AT_U];
    auto fetch = [&](double (&p)[AT_U], double (&w)[AT_U], int base) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < AT_U; ++u) {
            int jb = jb_t + ((base + u * T) >> 6);
            jb = jb < last_block ? jb : last_block;
            const int64_t off = AsvTileLayout::at(crot, jb, jlow);
            load(off, p[u], w[u]);
        }
    };
    bool stop = false;
    auto consume = [&](const double (&p)[AT_U], const double (&w)[AT_U], int base) __attribute__((always_inline)) {
        if (base < 2 * AT_U * T) {
#pragma unroll
            for (int u = 0; u < AT_U; ++u) {
                if (stop) break;
                pre(p[u], w[u], base + u * T + tid);
                stop = hook(base + (u + 1) * T);
                if (!stop) test(p[u], w[u], base + u * T + tid);
            }
        } else {
#pragma unroll
            for (int u = 0; u < AT_U; ++u) pre(p[u], w[u], base + u * T + tid);
            stop = hook(base + AT_U * T);
            if (!stop) {
#pragma unroll
                for (int u = 0; u < AT_U; ++u) test(p[u], w[u], base + u * T + tid);
            }
        }
    };
    fetch(pa, wa, 0);
    for (int base = 0; base < n && !stop; base += 2 * AT_U * T) {
        fetch(pb, wb, base + AT_U * T);
        consume(pa, wa, base);
        fetch(pa, wa, base + 2 * AT_U * T);
        if (base + AT_U * T < n && !stop) consume(pb, wb, base + AT_U * T);
    }
}

// The streamed cells of one call, in stream order (the own batch's restricted cells, then the reference's), as ONE
// contiguous matrix with their squared norms and -- for the own batch -- their cell ids: the tile kernel then reads plain
// consecutive rows (coalesced, prefetchable any distance ahead) instead of chasing restrict[] -> row -> norm per step.
__global__ __launch_bounds__(256) void asv_gather_stream(const double* __restrict__ data1, const double* __restrict__ data2,
                                                         int g, int gs, const int32_t* __restrict__ r1, int nr1,
                                                         const int32_t* __restrict__ r2, int nr2, int64_t npad,
                                                         double* __restrict__ S, double* __restrict__ snrm,
                                                         int32_t* __restrict__ sid) {
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (j >= npad) return;
    const bool live = j < (int64_t)nr1 + nr2, own = j < nr2;
    const int rid = !live ? -1 : (own ? r2[j] : r1[j - nr2]);
    const double* src = live ? (own ? data2 : data1) + (int64_t)rid * g : nullptr;
    double sq = 0.0;
    const bool aug = gs >= g + 2;  // (the register-streamed form: column g holds 1, column g + 1 the squared norm)
    for (int k = lane; k < gs; k += 64) {  // (rows of gs >= g values and npad >= nr1 + nr2 rows: zeros beyond the data)
        const double v = live && k < g ? src[k] : 0.0;
        if (!(aug && k == g + 1)) S[j * gs + k] = (aug && k == g && live) ? 1.0 : v;
        sq += v * v;
    }
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
    if (lane == 0) {
        snrm[j] = sq;
        sid[j] = own ? rid : -1;
        if (aug) S[j * gs + g + 1] = live ? sq : 0.0;
    }
}

// snrm[n] = max of snrm[0, n): non-negative doubles order like their bit patterns (one workgroup's maximum per atomic)
__global__ __launch_bounds__(256) void asv_max_norm(double* __restrict__ snrm, int64_t n, unsigned int* __restrict__ gbar,
                                                    unsigned int* __restrict__ tile_ctr) {
    __shared__ double sm[ASV_T];
    if (gbar && blockIdx.x == 0 && threadIdx.x == 0) *gbar = 0u;  // (the tile kernel's round barrier starts from zero)
    if (tile_ctr && blockIdx.x == 0 && threadIdx.x == 0) *tile_ctr = 0u;  // (... and so does its tile counter)
    double m = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) m = fmax(m, snrm[i]);
    m = block_max(m, sm);
    if (threadIdx.x == 0) atomicMax(reinterpret_cast<unsigned long long*>(snrm + n), (unsigned long long)__double_as_longlong(m));
}

#ifdef BMX_ASV_AB_NOLIT
constexpr bool ASV_LIT_ON = false;
#else
constexpr bool ASV_LIT_ON = true;
#endif
#ifdef BMX_ASV_AB_NOSO  // timing build: the literal re-run without the own batch's packed pairs (its results are then wrong)
constexpr bool ASV_SO_ON = false;
#else
constexpr bool ASV_SO_ON = true;
#endif

// ---------------------------------------------------------------------------------------------------
// asv_tile_kernel is its prologue, the tile loop and the phases below, in this order.  Two structs carry what the phases
// share: the LDS pointers of the prologue and the constants of the call and of the tile.  Every phase is inlined: the
// kernel's code is what it was when the phases were the body of one loop.
// ---------------------------------------------------------------------------------------------------
struct TileLds {
    double *cx, *cg;  // [16][GP] the tile's cells, their unit gradients (both live through the per-cell phase: the literal re-run reads them)
    // one region, three lives: the A operands in lane order during the stream (cxp / cgp, NB8 > 8), the collected bin of the
    // histogram walk (lp / lw_), the sort buffer of the literal re-run (2 lcap doubles)
    double* ub;
    double* rs;  // [64][KC + 2] a step of streamed cells (staged form only)
    double *sc_proj, *sc_n, *sc_l2, *sc_mx1, *sc_mx2, *sc_lo, *sc_hi, *sc_tmp;  // per cell: own projection, |x|^2, |vect|, maxima, projection range
    double* etab;  // [32] 2^(j / 32) for asv_exp_neg
    double* sm;    // [AT_SM] block reductions
    unsigned long long *hist, *binmax;  // [NB] each; binmax per projection bin: the largest log-weight (bit pattern), then the bin's threshold
    int *sh_cnt, *sh_bin;
    unsigned long long* sh_before;
    int* sh_sel;            // [4] literal re-run: kept addends (own batch, reference in restrict order, in projection order), abort flag
    int (*sh_K)[3];         // per cell of the tile: the lengths of its three lists (-1: the cell went the histogram way)
    double (*sh_chain)[3];  // per cell: totalprob2, prob2, totalprob1 as the chains leave them
};
struct TileCtx {
    int g, GP, nr1, nr2, n2, lcap;
    double sigma2;
    bool lit_on;            // the literal re-run of flagged cells is on (lcap > 0)
    int64_t N, Npad, Nown;  // streamed cells (own batch first, then the reference); padded; the own batch's part, padded
    const double *data2, *vect, *S, *snrm;
    const int32_t* sid;
    double* out;
    AsvTileLayout L;
    double *wg, *SP, *SW;  // the workgroup's scratch; its projections and log-weights
    // the own batch's pairs, for the literal re-run only (it picks the kept addends of a flagged cell's own-batch chains from
    // them): ONE float per pair, the log-weight with its two lowest mantissa bits replaced by a code -- 0: above the cell's
    // projection (not counted in prob2, :90-92), 1: within rounding of it, 2: at or below it, 3: the cell itself
    float* SO;
    int rot0, last_block;  // the workgroup's slot rotation; the last 64-cell block of a scratch row
    int c0;                // the tile's first cell
};
// one cell's walk: the largest reference log-weight, the projections still in play, the first histogram's scale
struct CellWalk {
    double mx, blo, bhi, scale0;
};
// a lane's running values of the stream, for its four cells (lane >> 4) + 4 i
struct StreamAcc {
    double om[4], oa[4], ob[4];  // own batch, online: running maximum, sum of all, sum of those at or below the projection
    double mx1[4], lo[4], hi[4];  // reference batch: largest log-weight, projection range
    double cp[4], cn[4];          // the cells' own projections and squared norms
};

// ---- 1. the tile's cells: coordinates, unit gradient (:57-70), own projection, squared norm; the table of asv_exp_neg
__device__ __forceinline__ void tile_load_cells(const TileLds& lds, const TileCtx& tc) {
    const int tid = threadIdx.x;
    const int g = tc.g;
    const int GP = tc.GP;
    const int n2 = tc.n2;
    const int c0 = tc.c0;
    const double* const data2 = tc.data2;
    const double* const vect = tc.vect;
    double* const cx = lds.cx;
    double* const cg = lds.cg;
    double* const sc_proj = lds.sc_proj;
    double* const sc_n = lds.sc_n;
    double* const sc_l2 = lds.sc_l2;
    double* const etab = lds.etab;
    for (int e = tid; e < AT_C * GP; e += T) {
        const int c = e / GP, x = e - c * GP;
        const bool in = c0 + c < n2 && x < g;
        cx[e] = in ? data2[(int64_t)(c0 + c) * g + x] : 0.0;
        cg[e] = in ? vect[(int64_t)(c0 + c) * g + x] : 0.0;
    }
    __syncthreads();
    if (tid < AT_C) {
        double l2 = 0.0, nn = 0.0;
        for (int x = 0; x < g; ++x) l2 += cg[tid * GP + x] * cg[tid * GP + x];
        l2 = sqrt(l2);
        if (l2 != 0.0)
            for (int x = 0; x < g; ++x) cg[tid * GP + x] /= l2;
        double p = 0.0;
        for (int x = 0; x < g; ++x) {
            p += cg[tid * GP + x] * cx[tid * GP + x];
            nn += cx[tid * GP + x] * cx[tid * GP + x];
        }
        sc_l2[tid] = l2;
        sc_proj[tid] = p;
        sc_n[tid] = nn;
    }
    __syncthreads();
    if (tid < 32) etab[tid] = exp2((double)tid * 0.03125);  // (for asv_exp_neg)
    __syncthreads();
}

// ---- 2. testing hook "asv_sync" (OFF by default): the workgroups start the stream of their round's tiles TOGETHER and
// run in convoy, the first to ask for a row of S brings it into its XCD's L2 for the other 31.  That halves the kernel's
// HBM reads (PMC: 3.36 -> 1.56 TB on a mid-size call) and leaves its time where it was -- the stream's loads are
// prefetched a block ahead and hidden either way -- while the spread of the per-cell phases becomes idle time every
// round (config 5: 9.94 -> 10.78 s per step; rounds 4 and 6, EXPERIMENTS.md).  One arrival per TILE on a device word
// zeroed before the launch; the tiles of round r go on when all tiles of rounds <= r have arrived (or 50 ms have gone
// by).  gbar is null unless the hook is on and the launch is no wider than the device.
__device__ __forceinline__ void tile_round_barrier(unsigned int* gbar, int tile, int ntiles) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        const unsigned int round = (unsigned int)((tile - (int)blockIdx.x) / (int)gridDim.x);
        const unsigned long long want_ = (unsigned long long)(round + 1u) * gridDim.x;
        const unsigned int want = want_ < (unsigned long long)ntiles ? (unsigned int)want_ : (unsigned int)ntiles;
        __hip_atomic_fetch_add(gbar, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        // (the barrier is a matter of speed, never of correctness: a workgroup that has waited 50 ms -- another
        // process's kernel holds CUs this launch counted on -- goes on by itself)
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        while (__hip_atomic_load(gbar, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < want &&
               __builtin_amdgcn_s_memrealtime() - t0 < 5000000ull)
            __builtin_amdgcn_s_sleep(16);
    }
    __syncthreads();
}

// the partial log-sum-exps of the 16 lanes that share a cell: to their common maximum, then added; parked per (wave,
// cell) in the block-reduction area (nobody else uses it during the stream) -- see the reduction behind the stream
__device__ __forceinline__ void stream_own_done(StreamAcc& acc, const TileLds& lds) {
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    double* const sm = lds.sm;
    double (&om)[4] = acc.om;
    double (&oa)[4] = acc.oa;
    double (&ob)[4] = acc.ob;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        for (int o = 1; o < 16; o <<= 1) {
            const double pm = __shfl_xor(om[i], o), pa = __shfl_xor(oa[i], o), pb = __shfl_xor(ob[i], o);
            const double mm = fmax(om[i], pm);
            const double f0 = om[i] == mm ? 1.0 : exp(om[i] - mm), f1 = pm == mm ? 1.0 : exp(pm - mm);
            oa[i] = oa[i] * f0 + pa * f1;
            ob[i] = ob[i] * f0 + pb * f1;
            om[i] = mm;
        }
        if ((lane & 15) == 0) {
            const int c = (lane >> 4) + 4 * i;
            sm[(w * AT_C + c) * 6 + 3] = om[i];
            sm[(w * AT_C + c) * 6 + 4] = oa[i];
            sm[(w * AT_C + c) * 6 + 5] = ob[i];
        }
    }
}

// NB8 > 0 (= ceil(g / 8), g <= 128): the streamed cells go from global memory straight into the B-operand registers.  A row
// is taken in blocks of 8 dimensions, each two MFMA steps: step (q, t) multiplies dimensions 8 q + 2 (lane >> 4) + t, so the
// two values a lane needs of a block are 16 contiguous bytes of its row and a row costs ceil(g / 8) * 8 dimensions of
// matrix work (104 at 100 PCs; blocks of 32 dimensions, the first form, paid for 128).  Every wave runs its 16 streamed
// cells on its own -- no staging through the LDS, no barrier in the stream, the next step's rows in flight while the
// current ones multiply.  NB8 = 0: the staged form (any g <= 256).
template <int NB8>
__device__ __forceinline__ void tile_stream_registers(const TileLds& lds, const TileCtx& tc, StreamAcc& acc, double tol_tile) {
    const int tid = threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    const double NEG = -__builtin_inf();
    const double POS = __builtin_inf();
    constexpr bool so_on = ASV_SO_ON;
    const int g = tc.g;
    const int GP = tc.GP;
    const int nr2 = tc.nr2;
    const int c0 = tc.c0;
    const int rot0 = tc.rot0;
    const double sigma2 = tc.sigma2;
    const bool lit_on = tc.lit_on;
    const int64_t N = tc.N;
    const int64_t Npad = tc.Npad;
    const double* const S = tc.S;
    const int32_t* const sid = tc.sid;
    double* const SP = tc.SP;
    double* const SW = tc.SW;
    float* const SO = tc.SO;
    double* const cx = lds.cx;
    double* const cg = lds.cg;
    double* const cxp = lds.ub;                                 // [2 NB8][64] the cells' coordinates as the lanes read them
    double* const cgp = cxp + (NB8 > 8 ? NB8 * 2 * 64 : 0);  // [2 NB8][64] the unit gradients likewise (NB8 > 8)
    double* const sc_n = lds.sc_n;
    double* const etab = lds.etab;
    double (&om)[4] = acc.om;
    double (&oa)[4] = acc.oa;
    double (&ob)[4] = acc.ob;
    double (&mx1)[4] = acc.mx1;
    double (&lo)[4] = acc.lo;
    double (&hi)[4] = acc.hi;
    double (&cp)[4] = acc.cp;
    typedef double d2a __attribute__((ext_vector_type(2)));
    constexpr int GS = NB8 * 8;  // row stride of the stream (zero filled beyond g)
    constexpr int NST = 2 * NB8;  // MFMA steps per product
    const int kq = lane >> 4;
    // the A operands of MFMA step st = 2 q + t: lane l holds cell l & 15, dimension 8 q + 2 (l >> 4) + t.  Up to 64
    // dimensions they live in registers for the whole stream, beyond that in the LDS in lane order.
    // Round 6: the distance chain's A operand is the cell SCALED and AUGMENTED -- (2 / sigma) x_c, then -|x_c|^2 / sigma
    // against the row's column of ones and -1 / sigma against its squared norm -- so that the chain delivers
    // -|x_c - x_o|^2 / sigma and the epilogue is left with one multiply, one fused multiply-add and a clamp per pair
    // where it had an add, a multiply, two subtractions, a clamp and a division (FP64 vector work does not run under
    // FP64 MFMAs on this part: EXPERIMENTS.md round 6).  The values differ from the division's by rounding of the order
    // of 1e-14 (|x_c|^2 + |x_o|^2) / sigma, inside the margin `mb` every use of them carries.
    const double isig = 1.0 / sigma2;
    auto a_dist = [&](int cell, int k) -> double {
        return k < g ? cx[cell * GP + k] * (2.0 * isig) : (k == g ? -sc_n[cell] * isig : (k == g + 1 ? -isig : 0.0));
    };
    double axr[NB8 <= 8 ? NST : 1], agr[NB8 <= 8 ? NST : 1];
    if constexpr (NB8 <= 8) {
#pragma unroll
        for (int st = 0; st < NST; ++st) {
            const int k = 8 * (st >> 1) + 2 * kq + (st & 1);
            axr[st] = a_dist(lane & 15, k);
            agr[st] = cg[(lane & 15) * GP + k];
        }
    } else {
        for (int e = tid; e < NST * 64; e += T) {
            const int st = e >> 6, ln = e & 63;
            const int k = 8 * (st >> 1) + 2 * (ln >> 4) + (st & 1);
            cxp[e] = a_dist(ln & 15, k);
            cgp[e] = cg[(ln & 15) * GP + k];
        }
        __syncthreads();
    }
    // this lane's streamed cell of step j0 is j0 + jl; rows, norms, ids and scratch are padded to whole pairs of
    // steps: no bounds checks (and no divergent branches) in the stream
    const int jl = 16 * w + (lane & 15);
    const double* srow = S + (int64_t)jl * GS + 2 * kq;
    double* spo = SP + jl;
    double* swo = SW + jl;
    // own-batch codes: [block of 64 streamed cells][kq][64][4 cells kq + 4 i] floats
    f4* so_ = reinterpret_cast<f4*>(SO) + kq * 64 + jl;
    auto load_rows = [&](double (&b)[NST], const double* src) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < NB8; ++q) {
            const d2a v = *reinterpret_cast<const d2a*>(src + 8 * q);
            b[2 * q] = v[0];
            b[2 * q + 1] = v[1];
        }
    };
    // One 64-row block of the stream for this wave's 16 rows of it.  Round 6: on this part NOTHING runs under an FP64 MFMA
    // -- every vector instruction of a SIMD, whichever wave it comes from, adds its ~4 cycles to the 64 of each MFMA
    // (scripts/microbench/mfma_f64_valu.hip) -- so what a block costs is its 52 MFMAs plus the COUNT of everything else,
    // and rounds 3-5's single loop carried ~450 vector instructions a block (per-element selects between the two kinds
    // of rows, SGPR spills, accumulator moves).  Hence one loop per KIND of block (MODE), each with only its own running
    // state and its own half of the epilogue, and ONE row set per wave, each piece re-loaded right behind the two MFMAs
    // that consumed it (the same prefetch distance as a second buffer, 52 registers less):
    //   0 every row of the block belongs to the OWN batch: the online log-sum-exps (and the float codes of the re-run);
    //   1 a block that holds the end of the own batch (or rows of both kinds, or padding): everything, by selects;
    //   2 every row belongs to the REFERENCE batch: maxima, projection range, the scratch stores;
    //   3 reference rows and the stream's zero padding behind them.
    auto step = [&](auto mode_tag, double (&b)[NST], int64_t j0) __attribute__((always_inline)) {
        constexpr int MODE = decltype(mode_tag)::value;
        const int64_t jo = j0 + jl;
        const double* nsrc = srow + (j0 + AT_R < Npad ? (j0 + AT_R) : j0) * GS;  // (the last block asks for its own again)
        int rid = -1;
        if constexpr (MODE <= 1) rid = sid[jo];
        // two accumulator pairs (k-steps alternate): D and P chains are independent of each other as well
        d4 Dq[2], Pq[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) Dq[a] = Pq[a] = d4{0.0, 0.0, 0.0, 0.0};
        // (NB8 > 8: the A operands come from the LDS, asked for AHEAD k-steps before the MFMAs that take them -- read
        // right in front of its MFMAs, as the compiler places them, every pair of k-steps waits out the LDS's latency:
        // the bare chains ran at 0.79 of the matrix pipe's rate)
        constexpr int AHEAD = 4;
        double axq[NB8 > 8 ? AHEAD : 1], agq[NB8 > 8 ? AHEAD : 1];
        if constexpr (NB8 > 8) {
#pragma unroll
            for (int t = 0; t < AHEAD; ++t) {
                axq[t] = cxp[t * 64 + lane];
                agq[t] = cgp[t * 64 + lane];
            }
        }
#pragma unroll
        for (int st = 0; st < NST; ++st) {
            double ax, ag;
            if constexpr (NB8 <= 8) {
                ax = axr[st];
                ag = agr[st];
            } else {
                ax = axq[st % AHEAD];
                ag = agq[st % AHEAD];
                if (st + AHEAD < NST) {
                    axq[st % AHEAD] = cxp[(st + AHEAD) * 64 + lane];
                    agq[st % AHEAD] = cgp[(st + AHEAD) * 64 + lane];
                }
            }
            Dq[st & 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, b[st], Dq[st & 1], 0, 0, 0);
            Pq[st & 1] = __builtin_amdgcn_mfma_f64_16x16x4f64(ag, b[st], Pq[st & 1], 0, 0, 0);
            if (st & 1) {  // both values of this 8-dimension block are consumed: the next block's piece takes their place
                const d2a v = *reinterpret_cast<const d2a*>(nsrc + 8 * (st >> 1));
                b[st - 1] = v[0];
                b[st] = v[1];
            }
            if constexpr (NB8 > 8) __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);  // (two MFMAs, then what belongs behind them)
        }
        const bool own = MODE == 0 ? true : (MODE >= 2 ? false : jo < nr2);
        const bool ref = MODE == 0 ? false : (MODE == 2 ? true : (!own && jo < N));
        const int blk = (int)(j0 >> 6);
        f4 oc = f4{0.f, 0.f, 0.f, 0.f};
        (void)tol_tile;
        double* sp_ = spo + (int64_t)blk * (AT_C * 64);
        double* sw_ = swo + (int64_t)blk * (AT_C * 64);
#pragma unroll
        for (int i = 0; i < 4; ++i) {  // this lane: streamed cell jo, tile cells (lane >> 4) + 4 i
            double pr = Pq[0][i] + Pq[1][i];
            const double s_ = cp[i] - pr;
            // -(|x_c - x_o|^2 - s^2) / sigma: the chain's value plus s^2 / sigma, never above zero
            double lw = __builtin_fma(s_, s_ * isig, Dq[0][i] + Dq[1][i]);
            lw = lw < 0.0 ? lw : -0.0;  // (log-weights are <= -0, as -d2 / sigma was: the per-bin maxima order them by bit pattern)
            bool self = false;
            if constexpr (MODE <= 1) {
                self = rid == c0 + kq + 4 * i;  // the cell itself: log-weight 0, always counted (:80-84)
                lw = self ? 0.0 : lw;
                pr = self ? NEG : pr;
            }
            if constexpr (MODE >= 1) {
                // (selects, not branches: the padding rows of the stream belong to neither batch)
                mx1[i] = fmax(mx1[i], ref ? lw : NEG);
                lo[i] = fmin(lo[i], ref ? pr : POS);
                hi[i] = fmax(hi[i], ref ? pr : NEG);
            }
            if constexpr (MODE <= 1) {
                if (own) {  // (whole waves but for the one block where the own batch ends)
                    if (lw > om[i]) {  // a new maximum: rare once the cell itself (log-weight 0) has gone by
                        const double f = asv_exp_neg(om[i] - lw, etab);  // exp(-inf) = 0 the first time
                        oa[i] *= f;
                        ob[i] *= f;
                        om[i] = lw;
                    }
                    const double e = asv_exp_neg(lw - om[i], etab);
                    oa[i] += e;
                    ob[i] += !(pr > cp[i]) ? e : 0.0;
                }
            }
            if (!own) {
                const int slot = (kq + 4 * i + blk + rot0) & (AT_C - 1);  // == at(kq + 4 i, jo)
                sp_[slot * 64] = pr;
                sw_[slot * 64] = lw;
            } else if (lit_on && so_on) {
                // (s_ = the cell's projection minus this one's; tol_tile >= the rounding of the two, for every cell of the tile)
                const unsigned code = self ? 3u : (s_ >= tol_tile ? 2u : (s_ >= -tol_tile ? 1u : 0u));
                oc[i] = __uint_as_float((__float_as_uint((float)fmax(lw, -3.0e38)) & ~3u) | code);
            }
        }
        // (this lane's four cells kq, kq + 4, kq + 8, kq + 12 of one streamed cell: one 16-byte store, 16 lanes a 256-byte run)
        if (own && lit_on && so_on) so_[(int64_t)blk * (AT_C * 16)] = oc;
    };
    double ba[NST];
    int64_t j0 = 0;
    load_rows(ba, srow);
    for (; j0 + AT_R <= nr2; j0 += AT_R) step(std::integral_constant<int, 0>{}, ba, j0);
    if (j0 < nr2) {
        step(std::integral_constant<int, 1>{}, ba, j0);
        j0 += AT_R;
    }
    stream_own_done(acc, lds);  // (the own batch's sums leave the registers: the reference loop runs without them; see below)
    for (; j0 + AT_R <= N; j0 += AT_R) step(std::integral_constant<int, 2>{}, ba, j0);
    for (; j0 < Npad; j0 += AT_R) step(std::integral_constant<int, 3>{}, ba, j0);
}

// The staged form of the stream (NB8 = 0: 126 < g <= 256): 64 streamed rows go through the LDS in steps of 32 dimensions.
__device__ __forceinline__ void tile_stream_staged(const TileLds& lds, const TileCtx& tc, StreamAcc& acc, double tol_tile) {
    const int tid = threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    const double NEG = -__builtin_inf();
    const double POS = __builtin_inf();
    const int g = tc.g;
    const int GP = tc.GP;
    const int nr2 = tc.nr2;
    const int c0 = tc.c0;
    const int rot0 = tc.rot0;
    const double sigma2 = tc.sigma2;
    const bool lit_on = tc.lit_on;
    const int64_t N = tc.N;
    const double* const S = tc.S;
    const double* const snrm = tc.snrm;
    const int32_t* const sid = tc.sid;
    double* const SP = tc.SP;
    double* const SW = tc.SW;
    float* const SO = tc.SO;
    auto at = [rot0](int c, int64_t j) { return AsvTileLayout::at(c + rot0, (int)(j >> 6), (int)(j & 63)); };
    double* const cx = lds.cx;
    double* const cg = lds.cg;
    double* const rs = lds.rs;
    double (&om)[4] = acc.om;
    double (&oa)[4] = acc.oa;
    double (&ob)[4] = acc.ob;
    double (&mx1)[4] = acc.mx1;
    double (&lo)[4] = acc.lo;
    double (&hi)[4] = acc.hi;
    double (&cp)[4] = acc.cp;
    double (&cn)[4] = acc.cn;
    // staging: 64 rows x 4 segments of 8 doubles per step of 32 dimensions; the step after the one being multiplied is
    // already on its way into registers (16-byte loads where the rows allow), the row pointers one streamed block ahead
    typedef double d2a __attribute__((ext_vector_type(2)));
    const int lr = tid >> 2, seg = (tid & 3) * 8;
    const bool vec = (g & 1) == 0;
    const int nkc = (g + AT_KC - 1) / AT_KC;
    auto row_ptr = [&](int64_t jr) -> const double* { return jr < N ? S + jr * g : nullptr; };
    double pf[8];
    auto fetch = [&](const double* src, int k0) __attribute__((always_inline)) {
        if (src && vec && k0 + seg + 8 <= g) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const d2a v = *reinterpret_cast<const d2a*>(src + k0 + seg + 2 * e);
                pf[2 * e] = v[0];
                pf[2 * e + 1] = v[1];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = k0 + seg + e;
                pf[e] = (src && k < g) ? src[k] : 0.0;
            }
        }
    };
    const double* src = row_ptr(lr);
    const double* src_next = row_ptr((int64_t)AT_R + lr);
    fetch(src, 0);
    for (int64_t j0 = 0; j0 < N; j0 += AT_R) {
        d4 D = d4{0.0, 0.0, 0.0, 0.0}, P = d4{0.0, 0.0, 0.0, 0.0};
        // this lane's streamed cell of the step: its norm and id are asked for now and used after the products
        const int64_t jo = j0 + 16 * w + (lane & 15);
        const double no = jo < N ? snrm[jo] : 0.0;
        const int rid = jo < N ? sid[jo] : -1;
        for (int kc = 0; kc < nkc; ++kc) {
            const int k0 = kc * AT_KC;
#pragma unroll
            for (int e = 0; e < 8; ++e) rs[lr * (AT_KC + 2) + seg + e] = pf[e];
            __syncthreads();
            if (kc + 1 < nkc) {
                fetch(src, k0 + AT_KC);
            } else {  // the next streamed block's first step; its successor's row pointer starts its own round trip
                src = src_next;
                fetch(src, 0);
                src_next = row_ptr(j0 + 2 * AT_R + lr);
                (void)src_next;
            }
#pragma unroll
            for (int kk = 0; kk < AT_KC / 4; ++kk) {
                const double b = rs[(16 * w + (lane & 15)) * (AT_KC + 2) + 4 * kk + (lane >> 4)];
                const double ax = cx[(lane & 15) * GP + k0 + 4 * kk + (lane >> 4)];
                const double ag = cg[(lane & 15) * GP + k0 + 4 * kk + (lane >> 4)];
                D = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, b, D, 0, 0, 0);
                P = __builtin_amdgcn_mfma_f64_16x16x4f64(ag, b, P, 0, 0, 0);
            }
            __syncthreads();
        }
        // this lane: streamed cell jo, tile cells (lane >> 4) + 4 i
        if (jo < N) {
            const bool own = jo < nr2;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = (lane >> 4) + 4 * i;
                double pr = P[i];
                const double s_ = cp[i] - pr;
                double d2 = (cn[i] + no) - 2.0 * D[i] - s_ * s_;
                d2 = d2 > 0.0 ? d2 : 0.0;
                double lw = -d2 / sigma2;
                if (own && rid == c0 + c) {  // the cell itself: log-weight 0, always counted (:80-84)
                    lw = 0.0;
                    pr = NEG;
                }
                mx1[i] = fmax(mx1[i], own ? NEG : lw);
                lo[i] = fmin(lo[i], own ? POS : pr);
                hi[i] = fmax(hi[i], own ? NEG : pr);
                if (own) {
                    if (lw > om[i]) {
                        const double f = exp(om[i] - lw);
                        oa[i] *= f;
                        ob[i] *= f;
                        om[i] = lw;
                    }
                    const double e = exp(lw - om[i]);
                    oa[i] += e;
                    ob[i] += !(pr > cp[i]) ? e : 0.0;
                }
                if (!own) {
                    SP[at(c, jo)] = pr;
                    SW[at(c, jo)] = lw;
                } else if (lit_on) {
                    const unsigned code = rid == c0 + c ? 3u : (s_ >= tol_tile ? 2u : (s_ >= -tol_tile ? 1u : 0u));
                    SO[AsvTileLayout::so_at(jo >> 6, (int)(jo & 63), c)] =
                        __uint_as_float((__float_as_uint((float)fmax(lw, -3.0e38)) & ~3u) | code);
                }
            }
        }
    }
}

// The reduction behind the stream: per-cell maxima and projection range over the 16 lanes of a row group, then over the
// waves, into sc_mx1 / sc_lo / sc_hi; the own batch's parked partial sums into prob2 (sc_mx2).
__device__ __forceinline__ void tile_stream_reduce(const TileLds& lds, const TileCtx& tc, StreamAcc& acc) {
    const int tid = threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    const double NEG = -__builtin_inf();
    const double POS = __builtin_inf();
    const int nr2 = tc.nr2;
    double* const sc_mx1 = lds.sc_mx1;
    double* const sc_mx2 = lds.sc_mx2;
    double* const sc_lo = lds.sc_lo;
    double* const sc_hi = lds.sc_hi;
    double* const sm = lds.sm;
    double (&mx1)[4] = acc.mx1;
    double (&lo)[4] = acc.lo;
    double (&hi)[4] = acc.hi;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        for (int o = 1; o < 16; o <<= 1) {
            mx1[i] = fmax(mx1[i], __shfl_xor(mx1[i], o));
            lo[i] = fmin(lo[i], __shfl_xor(lo[i], o));
            hi[i] = fmax(hi[i], __shfl_xor(hi[i], o));
        }
    }
    if ((lane & 15) == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = (lane >> 4) + 4 * i;
            sm[(w * AT_C + c) * 6 + 0] = mx1[i];
            sm[(w * AT_C + c) * 6 + 1] = lo[i];
            sm[(w * AT_C + c) * 6 + 2] = hi[i];
        }
    }
    __syncthreads();
    if (tid < AT_C) {
        double a = NEG, l = POS, h = NEG, m2 = NEG;
        for (int ww = 0; ww < 4; ++ww) {
            a = fmax(a, sm[(ww * AT_C + tid) * 6 + 0]);
            l = fmin(l, sm[(ww * AT_C + tid) * 6 + 1]);
            h = fmax(h, sm[(ww * AT_C + tid) * 6 + 2]);
            m2 = fmax(m2, sm[(ww * AT_C + tid) * 6 + 3]);
        }
        double all = 0.0, below = 0.0;  // the four waves' partial sums to the common maximum, in wave order
        for (int ww = 0; ww < 4; ++ww) {
            const double pm = sm[(ww * AT_C + tid) * 6 + 3];
            const double f = pm == m2 ? 1.0 : exp(pm - m2);
            all += sm[(ww * AT_C + tid) * 6 + 4] * f;
            below += sm[(ww * AT_C + tid) * 6 + 5] * f;
        }
        sc_mx1[tid] = a;
        // prob2 (:74-112): log-sum of the cells at or below the projection minus the log-sum of all of them; 0 - the
        // latter when none is at or below (:76: prob2 then keeps its starting value)
        sc_mx2[tid] = nr2 > 0 ? (below > 0.0 ? m2 + log(below) : 0.0) - (m2 + log(all)) : 0.0;
        sc_lo[tid] = l;
        sc_hi[tid] = h;
    }
    __threadfence_block();
    __syncthreads();
    // (the scratch rows were written by this block and are read by it: same CU, through the L2)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");
}

// ---- 3. pass over the streamed cells: projections and log-weights of every (cell, streamed cell) pair
// own batch: log-sum-exp of every cell's weights, all of them and those at or below its projection (:74-112), taken
// ONLINE in the stream's epilogue -- running maximum om, sums relative to it -- so that the own batch's 40 % of the
// (cell, streamed cell) pairs are not read back (round 3: 16 + 16 bytes per pair); they are written all the same when
// the literal re-run is on (lit_on): a flagged cell picks the kept addends of its own-batch chains from them
template <int NB8>
__device__ __forceinline__ void tile_stream(const TileLds& lds, const TileCtx& tc) {
    const int lane = threadIdx.x & 63;
    const double NEG = -__builtin_inf();
    const double POS = __builtin_inf();
    const bool lit_on = tc.lit_on;
    const int64_t Npad = tc.Npad;
    const double* const snrm = tc.snrm;
    double* const sc_proj = lds.sc_proj;
    double* const sc_n = lds.sc_n;
    StreamAcc acc;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        acc.om[i] = NEG;
        acc.oa[i] = acc.ob[i] = 0.0;
        acc.mx1[i] = NEG;
        acc.lo[i] = POS;
        acc.hi[i] = NEG;
        acc.cp[i] = sc_proj[(lane >> 4) + 4 * i];
        acc.cn[i] = sc_n[(lane >> 4) + 4 * i];
    }
    double tol_tile = 0.0;  // >= the rounding of g . x for any cell of the tile and any streamed cell (|g| = 1)
    if (lit_on) {
        double cmx = 0.0;
        for (int c = 0; c < AT_C; ++c) cmx = fmax(cmx, sc_n[c]);
        tol_tile = 1e-13 * (1.0 + cmx + snrm[Npad]);
    }
    if constexpr (NB8 > 0) {
        tile_stream_registers<NB8>(lds, tc, acc, tol_tile);
    } else {
        tile_stream_staged(lds, tc, acc, tol_tile);
        stream_own_done(acc, lds);  // (the register-streamed form parked the own batch's sums when its last own block was through)
    }
    tile_stream_reduce(lds, tc, acc);
}

// ---- 4. per cell: the first histogram of the walk; for a flagged cell also every bin's largest log-weight and the number
// of reference cells within 38.5 of the largest one (all of those are kept addends), which it returns (0: not flagged)
__device__ __forceinline__ int cell_first_histogram(const TileLds& lds, const TileCtx& tc, int c, bool flagged, CellWalk& cw) {
    const int tid = threadIdx.x;
    const double FIX = 1099511627776.0;  // 2^40: the histogram's fixed-point unit
    const int nr1 = tc.nr1;
    const int nr2 = tc.nr2;
    const int rot0 = tc.rot0;
    const int last_block = tc.last_block;
    double* const SP = tc.SP;
    double* const SW = tc.SW;
    double* const sm = lds.sm;
    unsigned long long* const hist = lds.hist;
    unsigned long long* const binmax = lds.binmax;
    int& sh_cnt = *lds.sh_cnt;
    const double blo = cw.blo;
    const double bhi = cw.bhi;
    const double mx = cw.mx;
    const unsigned long long NEGBITS = 0xFFF0000000000000ull;  // -inf
    for (int b = tid; b < AT_NB; b += T) {
        hist[b] = 0ull;
        binmax[b] = NEGBITS;
    }
    if (tid == 0) sh_cnt = 0;
    __syncthreads();
    const double scale0 = bhi > blo ? (double)AT_NB / (bhi - blo) : 0.0;
    int cG = 0;
    if (flagged) {
        asv_row_scan<true>(SP, SW, nr2, nr1, c + rot0, last_block, tid, [&](double pr, double lw, int o) {
            const bool in = o < nr1 && pr >= blo && pr <= bhi;
            int b = (int)((pr - blo) * scale0);
            b = b < 0 ? 0 : (b > AT_NB - 1 ? AT_NB - 1 : b);
            const double wv = exp(lw - mx) * FIX;
            atomicAdd(&hist[in ? b : (tid & (AT_NB - 1))], in ? (unsigned long long)wv : 0ull);
            // (log-weights are <= -0: as bit patterns the largest value is the smallest pattern)
            atomicMin(&binmax[in ? b : (tid & (AT_NB - 1))], in ? (unsigned long long)__double_as_longlong(lw) : NEGBITS);
            cG += in && lw >= mx - 38.5 ? 1 : 0;
        });
    } else {
        asv_row_scan<true>(SP, SW, nr2, nr1, c + rot0, last_block, tid, [&](double pr, double lw, int o) {
            const bool in = o < nr1 && pr >= blo && pr <= bhi;
            int b = (int)((pr - blo) * scale0);
            b = b < 0 ? 0 : (b > AT_NB - 1 ? AT_NB - 1 : b);
            const double wv = exp(lw - mx) * FIX;
            // (an element out of play adds nothing to a bin of the thread's own: no branch, no pile-up on one bin)
            atomicAdd(&hist[in ? b : (tid & (AT_NB - 1))], in ? (unsigned long long)wv : 0ull);
        });
    }
    __syncthreads();
    cw.scale0 = scale0;
    return flagged ? block_sum(cG, reinterpret_cast<int*>(sm)) : 0;
}

// ---- 5. per flagged cell, the literal re-run (see the comment in front of asv_noop_below).  cell_literal_select: the bin
// thresholds and the kept addends of the three chains, as index lists in the workgroup's scratch and their lengths in
// sh_sel; false: a chain keeps more than lcap_c addends, the cell goes the histogram way.
__device__ __forceinline__ bool cell_literal_select(const TileLds& lds, const TileCtx& tc, int c, int lcap_c, const CellWalk& cw, double nmax_s) {
    const int tid = threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    const double NEG = -__builtin_inf();
    const int nr1 = tc.nr1;
    const int nr2 = tc.nr2;
    const int lcap = tc.lcap;
    const int rot0 = tc.rot0;
    const int last_block = tc.last_block;
    const double sigma2 = tc.sigma2;
    const int64_t Nown = tc.Nown;
    double* const SP = tc.SP;
    double* const SW = tc.SW;
    float* const SO = tc.SO;
    double* const sc_n = lds.sc_n;
    double* const sm = lds.sm;
    unsigned long long* const binmax = lds.binmax;
    int* const sh_sel = lds.sh_sel;
    const double blo = cw.blo;
    const double bhi = cw.bhi;
    const double mx = cw.mx;
    const double scale0 = cw.scale0;
    int32_t* const giO = reinterpret_cast<int32_t*>(tc.wg + tc.L.GI);  // [3][lcap]: the index lists, reused per cell
    int32_t* const giR = reinterpret_cast<int32_t*>(tc.wg + tc.L.GI) + lcap;
    int32_t* const giS = reinterpret_cast<int32_t*>(tc.wg + tc.L.GI) + 2 * lcap;
    const double cn_c = sc_n[c];
    const double mb = 1e-3 + 1e-13 * (cn_c + nmax_s) / sigma2;      // >= the rounding of a GEMM-form log-weight
    const double tolp = 1e-13 * (sqrt(cn_c) + sqrt(nmax_s)) + 1e-300;  // >= the rounding of a projection
    // (b) per bin: the threshold below which a reference cell cannot change the SORTED chain -- from the
    // largest log-weight of the bins at least two back (every cell of those sorts in front of every cell of
    // this bin whatever the rounding of the projections, as long as a bin is much wider than that rounding)
    double* binthr = reinterpret_cast<double*>(binmax);
    {
        const bool wide = (bhi - blo) > 16.0 * AT_NB * tolp;
        double v[8], m8 = NEG;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            v[k] = __longlong_as_double((long long)binmax[8 * tid + k]);
            m8 = fmax(m8, v[k]);
        }
        double inc = m8;
        for (int o2 = 1; o2 < 64; o2 <<= 1) {
            const double t2 = __shfl_up(inc, o2);
            if (lane >= o2) inc = fmax(inc, t2);
        }
        __syncthreads();
        if (lane == 63) sm[w] = inc;
        __syncthreads();
        double run = __shfl_up(inc, 1);
        if (lane == 0) run = NEG;
        for (int ww = 0; ww < w; ++ww) run = fmax(run, sm[ww]);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const double E = run;  // largest log-weight of the bins in front of bin 8 tid + k
            run = fmax(run, v[k]);
            if (8 * tid + k + 1 < AT_NB)
                binthr[8 * tid + k + 1] = wide ? asv_thr_neg(E, mx, (double)nr1, mb) : NEG;
        }
        if (tid == 0) {
            binthr[0] = NEG;
            sh_sel[0] = sh_sel[1] = sh_sel[2] = 0;
        }
        __syncthreads();
    }
    // (c) the reference batch: kept addends of totalprob1's chain (restrict order) and of the walk's.  A piece's
    // elements are held against the largest log-weight of the pieces in front of it; the chain never exceeds
    // mx + log(nr1), mx the largest log-weight of all (from the stream).
    {
        double Mr = NEG, thrR = NEG, mT = NEG;
        int par = 0;
        const double hi_keep = bhi - 2.0 * tolp;  // (the last projection of the sort is the walk's default, :141)
        asv_row_scan_pieces(
            [&](int64_t off, double& p_, double& w_) {
                p_ = SP[off];
                w_ = SW[off];
            },
            nr2, nr1, c + rot0, last_block, tid,
            [&](double, double lw, int o) { mT = fmax(mT, o < nr1 ? lw : NEG); },
            [&](int) -> bool {
                thrR = asv_thr_neg(Mr, mx, (double)nr1, mb);  // (from the pieces in front of this one)
                double r = mT;
                for (int o2 = 1; o2 < 64; o2 <<= 1) r = fmax(r, __shfl_xor(r, o2));
                double* smx = sm + par * 8;
                if (lane == 0) smx[w] = r;
                if (tid == 0) smx[4] = (sh_sel[1] > lcap_c || sh_sel[2] > lcap_c) ? 1.0 : 0.0;
                __syncthreads();
                Mr = fmax(Mr, fmax(fmax(smx[0], smx[1]), fmax(smx[2], smx[3])));
                mT = NEG;
                par ^= 1;
                return smx[4] != 0.0;
            },
            [&](double pr, double lw, int o) {
                const bool in = o < nr1;
                int b = (int)((pr - blo) * scale0);
                b = b < 0 ? 0 : (b > AT_NB - 1 ? AT_NB - 1 : b);
                if (in && lw >= thrR) {
                    const int pos = atomicAdd(&sh_sel[1], 1);
                    if (pos < lcap) giR[pos] = o;
                }
                if (in && (lw >= binthr[b] || pr >= hi_keep)) {
                    const int pos = atomicAdd(&sh_sel[2], 1);
                    if (pos < lcap) giS[pos] = o;
                }
            });
        __syncthreads();
    }
    bool ok = sh_sel[1] <= lcap_c && sh_sel[2] <= lcap_c;
    // (d) the own batch: kept addends of totalprob2's and prob2's chains (one list: an addend that is a
    // no-op for one of them is one in the re-run as well).  The cell's own first place in restrict2 (spos: the
    // first code-3 element, found by the scan as it goes) splits the chains into their two regimes: elements in
    // front of it are held against the largest log-weight of the pieces in front of theirs, the chain bounded with
    // their own piece's included; those behind it against the largest OTHER log-weight of the pieces in front (the
    // cell's later occurrences, log-weight 0, are left out of that bound: lower bounds may always leave out).  The
    // pairs come as float codes (see SO): log-weights to 1e-6 relative (they are <= 0: x (1 + 1e-6) bounds one
    // from below, x (1 - 1e-6) from above), the side of the cell's projection as decided by the stream.
    if (ok) {
        const double DN = 1.0 + 1e-6, UP = 1.0 - 1e-6;
        const int last_own = (int)(Nown >> 6) - 1;
        int spos = 0x7fffffff, mspos = 0x7fffffff;
        double Tx = NEG, Px = NEG;      // totalprob2 / prob2: the largest other log-weight of the pieces gone by
        double mTx = NEG, mPx = NEG;    // the same of the current piece
        double thrTb = NEG, thrPb = NEG, thrTa = NEG, thrPa = NEG;
        int par = 0;
        asv_row_scan_pieces(
            [&](int64_t off, double& p_, double& w_) {
                // (the scanner's offset is (block * 16 + slot) * 64 + j: the block and j are what is needed)
                const unsigned u = __float_as_uint(SO[AsvTileLayout::so_at(off >> 10, (int)(off & 63), c)]);
                p_ = (double)(u & 3u);
                w_ = (double)__uint_as_float(u & ~3u);
            },
            0, nr2, c + rot0, last_own, tid,
            [&](double code, double lw, int o) {
                const bool in = o < nr2;
                const bool other = in && code != 3.0;
                const bool sure = other && code >= 2.0;    // counted in prob2 whatever the rounding (:90-92)
                mTx = fmax(mTx, other ? lw : NEG);
                mPx = fmax(mPx, sure ? lw : NEG);
                mspos = in && code == 3.0 && o < mspos ? o : mspos;
            },
            [&](int end) -> bool {
                double r1 = mTx, r3 = mPx;
                int rs_ = mspos;
                for (int o2 = 1; o2 < 64; o2 <<= 1) {
                    r1 = fmax(r1, __shfl_xor(r1, o2));
                    r3 = fmax(r3, __shfl_xor(r3, o2));
                    const int t2 = __shfl_xor(rs_, o2);
                    rs_ = t2 < rs_ ? t2 : rs_;
                }
                double* smx = sm + par * 32;
                if (lane == 0) {
                    smx[w * 4 + 0] = r1;
                    smx[w * 4 + 1] = r3;
                    smx[w * 4 + 2] = (double)rs_;
                }
                if (tid == 0) smx[16] = sh_sel[0] > lcap_c ? 1.0 : 0.0;
                __syncthreads();
                double pTx = NEG, pPx = NEG, ps = 2147483647.0;
                for (int ww = 0; ww < 4; ++ww) {
                    pTx = fmax(pTx, smx[ww * 4 + 0]);
                    pPx = fmax(pPx, smx[ww * 4 + 1]);
                    ps = fmin(ps, smx[ww * 4 + 2]);
                }
                if (spos == 0x7fffffff) spos = (int)ps;
                const double cnt = (double)(end < nr2 ? end : nr2);
                // in front of the cell: lower bound from the pieces in front, upper bound with this piece's (all of
                // its others: an upper bound may always take in more)
                const double hiT = fmax(Tx, pTx) * UP;
                thrTb = asv_thr_neg(Tx * DN, hiT, cnt, mb);
                thrPb = asv_thr_neg(Px * DN, hiT, cnt, mb);  // (prob2's chain never exceeds totalprob2's)
                // behind it: the chains stand at log(1 + others)
                thrTa = asv_thr_self(Tx * DN, mb);
                thrPa = asv_thr_self(Px * DN, mb);
                Tx = fmax(Tx, pTx);
                Px = fmax(Px, pPx);
                mTx = mPx = NEG;
                par ^= 1;
                return smx[16] != 0.0;
            },
            [&](double code, double lw, int o) {
                const bool behind = o > spos;
                const double tT = behind ? thrTa : thrTb, tP = behind ? thrPa : thrPb;
                const double up = lw * UP;  // (the log-weight is at most this)
                if (o < nr2 && (code == 3.0 || up >= tT || (code >= 1.0 && up >= tP))) {
                    const int pos = atomicAdd(&sh_sel[0], 1);
                    if (pos < lcap) giO[pos] = o;
                }
            });
        __syncthreads();
        ok = sh_sel[0] <= lcap_c;
    }
    return ok;
}

// cell_literal_reeval: (e) the kept addends, recomputed in the reference's order of operations (asv_pair_literal) and
// sorted, into the cell's lists LO / LR / LS; their lengths into sh_K.  Returns the number of kept addends.
template <int NB8>
__device__ __forceinline__ unsigned long long cell_literal_reeval(const TileLds& lds, const TileCtx& tc, int c) {
    const int tid = threadIdx.x;
    const double POS = __builtin_inf();
    const int g = tc.g;
    const int GP = tc.GP;
    const int nr2 = tc.nr2;
    const int lcap = tc.lcap;
    const int c0 = tc.c0;
    const double sigma2 = tc.sigma2;
    const double* const S = tc.S;
    const int32_t* const sid = tc.sid;
    double* const cx = lds.cx;
    double* const cg = lds.cg;
    double* const ub = lds.ub;
    int* const sh_sel = lds.sh_sel;
    int (*const sh_K)[3] = lds.sh_K;
    double* const LO = tc.wg + tc.L.LO;  // [16][lcap][2]
    double* const LR = tc.wg + tc.L.LR;  // [16][lcap]
    double* const LS = tc.wg + tc.L.LS;  // [16][lcap][2]
    int32_t* const giO = reinterpret_cast<int32_t*>(tc.wg + tc.L.GI);  // [3][lcap]: the index lists, reused per cell
    int32_t* const giR = reinterpret_cast<int32_t*>(tc.wg + tc.L.GI) + lcap;
    int32_t* const giS = reinterpret_cast<int32_t*>(tc.wg + tc.L.GI) + 2 * lcap;
    const double curproj = lds.sc_proj[c];
    const int gs_rt = NB8 > 0 ? NB8 * 8 : tc.g;  // row stride of the gathered stream
    const int KO = sh_sel[0], KR = sh_sel[1], KS = sh_sel[2];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");  // (the index lists went to global memory)
    int* ib = reinterpret_cast<int*>(ub);
    const double* cur = cx + c * GP;
    const double* grd = cg + c * GP;
    const int lsort = lcap < asv_tile_lsort(g) ? lcap : asv_tile_lsort(g);
    // an index list ascending: in the LDS (-> ib) up to 4 lsort entries, else where it lies
    auto sorted_ints = [&](int32_t* gi, int cnt) -> const int32_t* {
        int np2 = 1;
        while (np2 < cnt) np2 <<= 1;
        if (np2 > 4 * lsort) {
            for (int i = cnt + tid; i < np2; i += T) gi[i] = 0x7fffffff;
            asv_sort_global(gi, np2, ib, 4 * lsort, tid, [](int x, int y) { return x < y; });
            return gi;
        }
        for (int i = tid; i < np2; i += T) ib[i] = i < cnt ? gi[i] : 0x7fffffff;
        __syncthreads();
        for (int k = 2; k <= np2; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < np2; i += T) {
                    const int ixj = i ^ j;
                    if (ixj > i) {
                        const int x0 = ib[i], x1 = ib[ixj];
                        if (((i & k) == 0) ? x0 > x1 : x0 < x1) {
                            ib[i] = x1;
                            ib[ixj] = x0;
                        }
                    }
                }
                __syncthreads();
            }
        return ib;
    };
    {
        const int32_t* ix = sorted_ints(giR, KR);  // totalprob1's chain runs in restrict order (:117-131)
        for (int i = tid; i < KR; i += T) {
            double pr, lw;
            asv_pair_literal(cur, grd, S + ((int64_t)nr2 + ix[i]) * gs_rt, g, sigma2, pr, lw);
            LR[(int64_t)c * lcap + i] = lw;
        }
        __syncthreads();
    }
    {
        const int32_t* ix = sorted_ints(giO, KO);  // totalprob2's and prob2's likewise (:78-109)
        for (int i = tid; i < KO; i += T) {
            const int j = ix[i];
            double pr = 0.0, lw = 0.0;
            bool add = true;
            if (sid[j] != c0 + c) {  // :84
                asv_pair_literal(cur, grd, S + (int64_t)j * gs_rt, g, sigma2, pr, lw);
                add = !(pr > curproj);  // :90-92
            }
            LO[((int64_t)c * lcap + i) * 2] = lw;
            LO[((int64_t)c * lcap + i) * 2 + 1] = add ? 1.0 : 0.0;
        }
        __syncthreads();
    }
    // the walk's chain runs over the (projection, log-weight) pairs as std::sort orders them (:134)
    int np2 = 1;
    while (np2 < KS) np2 <<= 1;
    if (np2 <= lsort) {
        double* kp = ub;
        double* kw = ub + lsort;
        for (int i = tid; i < np2; i += T) {
            double pr = POS, lw = POS;
            if (i < KS) asv_pair_literal(cur, grd, S + ((int64_t)nr2 + giS[i]) * gs_rt, g, sigma2, pr, lw);
            kp[i] = pr;
            kw[i] = lw;
        }
        __syncthreads();
        for (int k = 2; k <= np2; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < np2; i += T) {
                    const int ixj = i ^ j;
                    if (ixj > i) {
                        const double p0 = kp[i], w0 = kw[i], p1 = kp[ixj], w1_ = kw[ixj];
                        const bool up = (i & k) == 0;
                        if (up ? pair_less(p1, w1_, p0, w0) : pair_less(p0, w0, p1, w1_)) {
                            kp[i] = p1;
                            kw[i] = w1_;
                            kp[ixj] = p0;
                            kw[ixj] = w0;
                        }
                    }
                }
                __syncthreads();
            }
        for (int i = tid; i < KS; i += T) {
            LS[((int64_t)c * lcap + i) * 2] = kp[i];
            LS[((int64_t)c * lcap + i) * 2 + 1] = kw[i];
        }
    } else {  // a long list: sorted where it lies, through an LDS window
        typedef double d2a __attribute__((ext_vector_type(2)));
        d2a* L2 = reinterpret_cast<d2a*>(LS + (int64_t)c * lcap * 2);
        for (int i = tid; i < np2; i += T) {
            double pr = POS, lw = POS;
            if (i < KS) asv_pair_literal(cur, grd, S + ((int64_t)nr2 + giS[i]) * gs_rt, g, sigma2, pr, lw);
            L2[i] = d2a{pr, lw};
        }
        asv_sort_global(L2, np2, reinterpret_cast<d2a*>(ub), lsort, tid,
                        [](const d2a& x, const d2a& y) { return pair_less(x[0], x[1], y[0], y[1]); });
    }
    if (tid == 0) {
        sh_K[c][0] = KO;
        sh_K[c][1] = KR;
        sh_K[c][2] = KS;
    }
    __syncthreads();
    return (unsigned long long)KO + KR + KS;
}

// ---- the histogram way: the crossing bin of the histogram (round 0: cell_first_histogram's), collected, sorted and walked; a
// bin that is still too full is subdivided.  Returns the quantile.
__device__ __forceinline__ double cell_histogram_quantile(const TileLds& lds, const TileCtx& tc, int c, const CellWalk& cw, double prob2) {
    const int tid = threadIdx.x;
    const double POS = __builtin_inf();
    const double FIX = 1099511627776.0;  // 2^40: the histogram's fixed-point unit
    const int nr1 = tc.nr1;
    const int nr2 = tc.nr2;
    const int rot0 = tc.rot0;
    const int last_block = tc.last_block;
    double* const SP = tc.SP;
    double* const SW = tc.SW;
    double* const lp = lds.ub;  // [CAP] collected projections
    unsigned long long* const lw_ = reinterpret_cast<unsigned long long*>(lds.ub + AT_CAP);  // [CAP] and their weights
    double* const sc_hi = lds.sc_hi;
    double* const sc_tmp = lds.sc_tmp;
    double* const sm = lds.sm;
    unsigned long long* const hist = lds.hist;
    int& sh_cnt = *lds.sh_cnt;
    int& sh_bin = *lds.sh_bin;
    unsigned long long& sh_before = *lds.sh_before;
    const double mx = cw.mx;
    // (own batch: streamed cells [0, nr2); reference batch: [nr2, N))
    auto w1 = [&](int64_t o_) { return SW[AsvTileLayout::at(c + rot0, (int)((nr2 + o_) >> 6), (int)((nr2 + o_) & 63))]; };
    double blo = cw.blo, bhi = cw.bhi;      // projections still in play: [blo, bhi]
    unsigned long long before = 0;          // weight of the projections below blo
    double target = -1.0;                   // in fixed-point units, known after the first histogram
    double ref_quan = sc_hi[c];             // default: the last one (:141)
    for (int round = 0; round < 40; ++round) {
        if (round > 0) {  // (round 0's histogram is the one taken above)
            for (int b = tid; b < AT_NB; b += T) hist[b] = 0ull;
            if (tid == 0) sh_cnt = 0;
            __syncthreads();
        }
        const double scale = bhi > blo ? (double)AT_NB / (bhi - blo) : 0.0;
        if (round > 0) {
            asv_row_scan<true>(SP, SW, nr2, nr1, c + rot0, last_block, tid, [&](double pr, double lw, int o) {
                const bool in = o < nr1 && pr >= blo && pr <= bhi;
                int b = (int)((pr - blo) * scale);
                b = b < 0 ? 0 : (b > AT_NB - 1 ? AT_NB - 1 : b);
                const double wv = exp(lw - mx) * FIX;
                // (an element out of play adds nothing to a bin of the thread's own: no branch, no pile-up on one bin)
                atomicAdd(&hist[in ? b : (tid & (AT_NB - 1))], in ? (unsigned long long)wv : 0ull);
            });
            __syncthreads();
        }
        const double ep2 = exp(prob2);
        const int at = asv_first_crossing(
            hist, AT_NB, before,
            [&](unsigned long long tot) { return round == 0 ? ep2 * (double)tot : target; },  // the target (:137), fixed-point units
            reinterpret_cast<unsigned long long*>(sm), &sh_bin, &sh_before, &target);
        if (at < 0) {  // no prefix reaches the target: the last projection (:141)
            ref_quan = sc_hi[c];
            break;
        }
        before = sh_before;
        // the projections that fall into bin `at`
        asv_row_scan<false>(SP, SW, nr2, nr1, c + rot0, last_block, tid, [&](double pr, double, int o) {
            int b = (int)((pr - blo) * scale);
            b = b < 0 ? 0 : (b > AT_NB - 1 ? AT_NB - 1 : b);
            if (!(o < nr1 && pr >= blo && pr <= bhi && b == at)) return;  // (rare: one bin of 2 048)
            const int pos = atomicAdd(&sh_cnt, 1);
            if (pos < AT_CAP) {
                lp[pos] = pr;
                lw_[pos] = (unsigned long long)(exp(w1(o) - mx) * FIX);
            }
        });
        __syncthreads();
        const int cnt = sh_cnt;
        if (cnt <= AT_CAP || !(bhi > blo)) {
            const int m = cnt < AT_CAP ? cnt : AT_CAP;
            int npad = 1;
            while (npad < m) npad <<= 1;
            for (int i = m + tid; i < npad; i += T) {
                lp[i] = POS;
                lw_[i] = 0ull;
            }
            __syncthreads();
            for (int k = 2; k <= npad; k <<= 1)
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int i = tid; i < npad; i += T) {
                        const int ixj = i ^ j;
                        if (ixj > i) {
                            const double a = lp[i], b2 = lp[ixj];
                            const unsigned long long wa = lw_[i], wb = lw_[ixj];
                            const bool up = (i & k) == 0;
                            // (projection, weight) ascending: equal projections in a fixed order
                            const bool gt = a > b2 || (a == b2 && wa > wb);
                            const bool lt = a < b2 || (a == b2 && wa < wb);
                            if (up ? gt : lt) {
                                lp[i] = b2;
                                lp[ixj] = a;
                                lw_[i] = wb;
                                lw_[ixj] = wa;
                            }
                        }
                    }
                    __syncthreads();
                }
            double tg2;
            const int hit = asv_first_crossing(
                lw_, m, before, [&](unsigned long long) { return target; },
                reinterpret_cast<unsigned long long*>(sm), &sh_bin, &sh_before, &tg2);
            if (tid == 0) sc_tmp[1] = hit >= 0 ? lp[hit] : (m > 0 ? lp[m - 1] : bhi);
            __syncthreads();
            ref_quan = sc_tmp[1];
            break;
        }
        // still too many in one bin: its range becomes the whole histogram
        const double nlo = blo + (double)at / scale, nhi = blo + (double)(at + 1) / scale;
        // (rounding of the bin edges: widen by an ulp-ish margin and keep inside the old range; entries that
        // fall outside the bin but inside the widened range are binned again, which is harmless -- except that
        // the weight below the range must then not contain them: recompute `before` as the weight below nlo)
        const double margin = 4e-16 * fmax(fabs(blo), fabs(bhi));
        blo = fmax(blo, nlo - margin);
        bhi = fmin(bhi, nhi + margin);
        ref_quan = bhi;  // (provisional: the quantile lies in [blo, bhi]; final unless another round refines it)
        unsigned long long mine = 0;
        asv_row_scan<true>(SP, SW, nr2, nr1, c + rot0, last_block, tid, [&](double pr, double lw, int o) {
            const double wv = exp(lw - mx) * FIX;
            mine += o < nr1 && pr < blo ? (unsigned long long)wv : 0ull;
        });
        // integer sums: any order gives the same total
        __syncthreads();
        before = block_sum(mine, reinterpret_cast<unsigned long long*>(sm));
    }
    return ref_quan;
}

// ---- 6. the literal re-run's chains: one lane per chain, the reference's sequential sums (:96-109, :127-131), then
// one lane per cell for the walk (:137-157)
__device__ __forceinline__ void tile_literal_chains(const TileLds& lds, const TileCtx& tc) {
    const int tid = threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int w = threadIdx.x >> 6;
    const int n2 = tc.n2;
    const int lcap = tc.lcap;
    const int c0 = tc.c0;
    double* const out = tc.out;
    double* const sc_proj = lds.sc_proj;
    double* const sc_l2 = lds.sc_l2;
    int (*const sh_K)[3] = lds.sh_K;
    double (*const sh_chain)[3] = lds.sh_chain;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");  // (the lists were written by other threads of the block)
    const double* LO = tc.wg + tc.L.LO;
    const double* LR = tc.wg + tc.L.LR;
    const double* LS = tc.wg + tc.L.LS;
    // (one WAVE per kind of sum -- total, counted, reference, walk --, a lane per cell: lanes of one wave on different
    // kinds would take their loops one after the other)
    static_assert(T == 256, "the chains take the block's four waves");
    if (lane < AT_C) {
        const int c = lane, which = w;
        const int KO = sh_K[c][0];
        if (KO >= 0) {
            double acc = 0.0;
            bool first = true;
            // (a chain is ONE lane's sequential sum: its addends are asked for eight at a time, ahead of the adds that use
            // them -- one by one, a step of the chain was a global load's round trip plus the add: 0.95 us, 59 ms for a
            // cell of config 5 at sigma 1 with 94 000 kept addends, the launch waiting for it)
            if (which < 2) {
                const double* L = LO + (int64_t)c * lcap * 2;
                int i = 0;
                for (; i + 8 <= KO; i += 8) {
                    double lw[8], fl[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        lw[u] = L[2 * (i + u)];
                        fl[u] = L[2 * (i + u) + 1];
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        if (which == 0 || fl[u] != 0.0) {
                            acc = first ? lw[u] : bmx_pm_logspace_add(acc, lw[u]);
                            first = false;
                        }
                }
                for (; i < KO; ++i) {
                    const double lw = L[2 * i];
                    if (which == 0 || L[2 * i + 1] != 0.0) {
                        acc = first ? lw : bmx_pm_logspace_add(acc, lw);
                        first = false;
                    }
                }
            } else if (which == 3) {
                // the walk's running sums (:147-151) do not depend on where the walk stops: a fourth lane takes them
                // WHILE the three chains run (the walk used to start when they were through: twice the sequential
                // length) and leaves sum i in the place of log-weight i; they never decrease (a log-sum is at least its
                // larger term), so the walk's stop is then a binary search for the target
                double* L = const_cast<double*>(LS) + (int64_t)c * lcap * 2;
                const int KS = sh_K[c][2];
                double cum = 0.0;
                int i = 0;
                for (; i + 8 <= KS; i += 8) {
                    double lw[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) lw[u] = L[2 * (i + u) + 1];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        cum = i + u == 0 ? lw[u] : bmx_pm_logspace_add(cum, lw[u]);
                        lw[u] = cum;
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) L[2 * (i + u) + 1] = lw[u];
                }
                for (; i < KS; ++i) {
                    cum = i == 0 ? L[1] : bmx_pm_logspace_add(cum, L[2 * i + 1]);
                    L[2 * i + 1] = cum;
                }
            } else {
                const double* L = LR + (int64_t)c * lcap;
                const int KR = sh_K[c][1];
                int i = 0;
                for (; i + 8 <= KR; i += 8) {
                    double lw[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) lw[u] = L[i + u];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        acc = first ? lw[u] : bmx_pm_logspace_add(acc, lw[u]);
                        first = false;
                    }
                }
                for (; i < KR; ++i) {
                    acc = first ? L[i] : bmx_pm_logspace_add(acc, L[i]);
                    first = false;
                }
            }
            if (which < 3) sh_chain[c][which] = acc;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");  // (the walk's sums, written by one wave, read by another)
    __syncthreads();
    if (tid < AT_C && c0 + tid < n2 && sh_K[tid][0] >= 0) {
        const int c = tid, KS = sh_K[c][2];
        const double* L = LS + (int64_t)c * lcap * 2;
        const double tgt = (sh_chain[c][1] - sh_chain[c][0]) + sh_chain[c][2];  // :111, :138
        // the first place whose running sum reaches the target (:147-151; the sums stand where the log-weights stood and
        // never decrease), the last projection if none does (:141; a NaN target: none)
        int lo_ = 0, hi_ = KS;
        while (lo_ < hi_) {
            const int mid = (lo_ + hi_) >> 1;
            if (L[2 * mid + 1] >= tgt) hi_ = mid;
            else lo_ = mid + 1;
        }
        const double rq = L[2 * (lo_ < KS ? lo_ : KS - 1)];
        out[c0 + c] = (rq - sc_proj[c]) / sc_l2[c];  // :160
    }
}

// diagnostics (bmx_dev_get "asv_ticks_stream" / "_wait" / "_cells"): 100 MHz ticks the workgroups of the tiled form spent in the
// stream, at the round barrier and in the per-cell phase, added up over all workgroups since the last "asv_tally_reset"
__device__ unsigned long long g_asv_ticks[8];  // stream, barrier wait, per-cell phase, (spare); literal cells: selection + re-evaluation + sort, chains + walk, kept addends, tiles with chains

template <int NB8>
__global__ __launch_bounds__(T) void asv_tile_kernel(int g, const double* __restrict__ data2, int n2,
                                                     const double* __restrict__ vect, double sigma2, int nr1, int nr2,
                                                     const double* __restrict__ S, const double* __restrict__ snrm,
                                                     const int32_t* __restrict__ sid, double* __restrict__ out,
                                                     double* __restrict__ scratch, int cell_begin, int cell_end, int lcap,
                                                     unsigned long long* __restrict__ tally, unsigned int* __restrict__ gbar,
                                                     unsigned int* __restrict__ tile_ctr, unsigned char* __restrict__ modes) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int GP = asv_tile_gp(g);
    double* cx = reinterpret_cast<double*>(smem_raw);
    double* cg = cx + AT_C * GP;
    double* ub = cg + AT_C * GP;
    double* rs = ub + asv_tile_ub_doubles(g, lcap);
    double* sc = rs + (NB8 == 0 ? AT_R * (AT_KC + 2) : 0);  // 8 x [16] per-cell values, then etab [32], then sm
    double* sm = sc + 8 * AT_C + 32;
    unsigned long long* hist = reinterpret_cast<unsigned long long*>(sm + AT_SM);
    __shared__ int sh_cnt, sh_bin, sh_tile;
    __shared__ unsigned long long sh_before;
    __shared__ int sh_sel[4];
    __shared__ int sh_K[AT_C][3];
    __shared__ double sh_chain[AT_C][3];
    const TileLds lds = {cx, cg, ub, rs, sc, sc + AT_C, sc + 2 * AT_C, sc + 3 * AT_C, sc + 4 * AT_C, sc + 5 * AT_C, sc + 6 * AT_C, sc + 7 * AT_C,
                         sc + 8 * AT_C, sm, hist, hist + AT_NB, &sh_cnt, &sh_bin, &sh_before, sh_sel, sh_K, sh_chain};
    const int tid = threadIdx.x;
    // the tile's scratch: per block of 64 streamed cells, 16 rows (cells) of 64 values -- a step of the stream writes ONE
    // contiguous 8 KB piece of each array (the [cell][N] layout of the first version wrote 32 rows 8 MB apart per step and
    // spent its time in address translation), and a cell's row is 512-byte pieces 8 KB apart, read by whole waves
    const AsvTileLayout L(g, nr1, nr2, lcap, 0, 1);  // (the per-workgroup part is all the kernel takes from it)
    double* wg = scratch + (int64_t)blockIdx.x * L.per_block;
    // (a rank of a multi-GPU run owns the cells [cell_begin, cell_end) only; n2 below and in the phases is the end of that range)
    TileCtx tc = {g, GP, nr1, nr2, cell_end, lcap, sigma2, ASV_LIT_ON && lcap > 0, (int64_t)nr1 + nr2, L.N, L.Nown, data2, vect, S, snrm, sid, out, L,
                  wg, wg + L.SP, wg + L.SW, reinterpret_cast<float*>(wg + L.SO), (int)blockIdx.x, (int)(L.N >> 6) - 1, 0};
    n2 = cell_end;
    const int ntiles = (cell_end - cell_begin + AT_C - 1) / AT_C;
    unsigned long long tk_stream = 0, tk_wait = 0, tk_cells = 0, tk0 = 0, tk1 = 0;  // (thread 0's)
    unsigned long long tk_lit = 0, tk_chain = 0, tk_lit_n = 0, tk_chain_tiles = 0;   // (the literal re-run's share of tk_cells)

    // Tiles are handed out as workgroups come free (round 6: a counter on the device): a tile with flagged cells takes several
    // times a plain one -- with tiles dealt in a fixed stride the workgroups of a launch ended 11 % apart on config 5 at
    // sigma 1 (5.7 % without the re-run).  Every cell's value is independent of which workgroup computes it and when.  (With the
    // testing hook "asv_sync" the rounds need the fixed deal.)
    for (int tile = blockIdx.x;; ) {
        if (tile_ctr && !gbar) {
            __syncthreads();  // (sh_tile of the previous turn has been read by everybody)
            if (tid == 0) sh_tile = (int)atomicAdd(tile_ctr, 1u);
            __syncthreads();
            tile = sh_tile;
        }
        if (tile >= ntiles) break;
        const int c0 = tc.c0 = cell_begin + tile * AT_C;
        tile_load_cells(lds, tc);
        tk0 = __builtin_amdgcn_s_memrealtime();
        if (gbar) tile_round_barrier(gbar, tile, ntiles);
        tk1 = __builtin_amdgcn_s_memrealtime();
        tk_wait += tk1 - tk0;
        tile_stream<NB8>(lds, tc);
        tk0 = __builtin_amdgcn_s_memrealtime();
        tk_stream += tk0 - tk1;
        // ---- cell by cell: own-batch probability, then the weighted quantile of the reference projections
        const double nmax_s = snrm[tc.Npad];  // the largest squared norm of a streamed cell (asv_max_norm; bounds the rounding of the GEMM-form distances)
        if (tid < AT_C) sh_K[tid][0] = -1;
        int n_lit = 0, n_back = 0;  // (thread 0's tallies: cells re-run literally, flagged cells that went the histogram way)
        for (int c = 0; c < AT_C && c0 + c < n2; ++c) {
            const double curproj = lds.sc_proj[c], l2 = lds.sc_l2[c];
            const double prob2 = lds.sc_mx2[c];  // (taken online by the stream)
            double ref_quan = __builtin_nan("");
            bool literal = false;
            int cell_mode = 0;  // 0: the histogram way (not flagged), 1: re-run literally, 2: flagged, beyond the re-run
            if (nr1 > 0) {
                CellWalk cw = {lds.sc_mx1[c], lds.sc_lo[c], lds.sc_hi[c], 0.0};
                // Flagged: (i) the own batch's cumulative probability at the cell is 1 to within 1e-6, i.e. the walk over the
                // reference batch runs to where all but 1e-6 of the weight has gone by -- and is decided by single addends of
                // relative size <= 1e-6, far enough down for the rounding of the two summation orders to matter; (ii) it is below
                // e^-12 (a cell that is not in its own batch's restrict vector can sit far below all the weight): the walk ends
                // among addends the 2^-40 fixed-point weights of the histogram do not resolve.  (Cells in between cross on
                // addends the histogram way resolves.)  How long a re-run a flagged cell is worth: within 1e-9 of 1 (or below
                // e^-12) the walk IS a statement about rounding and the histogram way picks another quantile on most such cells:
                // up to lcap addends per chain; between 1e-9 and 1e-6 the histogram way is right on all but a few cells of a
                // small call (and on every sampled cell of config 5 at sigma 1), and a re-run of tens of thousands of addends for
                // each of the 2.5 % of config 5's cells that sit there doubled the step: up to 8 192.
                const bool ill = -prob2 < 1e-6 || prob2 < -12.0;
                const bool flagged = tc.lit_on && ill;
                const int lcap_c = (-prob2 < 1e-9 || prob2 < -12.0) ? lcap : (lcap < 8192 ? lcap : 8192);
                const int cG = cell_first_histogram(lds, tc, c, flagged, cw);
                if (flagged) {
                    if (cG <= lcap_c) {
                        const unsigned long long tkl0 = __builtin_amdgcn_s_memrealtime();
                        if (cell_literal_select(lds, tc, c, lcap_c, cw, nmax_s)) {
                            tk_lit_n += cell_literal_reeval<NB8>(lds, tc, c);
                            literal = true;
                            ++n_lit;
                        }
                        tk_lit += __builtin_amdgcn_s_memrealtime() - tkl0;
                    }
                    if (!literal) ++n_back;
                    cell_mode = literal ? 1 : 2;
                } else if (modes && ill) {
                    cell_mode = 2;  // strict mode, no re-run at all (lcap = 0): the flag holds whatever lcap is
                }
                if (!literal) ref_quan = cell_histogram_quantile(lds, tc, c, cw, prob2);
            }
            if (!literal && tid == 0) out[c0 + c] = (ref_quan - curproj) / l2;  // :160
            // (testing hook "asv_modes": which way every cell went, one byte per cell behind the tallies)
            if (tid == 0 && tally && (unsigned long long)(c0 + c) < tally[3])
                reinterpret_cast<unsigned char*>(tally + 4)[c0 + c] = (unsigned char)cell_mode;
            // (strict mode: the call's own record, which the strict pass compacts into the list of mode-2 cells)
            if (tid == 0 && modes) modes[c0 + c] = (unsigned char)cell_mode;
            __syncthreads();
        }
        if (tc.lit_on) {
            const unsigned long long tkc0 = __builtin_amdgcn_s_memrealtime();
            const bool any_lit = n_lit > 0;  // (thread 0's count is the tile's)
            tile_literal_chains(lds, tc);
            // ---- 7. tallies and ticks
            if (any_lit) {
                tk_chain += __builtin_amdgcn_s_memrealtime() - tkc0;
                ++tk_chain_tiles;
            }
            if (tid == 0 && tally) {
                atomicAdd(&tally[0], (unsigned long long)n_lit);
                atomicAdd(&tally[1], (unsigned long long)n_back);
                atomicAdd(&tally[2], (unsigned long long)(n2 - c0 < AT_C ? n2 - c0 : AT_C));
            }
            __syncthreads();
        }
        tk_cells += __builtin_amdgcn_s_memrealtime() - tk0;
        if (!(tile_ctr && !gbar)) tile += gridDim.x;  // (the fixed deal)
    }
    if (tid == 0) {
        atomicAdd(&g_asv_ticks[0], tk_stream);
        atomicAdd(&g_asv_ticks[1], tk_wait);
        atomicAdd(&g_asv_ticks[2], tk_cells);
        if (tk_lit | tk_chain) {
            atomicAdd(&g_asv_ticks[4], tk_lit);
            atomicAdd(&g_asv_ticks[5], tk_chain);
            atomicAdd(&g_asv_ticks[6], tk_lit_n);
            atomicAdd(&g_asv_ticks[7], tk_chain_tiles);
        }
    }
}

}  // namespace

// Counters of the tiled form, per device, for tests and bench.py (bmx_dev_get "asv_literal_cells" / "asv_fallback_cells" /
// "asv_tiled_cells"): cells re-run literally, flagged cells that went the histogram way (more than lcap kept addends),
// all cells the tiled form has handled.  Added up until "asv_tally_reset".
// Testing hook "asv_modes" = n: the tiled form also records which way each of the first n cells of a call went (one byte
// per cell behind the four tally words: 0 the histogram way, 1 re-run literally, 2 flagged but beyond the re-run); the LAST
// call's bytes stay (bmx_dev_get_bytes "asv_modes").
static unsigned long long* g_tally[64] = {};
static size_t g_tally_modes[64] = {};
static long long g_tally_cap_set[64] = {};  // what word 3 holds + 1 (0: unknown)
static std::mutex g_tally_mu;  // (several host threads may drive engines on one device: the buffer is made and regrown under it)
unsigned long long* asv_tally_device() {
    int dev = 0;
    BMX_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(g_tally_mu);
    const size_t want = (size_t)std::max(0, dev_knobs().asv_modes);
    if (!g_tally[dev] || g_tally_modes[dev] < want) {
        unsigned long long keep[4] = {0, 0, 0, 0};
        if (g_tally[dev]) {
            BMX_HIP(hipDeviceSynchronize());
            BMX_HIP(hipMemcpy(keep, g_tally[dev], 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            (void)hipFree(g_tally[dev]);
            g_tally[dev] = nullptr;
        }
        BMX_HIP(hipMalloc(reinterpret_cast<void**>(&g_tally[dev]), 4 * sizeof(unsigned long long) + want + 8));
        BMX_HIP(hipMemset(g_tally[dev], 0, 4 * sizeof(unsigned long long) + want + 8));
        BMX_HIP(hipMemcpy(g_tally[dev], keep, 3 * sizeof(unsigned long long), hipMemcpyHostToDevice));
        g_tally_modes[dev] = want;
        g_tally_cap_set[dev] = 0;
    }
    if (g_tally_cap_set[dev] != (long long)want + 1) {  // (only when the hook changes: a blocking copy otherwise never happens)
        const unsigned long long cap = (unsigned long long)want;  // (0: no modes recorded)
        BMX_HIP(hipMemcpy(g_tally[dev] + 3, &cap, sizeof(cap), hipMemcpyHostToDevice));
        g_tally_cap_set[dev] = (long long)want + 1;
    }
    return g_tally[dev];
}
void asv_modes_read(unsigned char* dst, size_t n) {
    unsigned long long* t = asv_tally_device();
    int dev = 0;
    BMX_HIP(hipGetDevice(&dev));
    if (!t || dev < 0 || dev >= 64) {  // (a device beyond the table: nothing was recorded)
        for (size_t i = 0; i < n; ++i) dst[i] = 255;
        return;
    }
    BMX_HIP(hipDeviceSynchronize());
    const size_t have = std::min(n, g_tally_modes[dev]);
    if (have) BMX_HIP(hipMemcpy(dst, t + 4, have, hipMemcpyDeviceToHost));
    for (size_t i = have; i < n; ++i) dst[i] = 255;
}
void asv_tally_read(unsigned long long out[3], bool reset) {
    unsigned long long* t = asv_tally_device();
    out[0] = out[1] = out[2] = 0;
    if (!t) return;
    BMX_HIP(hipDeviceSynchronize());
    BMX_HIP(hipMemcpy(out, t, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (reset) {
        BMX_HIP(hipMemset(t, 0, 3 * sizeof(unsigned long long)));
        const unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        BMX_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_asv_ticks), z, sizeof(z)));
    }
}
void asv_ticks_read(unsigned long long out[8]) {
    unsigned long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    BMX_HIP(hipDeviceSynchronize());
    BMX_HIP(hipMemcpyFromSymbol(v, HIP_SYMBOL(g_asv_ticks), sizeof(v)));
    for (int i = 0; i < 8; ++i) out[i] = v[i];
}

static int device_cu_count() {
    static int cus[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    if (cus[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 0;
        cus[dev] = n > 0 ? n : -1;
    }
    return cus[dev] > 0 ? cus[dev] : 0;
}

void launch_asv_tile(hipStream_t stream, const double* data1, int g, const double* data2, int n2, const double* vect,
                     int vect_row_major, double sigma2, const int32_t* restrict1, int nr1, const int32_t* restrict2, int nr2,
                     double* out, double* ws_pairs, const AsvPlan& pl, int cell_begin, int cell_end, unsigned char* modes) {
    if (g > 256) throw Error(BMX_ERR_ARG, "adjust_shift_variance: more than 256 dimensions at this size are not supported");
    const int blocks = pl.blocks;
    const AsvTileLayout L(g, nr1, nr2, pl.lcap, n2, vect_row_major);
    double* extra = ws_pairs + pl.main_doubles;
    const int64_t N = L.N;
    const int gs = asv_tile_gs(g);
    double* S = extra + L.S;        // [N][gs] the streamed cells, zero rows up to whole pairs of steps
    double* snrm = extra + L.snrm;  // [N] + their maximum
    int32_t* sid = reinterpret_cast<int32_t*>(extra + L.sid);  // [N]
    const double* vrm = vect;
    if (!vect_row_major) {
        double* t = extra + L.vect_rm;
        transpose_cm_to_rm(stream, vect, n2, g, t);
        vrm = t;
    }
    BMX_HIP(hipMemsetAsync(extra + L.snrm_max, 0, sizeof(double), stream));
    hipLaunchKernelGGL(asv_gather_stream, dim3((unsigned)cdiv(N, 4)), dim3(256), 0, stream, data1, data2, g, gs, restrict1, nr1,
                       restrict2, nr2, N, S, snrm, sid);
    // the round barrier of the tile kernel needs every workgroup of the launch resident at once: one workgroup per CU is
    // always possible (its LDS and registers fit a CU by construction), so the launch must not be wider than the device
    // (testing hook "asv_sync" = 0: no barrier, round 5's free-running tiles)
    unsigned int* gbar = nullptr;
    if (dev_knobs().asv_sync != 0 && blocks <= device_cu_count()) gbar = reinterpret_cast<unsigned int*>(extra + L.gbar);
    unsigned int* tile_ctr = reinterpret_cast<unsigned int*>(extra + L.tile_ctr);
    hipLaunchKernelGGL(asv_max_norm, dim3(256), dim3(256), 0, stream, snrm, N, gbar, tile_ctr);
    const size_t lds = asv_tile_lds_bytes(g, pl.lcap);
    unsigned long long* tally = asv_tally_device();
#define BMX_ASV_TILE(NB8)                                                                                                    \
    case NB8:                                                                                                                \
        ensure_dynamic_lds(reinterpret_cast<const void*>(&asv_tile_kernel<NB8>), lds);                                       \
        hipLaunchKernelGGL(asv_tile_kernel<NB8>, dim3(blocks), dim3(T), lds, stream, g, data2, n2, vrm, sigma2, nr1, nr2,     \
                           (const double*)S, (const double*)snrm, (const int32_t*)sid, out, ws_pairs, cell_begin, cell_end,  \
                           pl.lcap, tally, gbar, tile_ctr, modes);                                                         \
        break
    switch (asv_tile_nb8(g)) {
#ifdef BMX_ASV_AB_ONLY13
        BMX_ASV_TILE(13);
#else
        BMX_ASV_TILE(1);
        BMX_ASV_TILE(2);
        BMX_ASV_TILE(3);
        BMX_ASV_TILE(4);
        BMX_ASV_TILE(5);
        BMX_ASV_TILE(6);
        BMX_ASV_TILE(7);
        BMX_ASV_TILE(8);
        BMX_ASV_TILE(9);
        BMX_ASV_TILE(10);
        BMX_ASV_TILE(11);
        BMX_ASV_TILE(12);
        BMX_ASV_TILE(13);
        BMX_ASV_TILE(14);
        BMX_ASV_TILE(15);
        BMX_ASV_TILE(16);
#endif
        default:
            BMX_ASV_TILE(0);
    }
#undef BMX_ASV_TILE
    BMX_LAUNCH_CHECK();
}

}  // namespace bmx
