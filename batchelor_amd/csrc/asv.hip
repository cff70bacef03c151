// HIP version of adjust_shift_variance (src/adjust_shift_variance.cpp:30-164), one of the two classic-mnnCorrect natives
// that stay registered in batchelor's .Call table (the other: smooth_gaussian_kernel, sgk.hip).  FP64 throughout.
// It comes in three forms.  Its quantile walk (sorted cumulative log-sum against a target that is
// itself a log-sum) decides on last-bit differences whenever the weights are concentrated -- in a few per cent of the
// cells of the reference's own test data -- so a form that sums in any other order picks a different CELL there, not a
// rounded value.  asv_exact_kernel (asv_literal.hip) therefore repeats the reference's order of operations literally
// (distances in parallel, then the sequential logspace_add chains in restrict order, a lexicographic sort of (projection,
// weight), the sequential walk), with the bit-reproducible exp / log1p of portable_math.hpp: bit for bit what a CPU
// following the same order of operations with the same arithmetic gets (the tests' checker does).  Its sequential chains
// cost O(cells x (nr1 + nr2)) dependent steps (1.6 ns per pair): it is taken up to 4e7 pairs per call; beyond that
// asv_tile_kernel (asv_tile.hip: 16-cell tiles on the FP64 matrix cores + a sort-free histogram quantile, 0.015 ns per pair)
// takes over and agrees except on those ill-conditioned cells (tests/testthat/test-mnn-correct.R:141,396-399 acknowledge
// the effect upstream).  Gene space beyond that size (more than 256 dimensions) goes the literal wide way (asv_literal.hip).
// This unit is the choice between them: the plan (asv_plan.hpp) and the dispatch.
#include "asv_internal.hpp"

namespace bmx {

AsvPlan adjust_shift_variance_plan(int g, int n2, int nr1, int nr2, int vect_row_major) {
    return plan_adjust_shift_variance(g, n2, nr1, nr2, vect_row_major, dev_knobs());
}

// Strict mode is on for a call that asks for it (or for every call under the testing hook "asv_strict" = 1) and whose plan
// is the tiled form: the exact and the wide form already are the reference's bits.
static bool strict_on(const AsvPlan& pl, int strict) { return (strict != 0 || dev_knobs().asv_strict == 1) && !pl.exact && !pl.wide; }

size_t adjust_shift_variance_scratch(const AsvPlan& pl, int g, int n2, int nr1, int nr2, int strict) {
    size_t n = pl.main_doubles + pl.extra_doubles;
    if (strict_on(pl, strict)) n += plan_asv_strict(g, n2, nr1, nr2, dev_knobs()).doubles;
    return n;
}

void adjust_shift_variance_device(hipStream_t stream, const double* data1, int g, int n1, const double* data2, int n2,
                                  const double* vect, double sigma2, const int32_t* restrict1, int nr1,
                                  const int32_t* restrict2, int nr2, double* out, double* ws_pairs, const AsvPlan& pl,
                                  int vect_row_major, int cell_begin, int cell_end, int strict, int64_t* counts) {
    (void)n1;
    if (counts) counts[0] = counts[1] = counts[2] = counts[3] = -1;
    if (cell_end < 0) cell_end = n2;
    if (n2 <= 0 || cell_end <= cell_begin) return;
    if (strict_on(pl, strict)) {
        // 1. the tiled form, which also records the way of every cell of the range in the call's own scratch
        const AsvStrictPlan sp = plan_asv_strict(g, n2, nr1, nr2, dev_knobs());
        double* sws = ws_pairs + pl.main_doubles + pl.extra_doubles;
        unsigned char* modes = reinterpret_cast<unsigned char*>(sws + sp.modes);
        int32_t* list = reinterpret_cast<int32_t*>(sws + sp.list);
        unsigned int* count = reinterpret_cast<unsigned int*>(sws + sp.count);
        launch_asv_tile(stream, data1, g, data2, n2, vect, vect_row_major, sigma2, restrict1, nr1, restrict2, nr2, out, ws_pairs,
                        pl, cell_begin, cell_end, modes);
        // 2. the mode-2 cells as an ascending list; its length comes to the host (the one wait strict mode adds)
        launch_asv_strict_compact(stream, modes, cell_begin, cell_end, list, count);
        unsigned int h[2] = {0, 0};
        BMX_HIP(hipMemcpyAsync(h, count, (counts ? 2 : 1) * sizeof(unsigned int), hipMemcpyDeviceToHost, stream));
        BMX_HIP(hipStreamSynchronize(stream));
        const int nlist = (int)std::min<unsigned int>(h[0], (unsigned int)(cell_end - cell_begin));
        // 3. exactly those cells again, in the reference's order of operations, over the histogram values
        const int64_t vs_cell = vect_row_major ? g : 1, vs_x = vect_row_major ? 1 : n2;
        launch_asv_strict_pass(stream, data1, g, data2, vect, vs_cell, vs_x, sigma2, restrict1, nr1, restrict2, nr2, out,
                               sws + sp.wide, sp, list, nlist);
        if (counts) {
            counts[0] = cell_end - cell_begin;
            counts[1] = (int64_t)h[1];
            counts[2] = counts[3] = nlist;
        }
        return;
    }
    if (pl.wide || pl.exact) {
        // vect is an R matrix [n2 x g] (column-major) at the .Call boundary, row-major [n2][g] inside the engine
        const int64_t vs_cell = vect_row_major ? g : 1, vs_x = vect_row_major ? 1 : n2;
        launch_asv_literal(stream, data1, g, data2, n2, vect, vs_cell, vs_x, sigma2, restrict1, nr1, restrict2, nr2, out,
                           ws_pairs, pl, cell_begin, cell_end);
    } else {
        launch_asv_tile(stream, data1, g, data2, n2, vect, vect_row_major, sigma2, restrict1, nr1, restrict2, nr2, out, ws_pairs,
                        pl, cell_begin, cell_end);
    }
}

}  // namespace bmx
