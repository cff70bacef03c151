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

void adjust_shift_variance_device(hipStream_t stream, const double* data1, int g, int n1, const double* data2, int n2,
                                  const double* vect, double sigma2, const int32_t* restrict1, int nr1,
                                  const int32_t* restrict2, int nr2, double* out, double* ws_pairs, const AsvPlan& pl,
                                  int vect_row_major, int cell_begin, int cell_end) {
    (void)n1;
    if (cell_end < 0) cell_end = n2;
    if (n2 <= 0 || cell_end <= cell_begin) return;
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
