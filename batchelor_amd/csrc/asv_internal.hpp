// Device pieces that more than one of sgk.hip, asv_literal.hip and asv_tile.hip use, and the two launchers asv.hip
// dispatches to.  Everything here is one copy on purpose: the tiled form's literal re-run is bit-equal to the exact form
// because both evaluate a pair with asv_pair_literal and order pairs with pair_less.
#pragma once
#include "asv_plan.hpp"
#include "bmx_ops.hpp"
#include "portable_math.hpp"

namespace bmx {

constexpr int ASV_T = 256;  // threads of a workgroup of the adjust_shift_variance kernels

// block-wide maximum / sum of one value per thread through `sm` (ASV_T doubles of LDS); every thread gets the result
__device__ __forceinline__ double block_max(double v, double* sm) {
    const int tid = threadIdx.x;
    sm[tid] = v;
    __syncthreads();
    for (int o = ASV_T / 2; o > 0; o >>= 1) {
        if (tid < o) sm[tid] = fmax(sm[tid], sm[tid + o]);
        __syncthreads();
    }
    const double r = sm[0];
    __syncthreads();
    return r;
}

// (integer sums as well: any order gives the same total)
template <class V>
__device__ __forceinline__ V block_sum(V v, V* sm) {
    const int tid = threadIdx.x;
    sm[tid] = v;
    __syncthreads();
    for (int o = ASV_T / 2; o > 0; o >>= 1) {
        if (tid < o) sm[tid] += sm[tid + o];
        __syncthreads();
    }
    const V r = sm[0];
    __syncthreads();
    return r;
}

// exp(x) for x <= 0 in the stream's epilogue (the own batch's online log-sum-exp: one per pair, two when a new maximum arrives).
// The library's exp costs the one wave of a SIMD ~1 000 cycles a call there -- a block of own-batch rows took 2.6 times a block
// of reference rows (round 6, by phase ticks with and without the division: EXPERIMENTS.md).  Table-driven instead: x = (32 m + j)
// ln 2 / 32 + r, |r| <= ln 2 / 64, exp(x) = 2^m 2^(j / 32) (1 + r + r^2 / 2 + ... + r^6 / 720); the 32 powers sit in the LDS (tab).
// Below 2 ulp (checked against extended precision over [-700, 0]); -inf and anything below -800 give 0.
__device__ __forceinline__ double asv_exp_neg(double x, const double* tab) {
    x = fmax(x, -800.0);
    const double nf = __builtin_rint(x * 46.16624130844683);     // 32 / ln 2
    const int n = (int)nf;
    double r = __builtin_fma(nf, -0x1.62e42fee00000p-6, x);      // ln 2 / 32, high part (n times it is exact)
    r = __builtin_fma(nf, -0x1.a39ef35793c76p-38, r);            // ... low part
    double p = 1.0 / 720.0;
    p = __builtin_fma(p, r, 1.0 / 120.0);
    p = __builtin_fma(p, r, 1.0 / 24.0);
    p = __builtin_fma(p, r, 1.0 / 6.0);
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = p * r;
    const double t = tab[n & 31];
    return ldexp(__builtin_fma(t, p, t), n >> 5);
}

__device__ __forceinline__ bool pair_less(double p0, double w0, double p1, double w1) {
    return p0 < p1 || (!(p1 < p0) && w0 < w1);  // std::pair<double, double> operator<
}

// projection of `other` on the cell's line and its squared distance to it, in the reference's order of operations
// (src/adjust_shift_variance.cpp:88-89 / :120-123 inner_product, :9-27 sq_distance_to_line); cur / grad: the cell and its
// unit gradient
__device__ __forceinline__ void asv_pair_literal(const double* cur, const double* grad, const double* __restrict__ other,
                                                 int g, double sigma2, double& proj, double& lw) {
    double pr = 0.0, sc = 0.0;
    for (int x = 0; x < g; ++x) pr += grad[x] * other[x];
    for (int x = 0; x < g; ++x) sc += (cur[x] - other[x]) * grad[x];
    double dist = 0.0;
    for (int x = 0; x < g; ++x) {
        const double w = (cur[x] - other[x]) - sc * grad[x];
        dist += w * w;
    }
    proj = pr;
    lw = -dist / sigma2;
}

// The launch sequences of the three forms; the arguments are adjust_shift_variance_device's, the empty call already handled.
// vs_cell / vs_x: strides of vect by cell and by dimension (an R matrix at the .Call boundary, row-major inside the engine).
void launch_asv_literal(hipStream_t stream, const double* data1, int g, const double* data2, int n2, const double* vect,
                        int64_t vs_cell, int64_t vs_x, double sigma2, const int32_t* restrict1, int nr1,
                        const int32_t* restrict2, int nr2, double* out, double* ws_pairs, const AsvPlan& pl, int cell_begin,
                        int cell_end);
void launch_asv_tile(hipStream_t stream, const double* data1, int g, const double* data2, int n2, const double* vect,
                     int vect_row_major, double sigma2, const int32_t* restrict1, int nr1, const int32_t* restrict2, int nr2,
                     double* out, double* ws_pairs, const AsvPlan& pl, int cell_begin, int cell_end,
                     unsigned char* modes = nullptr);  // modes: strict mode's per-call record of the cells' ways, [n2], or null
// Strict mode (asv_literal.hip): the record -> the ascending list of the mode-2 cells of [cell_begin, cell_end) and
// count[0..1] = {its length, cells re-run literally}; then the wide form over list[0, count), sp.chunk entries at a time,
// writing out[cell] over the histogram value (count: what the host has read back; 0 launches nothing).
void launch_asv_strict_compact(hipStream_t stream, const unsigned char* modes, int cell_begin, int cell_end, int32_t* list,
                               unsigned int* count);
void launch_asv_strict_pass(hipStream_t stream, const double* data1, int g, const double* data2, const double* vect,
                            int64_t vs_cell, int64_t vs_x, double sigma2, const int32_t* restrict1, int nr1,
                            const int32_t* restrict2, int nr2, double* out, double* ws_wide, const AsvStrictPlan& sp,
                            const int32_t* list, int count);

}  // namespace bmx
