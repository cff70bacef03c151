// adjust_shift_variance in the reference's own order of operations (src/adjust_shift_variance.cpp:30-164): the exact form
// (asv_exact_kernel, one workgroup per cell) and the wide form (asv_wide_*, gene space, cells in chunks).  Both end in
// asv_cell_phase and give, bit for bit, what a CPU following the same order of operations with the arithmetic of
// portable_math.hpp gets.  asv.hip says when each runs; AsvLiteralLayout (asv_plan.hpp) says where a cell's values lie.
#include "asv_internal.hpp"

#include <algorithm>

namespace bmx {
namespace {

constexpr int T = ASV_T;

// ---------------------------------------------------------------------------------------------------
// adjust_shift_variance, literal order of operations (src/adjust_shift_variance.cpp:52-161), one workgroup per cell.
// scratch per workgroup: one cell's values as AsvLiteralLayout lays them out.
// ---------------------------------------------------------------------------------------------------
// The per-cell phase of adjust_shift_variance (src/adjust_shift_variance.cpp:74-160) on one workgroup, from the values of
// every pair: lw2 [nr2] log-weights of the right batch's restricted cells, add2 [nr2] (1.0: the cell counts towards prob2),
// kp / kw [npad] projection and log-weight of the left batch's (padded with +inf), sorted in place.  Thread 0 writes *out.
// The caller has made the values visible to the workgroup (a __syncthreads); sh: 3 doubles of LDS.
__device__ void asv_cell_phase(const double* __restrict__ lw2, const double* __restrict__ add2, double* __restrict__ kp,
                               double* __restrict__ kw, int nr1, int nr2, int npad, double curproj, double l2,
                               double* __restrict__ out, double* sh) {
    const int tid = threadIdx.x;
    // the three sequential log-sum chains, in restrict order (:74-112, :117-131), one wave each
    if (tid == 0) {
        double prob2 = 0.0, tot2 = 0.0;
        bool first_p = true;
        for (int s = 0; s < nr2; ++s) {
            const double lp = lw2[s];
            if (add2[s] != 0.0) {
                prob2 = first_p ? lp : bmx_pm_logspace_add(prob2, lp);
                first_p = false;
            }
            tot2 = s == 0 ? lp : bmx_pm_logspace_add(tot2, lp);
        }
        sh[0] = prob2;
        sh[1] = tot2;
    } else if (tid == 64) {
        double tot1 = 0.0;
        for (int o = 0; o < nr1; ++o) tot1 = o == 0 ? kw[o] : bmx_pm_logspace_add(tot1, kw[o]);
        sh[2] = tot1;
    }
    __syncthreads();
    // std::sort of the (projection, log-weight) pairs (:134): bitonic network over npad slots
    for (int k = 2; k <= npad; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < npad; i += T) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const double p0 = kp[i], w0 = kw[i], p1 = kp[ixj], w1 = kw[ixj];
                    const bool up = (i & k) == 0;
                    if (up ? pair_less(p1, w1, p0, w0) : pair_less(p0, w0, p1, w1)) {
                        kp[i] = p1;
                        kw[i] = w1;
                        kp[ixj] = p0;
                        kw[ixj] = w0;
                    }
                }
            }
            __syncthreads();
        }
    if (tid == 0) {  // :137-160
        double ref_quan = __builtin_nan("");
        if (nr1 > 0) {
            const double target = (sh[0] - sh[1]) + sh[2];
            double cum = 0.0;
            ref_quan = kp[nr1 - 1];
            for (int o = 0; o < nr1; ++o) {
                cum = o == 0 ? kw[o] : bmx_pm_logspace_add(cum, kw[o]);
                if (cum >= target) {
                    ref_quan = kp[o];
                    break;
                }
            }
        }
        *out = (ref_quan - curproj) / l2;
    }
    __syncthreads();
}

__global__ __launch_bounds__(T) void asv_exact_kernel(const double* __restrict__ data1, int g, const double* __restrict__ data2,
                                                      int n2, const double* __restrict__ vect, int64_t vs_cell,
                                                      int64_t vs_x, double sigma2, const int32_t* __restrict__ r1, int nr1,
                                                      const int32_t* __restrict__ r2, int nr2, int npad,
                                                      double* __restrict__ out, double* __restrict__ scratch,
                                                      int cell_begin, int cell_end) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* grad = reinterpret_cast<double*>(smem_raw);  // [g]
    double* cur = grad + g;                              // [g]
    __shared__ double sh_l2, sh_proj, sh3[3];
    const int tid = threadIdx.x;
    const AsvLiteralLayout L(nr2, npad);
    double* base = scratch + (int64_t)blockIdx.x * L.per_cell;
    double* lw2 = base + L.lw2;
    double* add2 = base + L.add2;
    double* kp = base + L.kp;  // projections
    double* kw = base + L.kw;  // log-weights

    for (int cell = cell_begin + blockIdx.x; cell < cell_end; cell += gridDim.x) {
        for (int x = tid; x < g; x += T) {
            grad[x] = vect[(int64_t)x * vs_x + (int64_t)cell * vs_cell];
            cur[x] = data2[(int64_t)cell * g + x];
        }
        __syncthreads();
        if (tid == 0) {  // :57-70
            double l2 = 0.0;
            for (int x = 0; x < g; ++x) l2 += grad[x] * grad[x];
            sh_l2 = sqrt(l2);
        }
        __syncthreads();
        const double l2 = sh_l2;
        if (l2 != 0.0)
            for (int x = tid; x < g; x += T) grad[x] /= l2;
        __syncthreads();
        if (tid == 0) {
            double p = 0.0;
            for (int x = 0; x < g; ++x) p += grad[x] * cur[x];
            sh_proj = p;
        }
        __syncthreads();
        const double curproj = sh_proj;
        // every pair's projection and log-weight, in parallel (each value is computed exactly as the reference does:
        // asv_pair_literal, the one copy that the tiled form's re-run evaluates its kept addends with as well)
        for (int s = tid; s < nr2; s += T) {
            const int same = r2[s];
            double pr = 0.0, lw = 0.0;
            bool add = true;
            if (same != cell) {
                asv_pair_literal(cur, grad, data2 + (int64_t)same * g, g, sigma2, pr, lw);
                add = !(pr > curproj);
            }
            lw2[s] = lw;
            add2[s] = add ? 1.0 : 0.0;
        }
        for (int o = tid; o < npad; o += T) {
            double pr = __builtin_inf(), lw = __builtin_inf();
            if (o < nr1) asv_pair_literal(cur, grad, data1 + (int64_t)r1[o] * g, g, sigma2, pr, lw);
            kp[o] = pr;
            kw[o] = lw;
        }
        __syncthreads();
        asv_cell_phase(lw2, add2, kp, kw, nr1, nr2, npad, curproj, l2, out + cell, sh3);
    }
}

// ---------------------------------------------------------------------------------------------------
// adjust_shift_variance in gene space (g > 256 beyond the exact form's size; testing hook "asv_wide": any size), literally:
// the same doubles as asv_exact_kernel, cells handled in chunks of pl.chunk so that the pair values stay bounded.
//   asv_wide_prep:  one thread per cell of the chunk -- gradn [g][nc] (the correction vector over its l2 norm, :57-66),
//                   l2 and the cell's own projection (:67-70), each sum left to right as the reference has it;
//   asv_wide_pairs: LDS-tiled (32 cells x 64 streamed cells a workgroup, 32 genes staged at a time, the way knn_exact_dist
//                   tiles the kNN).  The streamed cells are the restricted cells of data1 then those of data2.  For every pair
//                   the projection and scale (first sweep over the genes) and the distance to the line (second sweep,
//                   sq_distance_to_line, :9-27), each accumulated left to right by one thread; writes the pair's values
//                   into the cell's scratch in asv_exact_kernel's layout (AsvLiteralLayout);
//   asv_wide_cells: one workgroup per cell, asv_cell_phase on those values.
// scratch: AsvLiteralLayout per cell of a chunk and its wide tail behind the chunk's cells.
// With a cell list (strict mode: the mode-2 cells of a tiled call) cell i of the chunk is list[c0 + i] instead of c0 + i; c0
// and nc then count entries of the list, and c0 + nc never passes the count the host has read.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void asv_wide_prep(const double* __restrict__ data2, int g, const double* __restrict__ vect,
                                                     int64_t vs_cell, int64_t vs_x, int c0, int nc,
                                                     const int32_t* __restrict__ list, double* __restrict__ gradn,
                                                     double* __restrict__ l2o, double* __restrict__ projo) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc) return;
    const int64_t cell = list ? (int64_t)list[c0 + i] : (int64_t)c0 + i;
    double l2 = 0.0;
    for (int x = 0; x < g; ++x) {
        const double v = vect[(int64_t)x * vs_x + cell * vs_cell];
        l2 += v * v;
    }
    l2 = sqrt(l2);
    double p = 0.0;
    for (int x = 0; x < g; ++x) {
        double v = vect[(int64_t)x * vs_x + cell * vs_cell];
        if (l2 != 0.0) v /= l2;
        gradn[(int64_t)x * nc + i] = v;
        p += v * data2[cell * g + x];
    }
    l2o[i] = l2;
    projo[i] = p;
}

__global__ __launch_bounds__(256) void asv_wide_pairs(const double* __restrict__ data1, const double* __restrict__ data2, int g,
                                                      const int32_t* __restrict__ r1, int nr1, const int32_t* __restrict__ r2,
                                                      int nr2, int npad, double sigma2, int c0, int nc, int sb0,
                                                      const int32_t* __restrict__ list, const double* __restrict__ gradn,
                                                      const double* __restrict__ projo, double* __restrict__ scratch) {
    __shared__ double sO[AW_KC][AW_S];   // streamed cells: [gene][cell]
    __shared__ double sG[AW_KC][AW_C];   // unit correction vectors of the tile's cells
    __shared__ double sX[AW_KC][AW_C];   // the tile's cells
    const int tid = threadIdx.x;
    const int j = tid & (AW_S - 1), w = tid >> 6;  // this thread's streamed cell; its cells are w + 4 q (uniform in a wave)
    const int i0 = blockIdx.x * AW_C;
    const int s0 = (sb0 + (int)blockIdx.y) * AW_S;  // (sb0: launches in slabs of at most 65 535 streamed tiles)
    const int S = nr1 + nr2;
    constexpr int Q = AW_C / 4;
    double pr[Q], sc[Q], dist[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) pr[q] = sc[q] = dist[q] = 0.0;
    auto stage = [&](int x0) {
        const int kx = min(AW_KC, g - x0);
        for (int e = tid; e < AW_S * AW_KC; e += 256) {
            const int r = e / AW_KC, x = e % AW_KC, s = s0 + r;
            double v = 0.0;
            if (x < kx && s < S) {
                const double* row = s < nr1 ? data1 + (int64_t)r1[s] * g : data2 + (int64_t)r2[s - nr1] * g;
                v = row[x0 + x];
            }
            sO[x][r] = v;
        }
        for (int e = tid; e < AW_C * AW_KC; e += 256) {
            const int x = e / AW_C, i = e % AW_C;
            sG[x][i] = (x < kx && i0 + i < nc) ? gradn[(int64_t)(x0 + x) * nc + i0 + i] : 0.0;
        }
        for (int e = tid; e < AW_C * AW_KC; e += 256) {
            const int i = e / AW_KC, x = e % AW_KC;
            double v = 0.0;
            if (x < kx && i0 + i < nc) {  // (entry c0 + i0 + i of the list lies below the count: i0 + i < nc)
                const int64_t cell = list ? (int64_t)list[c0 + i0 + i] : (int64_t)c0 + i0 + i;
                v = data2[cell * g + x0 + x];
            }
            sX[x][i] = v;
        }
        __syncthreads();
        return kx;
    };
    // sweep 1: projection of the streamed cell and the scale of the difference along the line (:12-15), left to right
    for (int x0 = 0; x0 < g; x0 += AW_KC) {
        const int kx = stage(x0);
        for (int x = 0; x < kx; ++x) {
            const double o = sO[x][j];
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const double gi = sG[x][w + 4 * q], ci = sX[x][w + 4 * q];
                pr[q] += gi * o;
                sc[q] += (ci - o) * gi;
            }
        }
        __syncthreads();
    }
    // sweep 2: the squared distance to the line (:17-24)
    for (int x0 = 0; x0 < g; x0 += AW_KC) {
        const int kx = stage(x0);
        for (int x = 0; x < kx; ++x) {
            const double o = sO[x][j];
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const double gi = sG[x][w + 4 * q], ci = sX[x][w + 4 * q];
                const double t = (ci - o) - sc[q] * gi;
                dist[q] += t * t;
            }
        }
        __syncthreads();
    }
    const int s = s0 + j;
    if (s >= S) return;
    const AsvLiteralLayout L(nr2, npad);
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int i = i0 + w + 4 * q;
        if (i >= nc) continue;
        double* base = scratch + (int64_t)i * L.per_cell;
        const double lw = -dist[q] / sigma2;
        if (s < nr1) {
            base[L.kp + s] = pr[q];
            base[L.kw + s] = lw;
        } else {
            const int s2 = s - nr1;
            const bool same = r2[s2] == (list ? list[c0 + i] : c0 + i);  // the cell itself: weight exp(0), always counted (:78-84)
            base[L.lw2 + s2] = same ? 0.0 : lw;
            base[L.add2 + s2] = (same || !(pr[q] > projo[i])) ? 1.0 : 0.0;
        }
    }
}

__global__ __launch_bounds__(T) void asv_wide_cells(int nr1, int nr2, int npad, int c0, int nc,
                                                    const int32_t* __restrict__ list, const double* __restrict__ l2o,
                                                    const double* __restrict__ projo, double* __restrict__ scratch,
                                                    double* __restrict__ out) {
    __shared__ double sh3[3];
    const AsvLiteralLayout L(nr2, npad);
    for (int i = blockIdx.x; i < nc; i += gridDim.x) {
        double* base = scratch + (int64_t)i * L.per_cell;
        double* kp = base + L.kp;
        double* kw = base + L.kw;
        for (int o = nr1 + threadIdx.x; o < npad; o += T) {  // padding: sorts last
            kp[o] = __builtin_inf();
            kw[o] = __builtin_inf();
        }
        __syncthreads();
        asv_cell_phase(base + L.lw2, base + L.add2, kp, kw, nr1, nr2, npad, projo[i], l2o[i],
                       out + (list ? list[c0 + i] : c0 + i), sh3);
    }
}

// Strict mode: the record of a tiled call's ways (modes, one byte per cell) -> the ascending list of the mode-2 cells of
// [cell_begin, cell_end) and its length in count[0]; count[1]: the cells re-run literally.  One workgroup: every thread
// takes a contiguous run of the cells, an exclusive scan over the threads' counts places the runs -- the order is the
// cells' own, whatever the timing (no atomic append).
__global__ __launch_bounds__(T) void asv_strict_compact(const unsigned char* __restrict__ modes, int cell_begin, int cell_end,
                                                        int32_t* __restrict__ list, unsigned int* __restrict__ count) {
    __shared__ int sc[T];
    __shared__ int s1[T];
    const int tid = threadIdx.x;
    const int n = cell_end - cell_begin;
    const int per = (n + T - 1) / T;
    const int b = cell_begin + min(n, tid * per), e = cell_begin + min(n, (tid + 1) * per);
    int n2 = 0, n1 = 0;
    for (int c = b; c < e; ++c) {
        const unsigned char m = modes[c];
        n2 += m == 2;
        n1 += m == 1;
    }
    sc[tid] = n2;
    const int lits = block_sum(n1, s1);  // (ends in a barrier: sc is written)
    for (int o = 1; o < T; o <<= 1) {    // inclusive scan
        const int v = tid >= o ? sc[tid - o] : 0;
        __syncthreads();
        sc[tid] += v;
        __syncthreads();
    }
    int at = sc[tid] - n2;
    for (int c = b; c < e; ++c)
        if (modes[c] == 2) list[at++] = c;
    if (tid == T - 1) {
        count[0] = (unsigned int)sc[tid];
        count[1] = (unsigned int)lits;
    }
}

}  // namespace

// the wide form over the cells [c_begin, c_end) -- or, with a list, over its entries [c_begin, c_end) -- nc_max at a time
static void launch_wide_chunks(hipStream_t stream, const double* data1, int g, const double* data2, const double* vect,
                               int64_t vs_cell, int64_t vs_x, double sigma2, const int32_t* restrict1, int nr1,
                               const int32_t* restrict2, int nr2, double* out, double* ws, int nc_max, int npad, int blocks,
                               const int32_t* list, int c_begin, int c_end) {
    const AsvLiteralLayout L(nr2, npad);
    double* gradn = ws + L.wide_gradn(nc_max);  // [g][nc]
    double* l2o = ws + L.wide_l2(g, nc_max);
    double* projo = ws + L.wide_proj(g, nc_max);
    for (int c0 = c_begin; c0 < c_end; c0 += nc_max) {
        const int nc = std::min(nc_max, c_end - c0);
        hipLaunchKernelGGL(asv_wide_prep, dim3((unsigned)cdiv(nc, 256)), dim3(256), 0, stream, data2, g, vect, vs_cell, vs_x, c0,
                           nc, list, gradn, l2o, projo);
        const int S = nr1 + nr2;
        const int sblocks = cdiv(S, AW_S);
        for (int sb0 = 0; sb0 < sblocks; sb0 += 65535)
            hipLaunchKernelGGL(asv_wide_pairs, dim3((unsigned)cdiv(nc, AW_C), (unsigned)std::min(65535, sblocks - sb0)), dim3(256),
                               0, stream, data1, data2, g, restrict1, nr1, restrict2, nr2, npad, sigma2, c0, nc, sb0, list,
                               (const double*)gradn, (const double*)projo, ws);
        hipLaunchKernelGGL(asv_wide_cells, dim3((unsigned)std::min(nc, blocks)), dim3(T), 0, stream, nr1, nr2, npad, c0, nc, list,
                           (const double*)l2o, (const double*)projo, ws, out);
        BMX_LAUNCH_CHECK();
    }
}

void launch_asv_literal(hipStream_t stream, const double* data1, int g, const double* data2, int n2, const double* vect,
                        int64_t vs_cell, int64_t vs_x, double sigma2, const int32_t* restrict1, int nr1,
                        const int32_t* restrict2, int nr2, double* out, double* ws_pairs, const AsvPlan& pl, int cell_begin,
                        int cell_end) {
    const int blocks = pl.blocks;
    if (pl.wide) {
        launch_wide_chunks(stream, data1, g, data2, vect, vs_cell, vs_x, sigma2, restrict1, nr1, restrict2, nr2, out, ws_pairs,
                           pl.chunk, pl.npad, blocks, nullptr, cell_begin, cell_end);
        return;
    }
    hipLaunchKernelGGL(asv_exact_kernel, dim3(blocks), dim3(T), (size_t)2 * g * sizeof(double), stream, data1, g, data2, n2,
                       vect, vs_cell, vs_x, sigma2, restrict1, nr1, restrict2, nr2, pl.npad, out, ws_pairs, cell_begin, cell_end);
    BMX_LAUNCH_CHECK();
}

void launch_asv_strict_compact(hipStream_t stream, const unsigned char* modes, int cell_begin, int cell_end, int32_t* list,
                               unsigned int* count) {
    hipLaunchKernelGGL(asv_strict_compact, dim3(1), dim3(T), 0, stream, modes, cell_begin, cell_end, list, count);
    BMX_LAUNCH_CHECK();
}

void launch_asv_strict_pass(hipStream_t stream, const double* data1, int g, const double* data2, const double* vect,
                            int64_t vs_cell, int64_t vs_x, double sigma2, const int32_t* restrict1, int nr1,
                            const int32_t* restrict2, int nr2, double* out, double* ws_wide, const AsvStrictPlan& sp,
                            const int32_t* list, int count) {
    if (count <= 0) return;  // (nothing flagged beyond the re-run: nothing is launched)
    launch_wide_chunks(stream, data1, g, data2, vect, vs_cell, vs_x, sigma2, restrict1, nr1, restrict2, nr2, out, ws_wide,
                       sp.chunk, sp.npad, std::min(sp.chunk, 2048), list, 0, count);  // (a cell's chains run on single lanes: eight workgroups a CU)
}

}  // namespace bmx
