// The kernels and the small host routines of the blocked subspace iteration of multiBatchPCA, shared by the dense handle
// (pca.hip) and the sparse one (pca_sparse.hip): the two FP64 matrix-core products over 64-wide tiles, the fixed-order
// reductions, the filter's recurrence, the residual, two launch sequences both handles use, and Cholesky / triangular
// inverse / Jacobi on the L x L matrices.  The iteration built on them is pca_iteration.hpp.
// Everything is in an unnamed namespace: each of the two files gets its own copy.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "bmx_ops.hpp"
#include "ordered_sums.hpp"

namespace bmx {
namespace {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2u __attribute__((ext_vector_type(2), aligned(8)));  // two doubles at any 8-byte boundary
constexpr int PL = 64;   // subspace width (MFMA tile multiple)
constexpr int KC = 32;   // K elements staged per step

// ---------------------------------------------------------------------------------------------------
// NT:  Z[r][j] = rs[r] * sum_k X[r][k] * B[j][k]  -  off[j]        X [n][K] row-major, B [64][K] row-major, Z [n][64]
// (rs = per-row factor, e.g. 1 / max(1e-8, l2) of the cosine normalisation; off = mu . B_j; either may be null)
// A operand of v_mfma_f64_16x16x4_f64: lane l holds A[row = l & 15][k = l >> 4]; B operand: B[k = l >> 4][col = l & 15];
// C/D: 4 doubles per lane, col = l & 15, row = (l >> 4) + 4 * reg.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gemm_nt64(const double* __restrict__ X, int64_t n, int K, int64_t ldx,
                                                 const double* __restrict__ B, int64_t ldb,
                                                 const double* __restrict__ rs, const double* __restrict__ off,
                                                 double* __restrict__ Z, int64_t ldz) {
    constexpr int P = KC + 2;  // pitch 34 doubles: lanes (row 0..15, k 0..1) hit 32 different 8-byte bank pairs
    __shared__ __attribute__((aligned(16))) double xs[64 * P];
    __shared__ __attribute__((aligned(16))) double bs[64 * P];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * 64;
    d4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
    // a K step of both operands is 64 rows x 256 bytes: sixteen lanes take one row piece in 16-byte loads (whole cache
    // lines per row), and the step after the one being multiplied is already on its way into registers
    const int lrow = tid >> 4, lk = (tid & 15) * 2;
    const double* xp[4];
    const double* bp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t r = r0 + lrow + 16 * i;
        xp[i] = X + (r < n ? r : n - 1) * ldx + lk;  // rows past the end: any valid row, never stored
        bp[i] = B + (int64_t)(lrow + 16 * i) * ldb + lk;
    }
    d2u px[4], pb[4];
    auto fetch = [&](const int k0) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            px[i] = *reinterpret_cast<const d2u*>(xp[i] + k0);
            pb[i] = *reinterpret_cast<const d2u*>(bp[i] + k0);
        }
    };
    auto multiply = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int kk = 0; kk < KC / 4; ++kk) {
            const double a = xs[(16 * w + (lane & 15)) * P + 4 * kk + (lane >> 4)];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const double b = bs[(16 * t + (lane & 15)) * P + 4 * kk + (lane >> 4)];
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
            }
        }
    };
    const int nfull = K / KC;
    if (nfull > 0) fetch(0);
    for (int st = 0; st < nfull; ++st) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<d2u*>(&xs[(lrow + 16 * i) * P + lk]) = px[i];
            *reinterpret_cast<d2u*>(&bs[(lrow + 16 * i) * P + lk]) = pb[i];
        }
        __syncthreads();
        if (st + 1 < nfull) fetch((st + 1) * KC);
        multiply();
        __syncthreads();
    }
    if (K % KC) {  // the ragged last step, element by element
        const int k0 = nfull * KC, lr = tid >> 2, seg = (tid & 3) * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = k0 + seg + e;
            xs[lr * P + seg + e] = (r0 + lr < n && k < K) ? X[(r0 + lr) * ldx + k] : 0.0;
            bs[lr * P + seg + e] = k < K ? B[(int64_t)lr * ldb + k] : 0.0;
        }
        __syncthreads();
        multiply();
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int j = 16 * t + (lane & 15);
        const double o = off ? off[j] : 0.0;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t r = r0 + 16 * w + (lane >> 4) + 4 * reg;
            if (r < n) Z[r * ldz + j] = (rs ? rs[r] : 1.0) * acc[t][reg] - o;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// TN:  Ypart[split][g][j] = sum_{r in split} X[r][g] * (rs[r] * Z[r][j])       X [n][G] row-major, Z [n][64]
// grid (ceil(G / 64), nsplit); the partial results are summed in a fixed order by reduce_parts.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gemm_tn64(const double* __restrict__ X, int64_t n, int G, int64_t ldx,
                                                 const double* __restrict__ Z, int64_t ldz, const double* __restrict__ rs,
                                                 int64_t rows_per_split, double* __restrict__ Ypart) {
    constexpr int P = 64 + 16;  // pitch 80 doubles: lanes (col 0..15, k 0..1) hit 32 different bank pairs
    __shared__ __attribute__((aligned(16))) double xs[KC * P];
    __shared__ __attribute__((aligned(16))) double zs[KC * P];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g0 = blockIdx.x * 64;
    const int64_t rbeg = (int64_t)blockIdx.y * rows_per_split, rend = min(n, rbeg + rows_per_split);
    d4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
    auto multiply = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int kk = 0; kk < KC / 4; ++kk) {
            const double a = xs[(4 * kk + (lane >> 4)) * P + 16 * w + (lane & 15)];  // A[row = gene][k = cell]
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const double b = zs[(4 * kk + (lane >> 4)) * P + 16 * t + (lane & 15)];  // B[k = cell][col = j]
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
            }
        }
    };
    if (g0 + 64 <= G) {
        // a step is 32 cells x 64 genes (and x 64 subspace columns): thirty-two lanes take one cell's 512 bytes in 16-byte
        // loads, the step after the one being multiplied already on its way into registers
        const int lr = tid >> 5, lg = (tid & 31) * 2;
        d2u px[4], pz[4];
        auto fetch = [&](const int64_t r0) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t r = r0 + lr + 8 * i;
                if (r < rend) {
                    const double f = rs ? rs[r] : 1.0;
                    px[i] = *reinterpret_cast<const d2u*>(X + r * ldx + g0 + lg);
                    const d2u z = *reinterpret_cast<const d2u*>(Z + r * ldz + lg);
                    pz[i] = d2u{f * z[0], f * z[1]};
                } else {
                    px[i] = d2u{0.0, 0.0};
                    pz[i] = d2u{0.0, 0.0};
                }
            }
        };
        if (rbeg < rend) fetch(rbeg);
        for (int64_t r0 = rbeg; r0 < rend; r0 += KC) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                *reinterpret_cast<d2u*>(&xs[(lr + 8 * i) * P + lg]) = px[i];
                *reinterpret_cast<d2u*>(&zs[(lr + 8 * i) * P + lg]) = pz[i];
            }
            __syncthreads();
            if (r0 + KC < rend) fetch(r0 + KC);
            multiply();
            __syncthreads();
        }
    } else {  // the ragged last gene tile, element by element
        const int lr = tid >> 3, seg = (tid & 7) * 8;  // 32 rows x 8 segments of 8 doubles
        for (int64_t r0 = rbeg; r0 < rend; r0 += KC) {
            const int64_t r = r0 + lr;
            const double f = (r < rend && rs) ? rs[r] : 1.0;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int g = g0 + seg + e;
                xs[lr * P + seg + e] = (r < rend && g < G) ? X[r * ldx + g] : 0.0;
                zs[lr * P + seg + e] = r < rend ? f * Z[r * ldz + seg + e] : 0.0;
            }
            __syncthreads();
            multiply();
            __syncthreads();
        }
    }
    double* out = Ypart + (int64_t)blockIdx.y * G * 64;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int j = 16 * t + (lane & 15);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int g = g0 + 16 * w + (lane >> 4) + 4 * reg;
            if (g < G) out[(int64_t)g * 64 + j] = acc[t][reg];
        }
    }
}

// Y[(e / w) * ldy + e % w] = beta * Y[..] + alpha * sum_p part[p][e]   (parts are dense rows of w columns)
__global__ void reduce_parts(const double* __restrict__ part, int nsplit, int64_t len, double alpha, double beta,
                             double* __restrict__ Y, int w, int64_t ldy) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= len) return;
    const double s = fold_ascending(0.0, 0, nsplit, [&](int p) { return part[(int64_t)p * len + e]; });
    const int64_t o = (e / w) * ldy + e % w;
    Y[o] = (beta == 0.0 ? 0.0 : beta * Y[o]) + alpha * s;
}

// column sums of Z [n][64] with the per-row factor: two stages, deterministic
__global__ __launch_bounds__(256) void colsum64_partial(const double* __restrict__ Z, const double* __restrict__ rs,
                                                        int64_t n, int64_t rows_per_block, double* __restrict__ part) {
    __shared__ double sm[4][64];
    const int j = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block, r1 = min(n, r0 + rows_per_block);
    double s = 0.0;
    for (int64_t r = r0 + q; r < r1; r += 4) s += (rs ? rs[r] : 1.0) * Z[r * 64 + j];
    sm[q][j] = s;
    __syncthreads();
    if (q == 0) part[(int64_t)blockIdx.x * 64 + j] = (sm[0][j] + sm[1][j]) + (sm[2][j] + sm[3][j]);
}

// gene sums over the cells of a chunk: part[chunk][g] = sum_c rs[c] X[c][g]
__global__ __launch_bounds__(256) void genesum_partial(const double* __restrict__ X, const double* __restrict__ rs, int64_t n,
                                                       int G, int64_t rows_per_chunk, double* __restrict__ part) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_chunk, r1 = min(n, r0 + rows_per_chunk);
    double s = 0.0;
    for (int64_t r = r0; r < r1; ++r) s += (rs ? rs[r] : 1.0) * X[r * G + g];
    part[(int64_t)blockIdx.y * G + g] = s;
}

__global__ void axpy_kernel(double* __restrict__ y, const double* __restrict__ x, double a, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] += a * x[i];
}

// Y[g][j] -= coef * mu[g] * zsum[j]
__global__ void rank1_sub(double* __restrict__ Y, int64_t ldy, const double* __restrict__ mu, const double* __restrict__ zsum,
                          double coef, int G) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)G * 64) return;
    Y[(e >> 6) * ldy + (e & 63)] -= coef * mu[e >> 6] * zsum[e & 63];
}

__global__ void transpose64(const double* __restrict__ in, int64_t ld, int64_t rows, double* __restrict__ out) {
    // 64 columns of in [rows][ld] -> out [64][rows]
    __shared__ double tile[64][65];
    const int64_t r0 = (int64_t)blockIdx.x * 64;
    for (int e = threadIdx.x; e < 64 * 64; e += 256) {
        const int rr = e >> 6, j = e & 63;
        tile[rr][j] = r0 + rr < rows ? in[(r0 + rr) * ld + j] : 0.0;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 64 * 64; e += 256) {
        const int j = e >> 6, rr = e & 63;
        if (r0 + rr < rows) out[(int64_t)j * rows + r0 + rr] = tile[rr][j];
    }
}

// out = a X + b Y + c Z, element by element (Z may be null); the three-term recurrence of the polynomial filter
__global__ void lincomb3(double* __restrict__ out, double a, const double* __restrict__ X, double b,
                         const double* __restrict__ Y, double c, const double* __restrict__ Z, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double v = a * X[i] + b * Y[i];
    if (Z) v += c * Z[i];
    out[i] = v;
}

// part[block][j] = sum over the block's rows g of (Yr[g][j] - theta[j] Xr[g][j])^2: the squared residual norms of the
// Ritz pairs (Xr, theta) of the operator whose image of Xr is Yr.  256 rows per block, deterministic.
__global__ __launch_bounds__(256) void resid_partial(const double* __restrict__ Yr, const double* __restrict__ Xr,
                                                     const double* __restrict__ theta, int64_t G, int L,
                                                     double* __restrict__ part) {
    __shared__ double sm[4][128];
    const int j0 = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * 256, r1 = min(G, r0 + 256);
    for (int jb = 0; jb < L; jb += 64) {
        const int j = jb + j0;
        const double th = theta[j];
        double s = 0.0;
        for (int64_t r = r0 + q; r < r1; r += 4) {
            const double t = Yr[r * L + j] - th * Xr[r * L + j];
            s += t * t;
        }
        sm[q][j] = s;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < L; j += 256) part[(int64_t)blockIdx.x * L + j] = (sm[0][j] + sm[1][j]) + (sm[2][j] + sm[3][j]);
}

// ---------------------------------------------------------------------------------------------------
// The streaming pass over the genes outside subset.row (PcaGenes below): one read of a block X [n][G] of leftover rows
// (cells x leftover genes, row-major = genes x cells column-major) gives both
//     Apart[h][split][g][j] = sum_{r in split} X[r][g] * (rs[r] * Z_h[r][j])     h < NH halves of 64 subspace columns
//     Spart[split][g]       = sum_{r in split} rs[r] * X[r][g]                   (the gene sums, for the centres)
// gemm_tn64's tiling, operand layout and LDS pitch with NH Z tiles a step; the gene sums are kept by the lanes that
// fetch X (each owns fixed genes and a fixed stride of cells) and reduced in a fixed order at the end.  Z_h [n][64] is at
// Z + h * zhalf.  grid (ceil(G / 64), nsplit); no atomics: the parts are summed by reduce_parts.
// ---------------------------------------------------------------------------------------------------
template <int NH>
__global__ __launch_bounds__(256) void gemm_tn64_sums(const double* __restrict__ X, int64_t n, int G,
                                                      const double* __restrict__ Z, int64_t zhalf,
                                                      const double* __restrict__ rs, int64_t rows_per_split,
                                                      double* __restrict__ Apart, double* __restrict__ Spart) {
    constexpr int P = 64 + 16;  // as gemm_tn64
    __shared__ __attribute__((aligned(16))) double xs[KC * P];
    __shared__ __attribute__((aligned(16))) double zs[NH][KC * P];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int g0 = blockIdx.x * 64;
    const int64_t rbeg = (int64_t)blockIdx.y * rows_per_split, rend = min(n, rbeg + rows_per_split);
    d4 acc[NH][4];
#pragma unroll
    for (int h = 0; h < NH; ++h)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[h][t] = d4{0.0, 0.0, 0.0, 0.0};
    auto multiply = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int kk = 0; kk < KC / 4; ++kk) {
            const double a = xs[(4 * kk + (lane >> 4)) * P + 16 * w + (lane & 15)];  // A[row = gene][k = cell]
#pragma unroll
            for (int h = 0; h < NH; ++h)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const double b = zs[h][(4 * kk + (lane >> 4)) * P + 16 * t + (lane & 15)];  // B[k = cell][col = j]
                    acc[h][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[h][t], 0, 0, 0);
                }
        }
    };
    int sum_rows;  // how many lanes hold a partial sum of each gene
    if (g0 + 64 <= G) {
        const int lr = tid >> 5, lg = (tid & 31) * 2;
        d2u px[4], pz[NH][4];
        d2u gs = d2u{0.0, 0.0};
        auto fetch = [&](const int64_t r0) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t r = r0 + lr + 8 * i;
                if (r < rend) {
                    const double f = rs ? rs[r] : 1.0;
                    px[i] = *reinterpret_cast<const d2u*>(X + r * G + g0 + lg);
                    gs[0] += f * px[i][0];
                    gs[1] += f * px[i][1];
#pragma unroll
                    for (int h = 0; h < NH; ++h) {
                        const d2u z = *reinterpret_cast<const d2u*>(Z + h * zhalf + r * 64 + lg);
                        pz[h][i] = d2u{f * z[0], f * z[1]};
                    }
                } else {
                    px[i] = d2u{0.0, 0.0};
#pragma unroll
                    for (int h = 0; h < NH; ++h) pz[h][i] = d2u{0.0, 0.0};
                }
            }
        };
        if (rbeg < rend) fetch(rbeg);
        for (int64_t r0 = rbeg; r0 < rend; r0 += KC) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                *reinterpret_cast<d2u*>(&xs[(lr + 8 * i) * P + lg]) = px[i];
#pragma unroll
                for (int h = 0; h < NH; ++h) *reinterpret_cast<d2u*>(&zs[h][(lr + 8 * i) * P + lg]) = pz[h][i];
            }
            __syncthreads();
            if (r0 + KC < rend) fetch(r0 + KC);
            multiply();
            __syncthreads();
        }
        *reinterpret_cast<d2u*>(&xs[lr * P + lg]) = gs;
        sum_rows = 8;
    } else {  // the ragged last gene tile, element by element
        const int lr = tid >> 3, seg = (tid & 7) * 8;  // 32 rows x 8 segments of 8 doubles
        double gs[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) gs[e] = 0.0;
        for (int64_t r0 = rbeg; r0 < rend; r0 += KC) {
            const int64_t r = r0 + lr;
            const double f = (r < rend && rs) ? rs[r] : 1.0;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int g = g0 + seg + e;
                const double x = (r < rend && g < G) ? X[r * G + g] : 0.0;
                xs[lr * P + seg + e] = x;
                gs[e] += f * x;
#pragma unroll
                for (int h = 0; h < NH; ++h) zs[h][lr * P + seg + e] = r < rend ? f * Z[h * zhalf + r * 64 + seg + e] : 0.0;
            }
            __syncthreads();
            multiply();
            __syncthreads();
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) xs[lr * P + seg + e] = gs[e];
        sum_rows = 32;
    }
    __syncthreads();
    if (tid < 64 && g0 + tid < G) {
        double s = 0.0;
        for (int i = 0; i < sum_rows; ++i) s += xs[i * P + tid];
        Spart[(int64_t)blockIdx.y * G + g0 + tid] = s;
    }
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        double* out = Apart + ((int64_t)h * gridDim.y + blockIdx.y) * G * 64;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int j = 16 * t + (lane & 15);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int g = g0 + 16 * w + (lane >> 4) + 4 * reg;
                if (g < G) out[(int64_t)g * 64 + j] = acc[h][t][reg];
            }
        }
    }
}

// rotation rows of the leftover genes, column-major [d][G]:  out[j][g] = (A_h[g][j % 64] - mu[g] * t[j]) / s2[j],  h = j / 64
__global__ void genes_rotation(const double* __restrict__ A, const double* __restrict__ mu, const double* __restrict__ t,
                               const double* __restrict__ s2, int G, int d, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)G * d) return;
    const int j = (int)(e / G), g = (int)(e % G);
    out[e] = (A[((int64_t)(j >> 6) * G + g) * 64 + (j & 63)] - mu[g] * t[j]) / s2[j];
}

// part[block] = sum over the block's cells c and all genes g of (rs[c] X[c][g] - mu[g])^2: one wave a cell, four cells in
// flight a workgroup, deterministic
__global__ __launch_bounds__(256) void centred_sq_partial(const double* __restrict__ X, const double* __restrict__ rs,
                                                          const double* __restrict__ mu, int64_t n, int G,
                                                          int64_t cells_per_block, double* __restrict__ part) {
    __shared__ double sm[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t c0 = (int64_t)blockIdx.x * cells_per_block, c1 = min(n, c0 + cells_per_block);
    double s = 0.0;
    for (int64_t c = c0 + w; c < c1; c += 4) {
        const double f = rs ? rs[c] : 1.0;
        const double* col = X + c * G;
        for (int g = lane; g < G; g += 64) {
            const double v = f * col[g] - mu[g];
            s += v * v;
        }
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) sm[w] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

// ---- two launch sequences the handles share ------------------------------------------------------------------------
// out[j] = beta out[j] + alpha * sum_c Z[c][j] for Z [n][64], two stages in a fixed order; zpart holds colsum_blocks(n)
// rows of 64
inline int colsum_blocks(int64_t n) { return (int)std::min<int64_t>(4096, std::max<int64_t>(1, n / 256)); }
inline void column_sums64(hipStream_t stream, const double* Z, int64_t n, double* zpart, double alpha, double beta,
                          double* out) {
    const int nb = colsum_blocks(n);
    const int64_t rpb = (n + nb - 1) / nb;
    hipLaunchKernelGGL(colsum64_partial, dim3(nb), dim3(256), 0, stream, Z, (const double*)nullptr, n, rpb, zpart);
    hipLaunchKernelGGL(reduce_parts, dim3(1), dim3(64), 0, stream, (const double*)zpart, nb, (int64_t)PL, alpha, beta, out,
                       PL, (int64_t)PL);
    BMX_LAUNCH_CHECK();
}
// The last step of the pass over G leftover genes: their rotation rows into rot [d][G] (genes_rotation) from their sums
// acc, centres mu and the projections' column sums tsum, divided by s2[j] = sdev_j^2 with sdev as fit reports it (ds2: d
// doubles on the device); then mu and rot go to the host (either pointer may be null) and the stream is drained
inline void leftover_rotation(hipStream_t stream, const std::vector<double>& theta, int d, const double* acc,
                              const double* mu, const double* tsum, double* ds2, int G, double* rot,
                              double* centers_left, double* rotation_left) {
    std::vector<double> s2((size_t)d);
    for (int j = 0; j < d; ++j) {
        const double sd = std::sqrt(std::max(0.0, theta[(size_t)j]));
        s2[(size_t)j] = sd * sd;
    }
    BMX_HIP(hipMemcpyAsync(ds2, s2.data(), (size_t)d * sizeof(double), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(genes_rotation, dim3((unsigned)cdiv((int64_t)G * d, 256)), dim3(256), 0, stream, acc, mu, tsum,
                       (const double*)ds2, G, d, rot);
    BMX_LAUNCH_CHECK();
    if (centers_left) BMX_HIP(hipMemcpyAsync(centers_left, mu, (size_t)G * sizeof(double), hipMemcpyDeviceToHost, stream));
    if (rotation_left)
        BMX_HIP(hipMemcpyAsync(rotation_left, rot, (size_t)G * d * sizeof(double), hipMemcpyDeviceToHost, stream));
    BMX_HIP(hipStreamSynchronize(stream));
}

// ---- small dense helpers on the host (L x L, L = 64 or 128) --------------------------------------------------------
// upper-triangular R with R^T R = S (S symmetric positive definite, row-major); returns false if not
bool cholesky_upper(std::vector<double>& S, int n) {
    for (int i = 0; i < n; ++i) {
        for (int j = i; j < n; ++j) {
            double s = S[(size_t)i * n + j];
            for (int k = 0; k < i; ++k) s -= S[(size_t)k * n + i] * S[(size_t)k * n + j];
            if (i == j) {
                if (!(s > 0.0)) return false;
                S[(size_t)i * n + i] = std::sqrt(s);
            } else {
                S[(size_t)i * n + j] = s / S[(size_t)i * n + i];
            }
        }
        for (int j = 0; j < i; ++j) S[(size_t)i * n + j] = 0.0;
    }
    return true;
}
// inverse of an upper-triangular matrix (row-major), in place
void invert_upper(std::vector<double>& R, int n) {
    std::vector<double> inv((size_t)n * n, 0.0);
    for (int j = 0; j < n; ++j) {
        inv[(size_t)j * n + j] = 1.0 / R[(size_t)j * n + j];
        for (int i = j - 1; i >= 0; --i) {
            double s = 0.0;
            for (int k = i + 1; k <= j; ++k) s += R[(size_t)i * n + k] * inv[(size_t)k * n + j];
            inv[(size_t)i * n + j] = -s / R[(size_t)i * n + i];
        }
    }
    R = inv;
}
// cyclic Jacobi eigen-decomposition of a symmetric matrix: A -> eigenvalues on the diagonal, V columns = eigenvectors
void jacobi_eigen(std::vector<double>& A, std::vector<double>& V, int n) {
    V.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) V[(size_t)i * n + i] = 1.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double offd = 0.0, diag = 0.0;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) (i == j ? diag : offd) += A[(size_t)i * n + j] * A[(size_t)i * n + j];
        if (offd <= 1e-30 * diag) break;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[(size_t)p * n + q];
                if (apq == 0.0) continue;
                const double theta = (A[(size_t)q * n + q] - A[(size_t)p * n + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; ++k) {
                    const double akp = A[(size_t)k * n + p], akq = A[(size_t)k * n + q];
                    A[(size_t)k * n + p] = c * akp - s * akq;
                    A[(size_t)k * n + q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {
                    const double apk = A[(size_t)p * n + k], aqk = A[(size_t)q * n + k];
                    A[(size_t)p * n + k] = c * apk - s * aqk;
                    A[(size_t)q * n + k] = s * apk + c * aqk;
                }
                for (int k = 0; k < n; ++k) {
                    const double vkp = V[(size_t)k * n + p], vkq = V[(size_t)k * n + q];
                    V[(size_t)k * n + p] = c * vkp - s * vkq;
                    V[(size_t)k * n + q] = s * vkp + c * vkq;
                }
            }
    }
}

}  // namespace
}  // namespace bmx
