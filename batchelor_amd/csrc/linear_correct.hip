// rescaleBatches() (R/rescaleBatches.R:103-150) and regressBatches() (R/regressBatches.R:93-158) on the device: per-gene
// passes over genes x cells FP64 matrices in R's layout, uploaded once (whole or in column blocks) and kept in HBM.
//   pass 1  per-gene sums over a batch's restricted cells.  The restricted cells, ascending, are cut into chunks of LCH at
//           fixed positions of that list; sum_partial_kernel adds a chunk's cells in list order (one workgroup per chunk
//           and tile of 256 genes, lanes along the genes), mean_kernel adds the chunk sums in ascending order: the rules
//           of ordered_sums.hpp (sum_partial_kernel keeps its own copy of the walk: the helper cost its pow forms 3 %).
//           A chunk is summed by the first add_block call after which all its cells are resident, on a second stream
//           behind the upload of the next block.
//             rescaleBatches          sums of log.base^x - pseudo.count (.unlog, :140-143)
//             regressBatches, default sums of x: the coefficient of a batch's indicator column is its mean
//             regressBatches, design  coef = X[:, R] %*% W (W = pinv(D[R, ])^T from the host's QR), chunks of GCH cells,
//                                     sixteen columns of W per workgroup; coef_reduce_kernel adds the chunks of all
//                                     batches in ascending order
//   stats   rescale_stats_kernel: ref = pmin over batches, rescale = ref / avg, 0 where not finite (:128-131)
//   pass 2  every cell, in blocks of about OUT_BLOCK_BYTES through two device buffers: the kernel of block i + 1 runs
//           while block i goes to the host through the download ring.
//             rescale_kernel  log((log.base^x - pseudo) * rescale + pseudo, log.base) (.relog)
//             subtract_kernel x - mean of the cell's batch
//             residual_kernel x - coef[, drop] %*% t(D[, drop]), the dropped columns added in ascending order
//   PCA     regressBatches(d=, deferred=TRUE): multiBatchPCA of the residuals over the first n_pca_rows rows, from the resident
//           batches.  The residual of batch b is x_b minus a term of rank <= 65, so the operator of pca.hip is applied to x_b
//           and the low-rank term is taken off the two skinny results (ResidualPca below); no residual is written.
// All FP64 vector arithmetic, contraction off.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "bmx_ops.hpp"
#include "host_xfer.hpp"
#include "ordered_sums.hpp"
#include "pca_iteration.hpp"
#include "resident_batches.hpp"

namespace bmx {
namespace {

constexpr int LCH = 256;    // cells per chunk of the per-gene sums
constexpr int GCH = 1024;   // cells per chunk of the product with W
constexpr int PT = 16;      // columns of W / of the design per register tile
constexpr int CPW = 16;     // cells per workgroup in the second pass
constexpr size_t OUT_BLOCK_BYTES = (size_t)64 << 20;

// MODE 0: x itself; 1: log.base 2 (exp2 / log2); 2: log.base 10 (pow / log10); 3: any other base (pow, log(v) / log(base):
// what R's log(x, base) does)
template <int MODE>
__device__ __forceinline__ double unlog(double x, double base, double pseudo) {
    if (MODE == 0) return x;
    if (MODE == 1) return exp2(x) - pseudo;
    return pow(base, x) - pseudo;
}
template <int MODE>
__device__ __forceinline__ double relog(double v, double log_of_base) {
    if (MODE == 1) return log2(v);
    if (MODE == 2) return log10(v);
    return log(v) / log_of_base;
}

// part[ch][g] = sum over the cells at positions [ch * LCH, min(m, (ch + 1) * LCH)) of the restricted list (order null:
// the cells themselves), in list order, of unlog(x[g, cell]); KEEP: the unlogged values go to u as well
template <int MODE, bool KEEP>
__global__ __launch_bounds__(256) void sum_partial_kernel(const double* __restrict__ x, int G,
                                                          const int32_t* __restrict__ order, int64_t m, int ch0,
                                                          double base, double pseudo, double* __restrict__ part,
                                                          double* __restrict__ u) {
    const int g = blockIdx.y * 256 + threadIdx.x;
    if (g >= G) return;
    const int ch = ch0 + blockIdx.x;
    const int64_t b = (int64_t)ch * LCH;
    const int64_t e = b + LCH < m ? b + LCH : m;
    double s = 0.0;
    int64_t i = b;
    // (its own loop, not ordered_walk4: on the helper the pow forms came out 3 % slower, MEASUREMENTS.md)
    for (; i + 4 <= e; i += 4) {  // four loads in flight, added in list order
        const int64_t c0 = order ? order[i] : i, c1 = order ? order[i + 1] : i + 1;
        const int64_t c2 = order ? order[i + 2] : i + 2, c3 = order ? order[i + 3] : i + 3;
        const double x0 = x[c0 * G + g], x1 = x[c1 * G + g], x2 = x[c2 * G + g], x3 = x[c3 * G + g];
        const double v0 = unlog<MODE>(x0, base, pseudo), v1 = unlog<MODE>(x1, base, pseudo);
        const double v2 = unlog<MODE>(x2, base, pseudo), v3 = unlog<MODE>(x3, base, pseudo);
        if (KEEP) {
            u[c0 * G + g] = v0;
            u[c1 * G + g] = v1;
            u[c2 * G + g] = v2;
            u[c3 * G + g] = v3;
        }
        s += v0;
        s += v1;
        s += v2;
        s += v3;
    }
    for (; i < e; ++i) {
        const int64_t c = order ? order[i] : i;
        const double v = unlog<MODE>(x[c * G + g], base, pseudo);
        if (KEEP) u[c * G + g] = v;
        s += v;
    }
    part[(int64_t)ch * G + g] = s;
}

// mean[g] = (sum of the chunk sums, ascending chunk) / m
__global__ __launch_bounds__(256) void mean_kernel(const double* __restrict__ part, int G, int nchunks, double m,
                                                   double* __restrict__ mean) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    const auto at = [&](int ch) { return part[(int64_t)ch * G + g]; };
    mean[g] = fold_ascending(at(0), 1, nchunks, at) / m;
}

// avg [B][G] -> ref [G] = pmin over the batches (NaN if any is), scale [B][G] = ref / avg, 0 where that is not finite
__global__ __launch_bounds__(256) void rescale_stats_kernel(const double* __restrict__ avg, int G, int B,
                                                            double* __restrict__ ref, double* __restrict__ scale) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    double r = avg[g];
    for (int b = 1; b < B; ++b) {
        const double a = avg[(int64_t)b * G + g];
        if (a != a || r != r)
            r = __longlong_as_double(0x7ff8000000000000ll);
        else if (a < r)
            r = a;
    }
    ref[g] = r;
    for (int b = 0; b < B; ++b) {
        const double s = r / avg[(int64_t)b * G + g];
        scale[(int64_t)b * G + g] = isfinite(s) ? s : 0.0;
    }
}

// out[g, c] = relog(unlog(x[g, c]) * scale[g] + pseudo), cells [0, mb) of the block at x / out; FROMU: x holds the
// unlogged values already
template <int MODE, bool FROMU>
__global__ __launch_bounds__(256) void rescale_kernel(const double* __restrict__ x, int G, int mb,
                                                      const double* __restrict__ scale, double base, double pseudo,
                                                      double log_of_base, double* __restrict__ out) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    const double sc = scale[g];
    const int c0 = blockIdx.y * CPW, c1 = min(mb, c0 + CPW);
    for (int c = c0; c < c1; ++c) {
        const int64_t at = (int64_t)c * G + g;
        const double v = FROMU ? x[at] : unlog<MODE>(x[at], base, pseudo);
        out[at] = relog<MODE>(v * sc + pseudo, log_of_base);
    }
}

__global__ __launch_bounds__(256) void subtract_kernel(const double* __restrict__ x, int G, int mb,
                                                       const double* __restrict__ mean, double* __restrict__ out) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    const double mu = mean[g];
    const int c0 = blockIdx.y * CPW, c1 = min(mb, c0 + CPW);
    for (int c = c0; c < c1; ++c) {
        const int64_t at = (int64_t)c * G + g;
        out[at] = x[at] - mu;
    }
}

// part[ch][j][g] = sum over the cells at positions [ch * GCH, ...) of the batch's restricted list, in list order, of
// x[g, cell] * w[row0 + position][j], j in this workgroup's tile of PT columns (w [rows][p16] row-major, zero padded:
// a cell's weights are one uniform load)
__global__ __launch_bounds__(256) void coef_partial_kernel(const double* __restrict__ x, int G,
                                                           const int32_t* __restrict__ order, int64_t m,
                                                           const double* __restrict__ w, int64_t row0, int p16,
                                                           double* __restrict__ part) {
    const int g = blockIdx.y * 256 + threadIdx.x;
    if (g >= G) return;
    const int ch = blockIdx.x, t0 = blockIdx.z * PT;
    const int64_t b = (int64_t)ch * GCH;
    const int64_t e = b + GCH < m ? b + GCH : m;
    double acc[PT];
#pragma unroll
    for (int j = 0; j < PT; ++j) acc[j] = 0.0;
    for (int64_t i = b; i < e; ++i) {
        const int64_t c = order ? order[i] : i;
        const double xv = x[c * G + g];
        const double* wr = w + (row0 + i) * p16 + t0;
#pragma unroll
        for (int j = 0; j < PT; ++j) acc[j] += xv * wr[j];
    }
#pragma unroll
    for (int j = 0; j < PT; ++j) part[((int64_t)ch * p16 + t0 + j) * G + g] = acc[j];
}

// coef[j][g] = sum over all chunks of all batches, ascending, of part[ch][j][g]
__global__ __launch_bounds__(256) void coef_reduce_kernel(const double* __restrict__ part, int G, int p16, int nchunks,
                                                          double* __restrict__ coef) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int j = blockIdx.y;
    if (g >= G) return;
    const auto at = [&](int ch) { return part[((int64_t)ch * p16 + j) * G + g]; };
    coef[(int64_t)j * G + g] = fold_ascending(at(0), 1, nchunks, at);
}

// out[g, c] = x[g, c] - sum_j coef[g, drop[j]] * dd[c][j]: the dropped columns in tiles of PT, ascending; dd [mb][pd16]
// row-major, zero padded, drop [pd16] (-1: padding)
__global__ __launch_bounds__(256) void residual_kernel(const double* __restrict__ x, int G, int mb,
                                                       const double* __restrict__ coef, const int32_t* __restrict__ drop,
                                                       const double* __restrict__ dd, int pd16, double* __restrict__ out) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    const int c0 = blockIdx.y * CPW, c1 = min(mb, c0 + CPW);
    if (pd16 == 0) {
        for (int c = c0; c < c1; ++c) out[(int64_t)c * G + g] = x[(int64_t)c * G + g];
        return;
    }
    for (int t0 = 0; t0 < pd16; t0 += PT) {
        double cf[PT];
#pragma unroll
        for (int j = 0; j < PT; ++j) {
            const int col = drop[t0 + j];
            cf[j] = col >= 0 ? coef[(int64_t)col * G + g] : 0.0;
        }
        for (int c = c0; c < c1; ++c) {
            const int64_t at = (int64_t)c * G + g;
            const double* dr = dd + (int64_t)c * pd16 + t0;
            double acc = 0.0;
#pragma unroll
            for (int j = 0; j < PT; ++j) acc += cf[j] * dr[j];
            out[at] = (t0 == 0 ? x[at] : out[at]) - acc;
        }
    }
}

// ---- the deferred PCA of the residuals (ResidualPca)
constexpr int RPW = 16;  // rows per wave of lowrank_sub_kernel

// Y[r][j] -= alpha * sum_k A[r][k] * M[k][j], j < 64, k ascending.  A [rows][pk] row-major and M [pk][64], pk a multiple of
// PT, both zero padded.  A lane owns a column j and keeps a tile of PT rows of M in registers (as residual_kernel keeps
// the coefficients); a wave takes RPW rows: a row's piece of A is one wave-uniform 128-byte load, its 64 columns of Y one
// 512-byte row.  Both skinny corrections of the operator are this kernel: Z -= E_b T along the cells (A = E_b, M = T) and
// Y -= coef F S_b along the genes (A = F, M = S_b).  No LDS, no atomics.
__global__ __launch_bounds__(256) void lowrank_sub_kernel(double* __restrict__ Y, int64_t ldy, int64_t rows,
                                                          const double* __restrict__ A, const double* __restrict__ M,
                                                          int pk, double alpha) {
    const int j = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t r0 = ((int64_t)blockIdx.x * 4 + w) * RPW;
    if (r0 >= rows) return;
    const int nr = (int)min((int64_t)RPW, rows - r0);
    double acc[RPW];
#pragma unroll
    for (int i = 0; i < RPW; ++i) acc[i] = 0.0;
    for (int t0 = 0; t0 < pk; t0 += PT) {
        double m[PT];
#pragma unroll
        for (int k = 0; k < PT; ++k) m[k] = M[(int64_t)(t0 + k) * 64 + j];
#pragma unroll
        for (int i = 0; i < RPW; ++i) {
            if (i < nr) {
                const double* a = A + (r0 + i) * pk + t0;
#pragma unroll
                for (int k = 0; k < PT; ++k) acc[i] += a[k] * m[k];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < RPW; ++i)
        if (i < nr) Y[(r0 + i) * ldy + j] -= alpha * acc[i];
}

// mu[g] += f * (mean[g] - sum_k coef[drop[k]][g] * dbar[k]), k ascending, g < n: a batch's share of the grand centre, the
// mean of its residuals over all its cells (coef [.][ldc], dbar the batch's mean design row over the dropped columns)
__global__ __launch_bounds__(256) void residual_centre_kernel(double* __restrict__ mu, const double* __restrict__ mean,
                                                              const double* __restrict__ coef, int64_t ldc,
                                                              const int32_t* __restrict__ drop,
                                                              const double* __restrict__ dbar, int pd, double f, int n) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    double fitted = 0.0;
    for (int k = 0; k < pd; ++k) fitted += coef[(int64_t)drop[k] * ldc + g] * dbar[k];
    mu[g] += f * (mean[g] - fitted);
}

// F = [coef[, drop] | mu] over the first n rows, both ways round: Ft [pd + 1][n] (its rows are the "cells" of the NT
// product that forms F^T Q) and Fg [n][pe16] zero padded (the A operand of lowrank_sub_kernel)
__global__ __launch_bounds__(256) void pack_f_kernel(const double* __restrict__ coef, int64_t ldc,
                                                     const int32_t* __restrict__ drop, int pd,
                                                     const double* __restrict__ mu, int n, int pe16,
                                                     double* __restrict__ Ft, double* __restrict__ Fg) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)n * pe16) return;
    const int g = (int)(e / pe16), k = (int)(e % pe16);
    const double v = k < pd ? coef[(int64_t)drop[k] * ldc + g] : (k == pd ? mu[g] : 0.0);
    Fg[e] = v;
    if (k <= pd) Ft[(int64_t)k * n + g] = v;
}

int mode_of(double log_base) { return log_base == 2.0 ? 1 : (log_base == 10.0 ? 2 : 3); }

constexpr int LINEAR_MAX_P = 64;  // columns a design may have

}  // namespace

// argument checks of Linear::begin_batch / rescale / regress without a device (throw Error(BMX_ERR_ARG))
void linear_check_batch(int64_t n, const int32_t* restrict_idx, int64_t n_restrict) {
    check_cell_count(n);
    check_restriction(n, restrict_idx, n_restrict);
}

void linear_check_rescale(double log_base, double pseudo_count) {
    if (!(log_base > 0.0) || !std::isfinite(log_base) || log_base == 1.0)
        throw Error(BMX_ERR_ARG, "'log_base' must be positive, finite and not 1");
    if (!std::isfinite(pseudo_count)) throw Error(BMX_ERR_ARG, "'pseudo_count' must be finite");
}

void linear_check_regress(const double* design, int p, const double* w, const int32_t* keep, int n_keep) {
    if (!design) {
        if (w || n_keep > 0) throw Error(BMX_ERR_ARG, "'w' and 'keep' need a design");
        return;
    }
    if (p < 1 || p > LINEAR_MAX_P) throw Error(BMX_ERR_ARG, "a design has between 1 and 64 columns");
    if (!w) throw Error(BMX_ERR_ARG, "a design needs 'w', the transposed pseudo-inverse of its restricted rows");
    if (n_keep < 0 || (n_keep > 0 && !keep)) throw Error(BMX_ERR_ARG, "invalid 'keep'");
    for (int i = 0; i < n_keep; ++i)
        if (keep[i] < 1 || keep[i] > p) throw Error(BMX_ERR_ARG, "'keep' indices out of range");
}

void linear_check_pca(int G, int n_pca_rows, int d, double tol, int max_applies, const double* weights, int n_batches) {
    if (G < 1) throw Error(BMX_ERR_ARG, "the linear corrections need at least one gene");
    if (n_pca_rows < 1 || n_pca_rows > G) throw Error(BMX_ERR_ARG, "'n_pca_rows' is between 1 and the number of genes");
    if (d < 1 || d > 2 * PL - 8) throw Error(BMX_ERR_ARG, "the device PCA takes 1 <= d <= 120");
    if (d > n_pca_rows) throw Error(BMX_ERR_ARG, "d exceeds the number of genes");
    if (tol != tol || std::isinf(tol)) throw Error(BMX_ERR_ARG, "the PCA tolerance must be finite");
    if (max_applies < 1) throw Error(BMX_ERR_ARG, "the PCA needs at least one iteration");
    if (n_batches < 0) throw Error(BMX_ERR_ARG, "the number of batches is negative");
    for (int b = 0; weights && b < n_batches; ++b)
        if (!(weights[b] > 0.0) || !std::isfinite(weights[b]))
            throw Error(BMX_ERR_ARG, "the PCA weights must be positive and finite");
}

struct LinearBatch : ResidentBatch, ChunkProgress {
    DevBuf<double> u;        // [n][G] unlogged values, when they are kept
    DevBuf<double> part;     // [nchunks][G]
    DevBuf<int32_t> order;   // restricted cells (0-based) ascending, empty without restriction
    std::vector<int32_t> order_host;
    int64_t m = 0;  // restricted cells
    int sum_kind = 0;  // what part / the mean slot hold: 0 nothing, 1 plain, 2 unlogged
    double sum_base = 0.0, sum_pseudo = 0.0;
    bool has_u = false;
};

// The batches stay resident between the pass that needs every cell (the per-gene statistics) and the pass that writes the
// result.
class Linear : ResidentBatches<LinearBatch> {
    friend class ResidualPca;  // borrows the resident batches and the coefficient fit

  public:
    Linear(int device, int G) : ResidentBatches(device, G, "bmx_linear_begin_batch") {
        BMX_HIP(hipStreamCreateWithFlags(&kstream_, hipStreamNonBlocking));
        BMX_HIP(hipEventCreateWithFlags(&landed_, hipEventDisableTiming));
    }
    ~Linear() {
        retire({kstream_});
        if (landed_) (void)hipEventDestroy(landed_);
    }

    // What the caller is going to ask for, said before the upload so that the per-gene sums of a column block run behind
    // the upload of the next one: kind 0 nothing, 1 plain sums (regressBatches, default design), 2 sums of log_base^x -
    // pseudo (rescaleBatches).  keep_unlogged != 0 (kind 2): the unlogged values are kept in HBM for the second pass.
    void expect(int kind, double log_base, double pseudo, int keep_unlogged) {
        if (kind < 0 || kind > 2) throw Error(BMX_ERR_ARG, "'kind' is 0, 1 or 2");
        if (kind == 2) linear_check_rescale(log_base, pseudo);
        if (!batches_.empty()) throw Error(BMX_ERR_ARG, "bmx_linear_expect comes before the first batch");
        expect_kind_ = kind;
        expect_base_ = log_base;
        expect_pseudo_ = pseudo;
        keep_u_ = kind == 2 && keep_unlogged != 0;
    }

    // a batch of n cells, restrict_idx 1-based cells (null / nr < 0: all); its columns follow in blocks, in order
    void begin_batch(int64_t n, const int32_t* restrict_idx, int64_t nr) {
        linear_check_batch(n, restrict_idx, nr);
        ++generation_;
        begin(n, [&](LinearBatch& b) {
            const bool restricted = is_restricted(restrict_idx, nr);
            if (restricted) {  // (a cell named twice counts twice, as R's subsetting would)
                b.order_host.assign(restrict_idx, restrict_idx + nr);
                for (int32_t& v : b.order_host) v -= 1;
                std::sort(b.order_host.begin(), b.order_host.end());
            }
            b.m = restricted ? nr : n;
            b.nchunks = cdiv(b.m, LCH);
            b.part.reserve((size_t)b.nchunks * G_);
            if (keep_u_ && !restricted) {
                b.u.reserve((size_t)n * G_);
                b.has_u = true;
            }
            if (restricted) {
                BMX_HIP(hipMemcpyAsync(b.order.reserve(b.order_host.size()), b.order_host.data(),
                                       b.order_host.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
                BMX_HIP(hipStreamSynchronize(stream_));
            }
        });
    }

    void add_block(const double* x_block, int64_t m) {
        const double t0 = now_ms();
        add(x_block, m, [&](LinearBatch& b, double*) {
            if (expect_kind_ != 0) {
                BMX_HIP(hipEventRecord(landed_, stream_));
                BMX_HIP(hipStreamWaitEvent(kstream_, landed_, 0));
                launch_sums(b, expect_kind_, expect_base_, expect_pseudo_);
            }
            if (b.complete()) {
                BMX_HIP(hipStreamSynchronize(stream_));
                BMX_HIP(hipStreamSynchronize(kstream_));
                timer_.collect(ms_);
            }
        });
        ms_[0] += now_ms() - t0;
    }

    // outs[b]: [G x n_b] column-major host memory; avg_out [G x B], ref_out [G] (nullable)
    void rescale(double log_base, double pseudo, double* const* outs, double* avg_out, double* ref_out) {
        linear_check_rescale(log_base, pseudo);
        if (batches_.size() < 2) throw Error(BMX_ERR_ARG, "at least two batches must be specified");
        check_ready(outs);
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        const int G = G_, B = (int)batches_.size();
        double* stats = stats_.reserve((size_t)(2 * B + 1) * G);  // avg [B][G], scale [B][G], ref [G]
        double* scale = stats + (size_t)B * G;
        double* ref = scale + (size_t)B * G;
        means(2, log_base, pseudo, stats);
        const int ea = mark();
        hipLaunchKernelGGL(rescale_stats_kernel, dim3((unsigned)cdiv(G, 256)), dim3(256), 0, kstream_, (const double*)stats,
                           G, B, ref, scale);
        BMX_LAUNCH_CHECK();
        timer_.span(2, ea, mark());
        const int mode = mode_of(log_base);
        const double lob = std::log(log_base);
        second_pass(outs, [&](int bi, const LinearBatch& b, int64_t c0, int mb, double* out) {
            const dim3 grid((unsigned)cdiv(G, 256), (unsigned)cdiv(mb, CPW));
            const double* sc = scale + (size_t)bi * G;
            const double* src = (b.has_u ? b.u.p : b.x.p) + c0 * G;
#define BMX_RESCALE(MODE, FROMU)                                                                                       \
    hipLaunchKernelGGL((rescale_kernel<MODE, FROMU>), grid, dim3(256), 0, kstream_, src, G, mb, sc, log_base, pseudo, \
                       lob, out)
            switch (mode * 2 + (b.has_u ? 1 : 0)) {
                case 2: BMX_RESCALE(1, false); break;
                case 3: BMX_RESCALE(1, true); break;
                case 4: BMX_RESCALE(2, false); break;
                case 5: BMX_RESCALE(2, true); break;
                case 6: BMX_RESCALE(3, false); break;
                default: BMX_RESCALE(3, true); break;
            }
#undef BMX_RESCALE
        });
        fetch_small(avg_out, stats, (size_t)B * G);
        fetch_small(ref_out, ref, (size_t)G);
        timer_.collect(ms_);
    }

    // design null: one indicator column per batch, coef_out [G x B] (the batch means).  Otherwise design [N x p]
    // column-major over the cells of all batches in upload order, w [R x p] column-major with coef = X[:, restricted] %*% w
    // (R: the restricted cells, batch by batch, ascending within a batch), keep 1-based columns that are not regressed
    // out; coef_out [G x p] (nullable)
    void regress(const double* design, int p, const double* w, const int32_t* keep, int n_keep, double* const* outs,
                 double* coef_out) {
        linear_check_regress(design, p, w, keep, n_keep);
        check_ready(outs);
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        const int G = G_;
        const Coefficients cf = fit_coefficients(design, p, w, keep, n_keep);
        if (!design) {
            second_pass(outs, [&](int bi, const LinearBatch& b, int64_t c0, int mb, double* out) {
                hipLaunchKernelGGL(subtract_kernel, dim3((unsigned)cdiv(G, 256), (unsigned)cdiv(mb, CPW)), dim3(256), 0,
                                   kstream_, (const double*)(b.x.p + c0 * G), G, mb, cf.coef + (size_t)bi * G, out);
            });
        } else {
            const std::vector<int64_t> cell0 = first_cells();
            second_pass(outs, [&](int bi, const LinearBatch& b, int64_t c0, int mb, double* out) {
                hipLaunchKernelGGL(residual_kernel, dim3((unsigned)cdiv(G, 256), (unsigned)cdiv(mb, CPW)), dim3(256), 0,
                                   kstream_, (const double*)(b.x.p + c0 * G), G, mb, cf.coef, (const int32_t*)drop_.p,
                                   (const double*)(d_.p + (size_t)(cell0[(size_t)bi] + c0) * cf.pd16), cf.pd16, out);
            });
        }
        fetch_small(coef_out, cf.coef, (size_t)cf.ncoef * G);
        timer_.collect(ms_);
    }

    // the batches as they were uploaded, back through the download ring with no kernel in between: what moving a call's
    // bytes in and out costs at the least
    void fetch(double* const* outs) {
        check_ready(outs);
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        const double t0 = now_ms();
        std::vector<XferPiece> pieces;
        for (size_t i = 0; i < batches_.size(); ++i)
            pieces.push_back(XferPiece{outs[i], batches_[i]->x.p, (size_t)batches_[i]->n * G_ * sizeof(double)});
        download_pieces(pieces.data(), pieces.size(), stream_);
        BMX_HIP(hipStreamSynchronize(stream_));
        ms_[4] += now_ms() - t0;
    }

    // milliseconds since the handle was made: upload (host wall time), HIP-event time of the first pass (chunk sums or
    // the product with w), of the statistics kernels, of the second pass's kernels, and the host wall time of the second
    // pass with its downloads
    using ResidentBatches::stage_ms;

  private:
    int mark() { return timer_.mark(kstream_); }  // a timing event recorded on the kernel stream now
    void check_ready(double* const* outs) {
        if (batches_.empty()) throw Error(BMX_ERR_ARG, "no batch has been added");
        if (!outs) throw Error(BMX_ERR_ARG, "'outs' is missing");
        for (size_t i = 0; i < batches_.size(); ++i) {
            if (batches_[i]->filled != batches_[i]->n) throw Error(BMX_ERR_ARG, "a batch has not received all its cells");
            if (!outs[i]) throw Error(BMX_ERR_ARG, "an output matrix is missing");
        }
    }
    void check_filled() const {
        if (batches_.empty()) throw Error(BMX_ERR_ARG, "no batch has been added");
        for (auto& b : batches_)
            if (b->filled != b->n) throw Error(BMX_ERR_ARG, "a batch has not received all its cells");
    }
    std::vector<int64_t> first_cells() const {  // [B + 1]: where each batch's cells start among all cells
        std::vector<int64_t> cell0(batches_.size() + 1, 0);
        for (size_t bi = 0; bi < batches_.size(); ++bi) cell0[bi + 1] = cell0[bi] + batches_[bi]->n;
        return cell0;
    }

    // The first pass of regress(): the coefficients on the device, in stats_ as [ncoef][G].  Without a design they are
    // the batch means; with one, d_ holds the dropped design columns [N][pd16] and drop_ their indices for residual_kernel.
    struct Coefficients {
        const double* coef;
        int ncoef, pd, pd16;
        std::vector<int32_t> drop;  // the dropped columns, ascending (pd of them)
    };
    Coefficients fit_coefficients(const double* design, int p, const double* w, const int32_t* keep, int n_keep) {
        const int G = G_, B = (int)batches_.size();
        if (!design) {
            double* mean = stats_.reserve((size_t)(2 * B + 1) * G);
            means(1, 0.0, 0.0, mean);
            return {mean, B, 0, 0, {}};
        }
        // the weights and the dropped columns of the design, row-major and padded to whole tiles, on the host
        int64_t N = 0, R = 0, nch = 0;
        for (auto& b : batches_) {
            N += b->n;
            R += b->m;
            nch += cdiv(b->m, GCH);
        }
        if (nch > 0x7fffffffll) throw Error(BMX_ERR_ARG, "too many cells");
        const int p16 = cdiv(p, PT) * PT;
        std::vector<char> kept((size_t)p, 0);
        for (int i = 0; i < n_keep; ++i) kept[(size_t)(keep[i] - 1)] = 1;
        std::vector<int32_t> drop;
        for (int j = 0; j < p; ++j)
            if (!kept[(size_t)j]) drop.push_back(j);
        const int pd = (int)drop.size();
        const int pd16 = cdiv(pd, PT) * PT;
        std::vector<int32_t> dropped = drop;
        drop.resize((size_t)pd16, -1);
        std::vector<double> wp((size_t)R * p16, 0.0), dp((size_t)N * pd16, 0.0);
        HostPool::get().parallel_for((size_t)p, [&](size_t j) {
            for (int64_t r = 0; r < R; ++r) wp[(size_t)r * p16 + j] = w[j * (size_t)R + r];
        });
        HostPool::get().parallel_for((size_t)pd, [&](size_t j) {
            const double* col = design + (size_t)drop[j] * N;
            for (int64_t c = 0; c < N; ++c) dp[(size_t)c * pd16 + j] = col[c];
        });
        double* W = w_.reserve(wp.size());
        double* D = d_.reserve(dp.size() + 1);
        int32_t* dropd = drop_.reserve(drop.size() + 1);
        double* part = gpart_.reserve((size_t)nch * p16 * G);
        double* coef = stats_.reserve((size_t)std::max(p16, 2 * B + 1) * G);
        const double t0 = now_ms();
        upload_pageable(W, wp.data(), wp.size() * sizeof(double), stream_);
        upload_pageable(D, dp.data(), dp.size() * sizeof(double), stream_);
        if (!drop.empty())
            BMX_HIP(hipMemcpyAsync(dropd, drop.data(), drop.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
        BMX_HIP(hipStreamSynchronize(stream_));
        ms_[0] += now_ms() - t0;
        const int ea = mark();
        int64_t row0 = 0, ch0 = 0;
        for (auto& bp : batches_) {
            LinearBatch& b = *bp;
            const int nc = cdiv(b.m, GCH);
            hipLaunchKernelGGL(coef_partial_kernel, dim3((unsigned)nc, (unsigned)cdiv(G, 256), (unsigned)(p16 / PT)),
                               dim3(256), 0, kstream_, (const double*)b.x.p, G,
                               (const int32_t*)(b.order_host.empty() ? nullptr : b.order.p), b.m, (const double*)W, row0, p16,
                               part + (size_t)ch0 * p16 * G);
            BMX_LAUNCH_CHECK();
            row0 += b.m;
            ch0 += nc;
        }
        hipLaunchKernelGGL(coef_reduce_kernel, dim3((unsigned)cdiv(G, 256), (unsigned)p16), dim3(256), 0, kstream_,
                           (const double*)part, G, p16, (int)nch, coef);
        BMX_LAUNCH_CHECK();
        timer_.span(1, ea, mark());
        return {coef, p, pd, pd16, std::move(dropped)};
    }

    void fetch_small(double* host, const double* dev, size_t n) {
        if (!host) return;
        BMX_HIP(hipMemcpyAsync(host, dev, n * sizeof(double), hipMemcpyDeviceToHost, kstream_));
        BMX_HIP(hipStreamSynchronize(kstream_));
    }

    // the chunks of b that are complete with the cells resident so far and not summed yet, on the kernel stream
    void launch_sums(LinearBatch& b, int kind, double base, double pseudo) {
        if (b.sum_kind != kind || b.sum_base != base || b.sum_pseudo != pseudo) {
            b.sum_kind = kind;
            b.sum_base = base;
            b.sum_pseudo = pseudo;
            b.sum_done = 0;
        }
        int64_t have = b.filled;  // restricted cells resident: the list is ascending, so they are a prefix of it
        if (!b.order_host.empty())
            have = std::lower_bound(b.order_host.begin(), b.order_host.end(), (int32_t)std::min<int64_t>(b.filled, 0x7fffffff)) -
                   b.order_host.begin();
        const int complete = b.chunks_complete(have, b.m, LCH);
        if (complete <= b.sum_done) return;
        const int G = G_;
        const dim3 grid((unsigned)(complete - b.sum_done), (unsigned)cdiv(G, 256));
        const int32_t* order = b.order_host.empty() ? nullptr : b.order.p;
        const int mode = kind == 1 ? 0 : mode_of(base);
        const int ea = mark();
#define BMX_SUMS(MODE, KEEP)                                                                                          \
    hipLaunchKernelGGL((sum_partial_kernel<MODE, KEEP>), grid, dim3(256), 0, kstream_, (const double*)b.x.p, G, order, \
                       b.m, b.sum_done, base, pseudo, b.part.p, b.u.p)
        switch (mode * 2 + (mode != 0 && b.has_u ? 1 : 0)) {
            case 0: BMX_SUMS(0, false); break;
            case 2: BMX_SUMS(1, false); break;
            case 3: BMX_SUMS(1, true); break;
            case 4: BMX_SUMS(2, false); break;
            case 5: BMX_SUMS(2, true); break;
            case 6: BMX_SUMS(3, false); break;
            default: BMX_SUMS(3, true); break;
        }
#undef BMX_SUMS
        BMX_LAUNCH_CHECK();
        timer_.span(1, ea, mark());
        b.sum_done = complete;
    }

    // mean [B][G] of every batch's (unlogged) restricted cells: the chunk sums that add_block has not made, then the means
    void means(int kind, double base, double pseudo, double* mean) {
        const int G = G_;
        for (size_t bi = 0; bi < batches_.size(); ++bi) {
            LinearBatch& b = *batches_[bi];
            launch_sums(b, kind, base, pseudo);
            const int ea = mark();
            hipLaunchKernelGGL(mean_kernel, dim3((unsigned)cdiv(G, 256)), dim3(256), 0, kstream_, (const double*)b.part.p, G,
                               b.nchunks, (double)b.m, mean + bi * (size_t)G);
            BMX_LAUNCH_CHECK();
            timer_.span(2, ea, mark());
        }
    }

    // Every batch in blocks of cells: launch(bi, batch, first cell, cells, device out) queues the kernel of a block on the
    // kernel stream; the block then goes to outs[bi] through the download ring on the copy stream while the next
    // block's kernel runs into the other buffer.
    template <class F>
    void second_pass(double* const* outs, F&& launch) {
        const double t0 = now_ms();
        const int G = G_;
        // (the second grid dimension holds at most 65 535 workgroups of CPW cells)
        const int64_t per = std::min<int64_t>(
            65535 * (int64_t)CPW, std::max<int64_t>(1, (int64_t)(OUT_BLOCK_BYTES / (sizeof(double) * (size_t)G))));
        blocked_output(batches_, G, per, kstream_, stream_, timer_, 3, out_, outs, launch);
        ms_[4] += now_ms() - t0;
    }

    hipStream_t kstream_ = nullptr;  // kernels (the store's stream_ takes the copies)
    hipEvent_t landed_ = nullptr;
    DevBuf<double> stats_, w_, d_, gpart_, out_[2];
    DevBuf<int32_t> drop_;
    int expect_kind_ = 0;
    double expect_base_ = 0.0, expect_pseudo_ = 0.0;
    bool keep_u_ = false;
    unsigned long long generation_ = 0;  // counts begin_batch: what a ResidualPca was made for
};

// ---------------------------------------------------------------------------------------------------
// regressBatches(d=, deferred=TRUE) (R/regressBatches.R:148-155): multiBatchPCA of the residuals, which are never formed.
// Borrows a Linear whose batches are all resident, as PcaGenes borrows a Pca: its batches are the PCA's batches, its first
// pass fits the coefficients.  The Linear must outlive this handle; a batch begun on it since makes every later call an
// error.  Own stream, own buffers: nothing here is touched by rescale() / regress(), which still write every cell.
// ---------------------------------------------------------------------------------------------------
class ResidualPca {
  public:
    // the PCA runs over the first nS rows of the Linear's batches
    ResidualPca(int nS, Linear* lin) : lin_(*lin), made_for_(lin->generation_), device_(lin->device_), nS_(nS) {
        if (nS < 1 || nS > lin_.G_) throw Error(BMX_ERR_ARG, "'n_pca_rows' is between 1 and the number of genes");
        lin_.check_filled();
        BMX_HIP(hipSetDevice(device_));
        BMX_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    }
    ResidualPca(const ResidualPca&) = delete;
    ResidualPca& operator=(const ResidualPca&) = delete;
    ~ResidualPca() {
        (void)hipSetDevice(device_);
        if (stream_) {
            (void)hipStreamSynchronize(stream_);
            (void)hipStreamDestroy(stream_);
        }
        DevBlockCache::current() = &cache_;  // as ResidentBatches::retire(): the buffers below go back to cache_
    }

    // regressBatches(d=, deferred=TRUE): the coefficients exactly as regress() fits them (coef_out as there), then
    // multiBatchPCA (R/multiBatchPCA.R:211-322, the iteration of pca.hip) of the residuals over the first nS rows, the
    // resident batches being the PCA's batches with weights[b] (null: equal).  With K = coef[, drop] (G x pd), Dd_b the
    // dropped design columns of batch b's cells and d_b their mean row, the residual of batch b is R_b = x_b - K Dd_b^T, its
    // mean over ALL its cells r_b = mean(x_b) - K d_b, the grand centre mu = sum_b w_b r_b / sum_b w_b and the centred
    // batch C_b = R_b - mu 1^T = x_b - F E_b^T with E_b = [Dd_b | 1] (n_b x (pd + 1)), F = [K | mu].  Per 64 columns Q:
    //     T = F^T Q;   Z_b = x_b^T Q - E_b T;   S_b = E_b^T Z_b;   Y += (w_b / n_b) (x_b Z_b - F S_b)
    // Both big products are gemm_nt64 / gemm_tn64 on the resident x_b (rows nS of leading dimension G); T and S_b are the
    // same two kernels on F^T and E_b; the two corrections are lowrank_sub_kernel.  Without a design the term is rank one
    // per batch, c_b = (restricted mean of b) + mu: gemm_nt64's `off` and rank1_sub, as Pca::apply_operator.  Every sum is
    // in a fixed order (splits through reduce_parts), no atomics.  centers [nS], rotation [nS x d] column-major, sdev [d];
    // tol <= 0: exactly max_applies plain steps (Pca::fit).  Throws after writing the results when tol is not reached.
    void fit(const double* design, int p, const double* w, const int32_t* keep, int n_keep, const double* weights, int d,
             double tol, int max_applies, double* coef_out, double* centers, double* rotation, double* sdev,
             int* applies_used, double* resid_out) {
        const int nS = nS_;
        linear_check_regress(design, p, w, keep, n_keep);
        linear_check_pca(lin_.G_, nS, d, tol, max_applies, weights, (int)lin_.batches_.size());
        check_fresh();
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        fitted_ = false;
        const int G = lin_.G_, B = (int)lin_.batches_.size();
        int64_t N = 0;
        for (auto& b : lin_.batches_) N += b->n;
        const int L = SubspaceIteration::width_for(d, nS, N, max_applies);
        const Linear::Coefficients cf = [&] {  // on the Linear's own stream and buffers, drained before the PCA reads them
            CacheScope theirs(&lin_.cache_);
            Linear::Coefficients c = lin_.fit_coefficients(design, p, w, keep, n_keep);
            lin_.fetch_small(coef_out, c.coef, (size_t)c.ncoef * G);
            BMX_HIP(hipStreamSynchronize(lin_.kstream_));
            lin_.timer_.collect(lin_.ms_);
            return c;
        }();
        // ---- what the operator keeps: the weights, and per batch the dropped columns and their mean design row
        pca_w_.assign((size_t)B, 1.0);
        if (weights) pca_w_.assign(weights, weights + B);
        double wsum = 0.0;
        for (double v : pca_w_) wsum += v;
        const int pd = design ? cf.pd : 1;  // without a design batch b drops its own indicator column
        pca_design_ = design != nullptr;
        pe_ = pd + 1;
        pe16_ = cdiv(pe_, PT) * PT;
        const std::vector<int64_t> cell0 = first_cell_ = lin_.first_cells();
        std::vector<int32_t> drops((size_t)B * pd);
        std::vector<double> dbar((size_t)B * pd, 1.0);
        for (int bi = 0; bi < B; ++bi)
            for (int k = 0; k < pd; ++k) {
                drops[(size_t)bi * pd + k] = design ? cf.drop[(size_t)k] : bi;
                if (!design) continue;
                const double* col = design + (size_t)cf.drop[(size_t)k] * N + cell0[(size_t)bi];
                double s = 0.0;
                for (int64_t c = 0; c < lin_.batches_[(size_t)bi]->n; ++c) s += col[c];
                dbar[(size_t)bi * pd + k] = s / (double)lin_.batches_[(size_t)bi]->n;
            }
        int32_t* ddrops = pdrop_.reserve(drops.size() + 1);
        double* ddbar = pdbar_.reserve(dbar.size() + 1);
        if (!drops.empty()) {
            BMX_HIP(hipMemcpyAsync(ddrops, drops.data(), drops.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
            BMX_HIP(hipMemcpyAsync(ddbar, dbar.data(), dbar.size() * sizeof(double), hipMemcpyHostToDevice, stream_));
        }
        // ---- scratch for the largest batch, sized once: a buffer that grew while kernels run would change hands
        size_t zmax = 0, pmax = 0;
        for (auto& bp : lin_.batches_) {
            int64_t per = 0;
            const size_t sums = (size_t)std::min<int64_t>(512, std::max<int64_t>(1, bp->n / 256)) * G + (size_t)G;
            const size_t prod = (size_t)tn_splits(cdiv(nS, 64), bp->n, per) * nS * PL +
                                (size_t)tn_splits(cdiv(pe_, 64), bp->n, per) * pe16_ * PL + (size_t)4096 * PL;
            zmax = std::max(zmax, (size_t)bp->n * PL);
            pmax = std::max({pmax, sums, prod});
        }
        z_.reserve(zmax);
        zt_.reserve(zmax);
        ppart_.reserve(pmax);
        // ---- the grand centre of the residuals, from every batch's mean over all its cells
        double* mu = mu_.reserve((size_t)nS);
        BMX_HIP(hipMemsetAsync(mu, 0, (size_t)nS * sizeof(double), stream_));
        for (int bi = 0; bi < B; ++bi) {
            LinearBatch& b = *lin_.batches_[(size_t)bi];
            const int nchunk = (int)std::min<int64_t>(512, std::max<int64_t>(1, b.n / 256));
            const int64_t per = (b.n + nchunk - 1) / nchunk;
            double* part = ppart_.p;
            double* mean = part + (size_t)nchunk * G;
            hipLaunchKernelGGL(genesum_partial, dim3(cdiv(G, 256), nchunk), dim3(256), 0, stream_, (const double*)b.x.p,
                               (const double*)nullptr, b.n, G, per, part);
            hipLaunchKernelGGL(reduce_parts, dim3((unsigned)cdiv(G, 256)), dim3(256), 0, stream_, (const double*)part, nchunk,
                               (int64_t)G, 1.0 / (double)b.n, 0.0, mean, G, (int64_t)G);
            hipLaunchKernelGGL(residual_centre_kernel, dim3((unsigned)cdiv(nS, 256)), dim3(256), 0, stream_, mu,
                               (const double*)mean, cf.coef, (int64_t)G, (const int32_t*)(ddrops + (size_t)bi * pd),
                               (const double*)(ddbar + (size_t)bi * pd), pd, pca_w_[(size_t)bi] / wsum, nS);
            BMX_LAUNCH_CHECK();
        }
        // ---- the low-rank term's operands
        if (pca_design_) {
            std::vector<double> ep((size_t)N * pe16_, 0.0);  // E = [D[, drop] | 1], row-major, zero padded
            HostPool::get().parallel_for((size_t)pe_, [&](size_t k) {
                const double* col = (int)k < pd ? design + (size_t)cf.drop[k] * N : nullptr;
                for (int64_t c = 0; c < N; ++c) ep[(size_t)c * pe16_ + k] = col ? col[c] : 1.0;
            });
            upload_pageable(e_.reserve(ep.size()), ep.data(), ep.size() * sizeof(double), stream_);
            BMX_HIP(hipStreamSynchronize(stream_));
            ft_.reserve((size_t)pe_ * nS);
            fg_.reserve((size_t)nS * pe16_);
            hipLaunchKernelGGL(pack_f_kernel, dim3((unsigned)cdiv((int64_t)nS * pe16_, 256)), dim3(256), 0, stream_, cf.coef,
                               (int64_t)G, (const int32_t*)ddrops, pd, (const double*)mu, nS, pe16_, ft_.p, fg_.p);
            BMX_LAUNCH_CHECK();
            ts_.reserve(2 * (size_t)pe16_ * PL);  // T and S_b, rows pe_ .. pe16_ stay zero
            BMX_HIP(hipMemsetAsync(ts_.p, 0, 2 * (size_t)pe16_ * PL * sizeof(double), stream_));
        } else {
            double* c = c_.reserve((size_t)B * nS);  // c_b = (restricted mean of b) + mu
            for (int bi = 0; bi < B; ++bi) {
                hipLaunchKernelGGL(lincomb3, dim3((unsigned)cdiv(nS, 256)), dim3(256), 0, stream_, c + (size_t)bi * nS, 1.0,
                                   cf.coef + (size_t)bi * G, 1.0, (const double*)mu, 0.0, (const double*)nullptr, (int64_t)nS);
                BMX_LAUNCH_CHECK();
            }
        }
        qt_.reserve((size_t)nS * PL);
        off_.reserve(2 * (size_t)PL);
        BMX_HIP(hipStreamSynchronize(stream_));
        const SubspaceIteration::Outcome outcome =
            it_.run(stream_, nS, d, tol, max_applies, [&](const double* Q, double* Y) { apply_operator(Q, Y); });
        // ---- results: rotation = the first d Ritz vectors, kept transposed for the projections
        const double* Xr = it_.ritz_vectors();
        double* Ut = ut_.reserve((size_t)nS * L);
        for (int h = 0; h < L / PL; ++h) {
            hipLaunchKernelGGL(transpose64, dim3((unsigned)cdiv(nS, 64)), dim3(256), 0, stream_, (const double*)(Xr + h * PL),
                               (int64_t)L, (int64_t)nS, Ut + (size_t)h * PL * nS);
            BMX_LAUNCH_CHECK();
        }
        if (centers) BMX_HIP(hipMemcpyAsync(centers, mu, (size_t)nS * sizeof(double), hipMemcpyDeviceToHost, stream_));
        if (rotation)
            BMX_HIP(hipMemcpyAsync(rotation, Ut, (size_t)nS * d * sizeof(double), hipMemcpyDeviceToHost, stream_));
        BMX_HIP(hipStreamSynchronize(stream_));
        fitted_ = true;
        it_.report(tol, outcome, sdev, applies_used, resid_out);
    }

    // crossprod(residuals of batch b - centers, rotation) of the PCA fitted last: [n_b x d] column-major
    void project(int b, double* out) {
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        check_fresh();
        if (!fitted_) throw Error(BMX_ERR_ARG, "bmx_residual_pca_fit has not been run");
        if (b < 0 || b >= (int)lin_.batches_.size()) throw Error(BMX_ERR_ARG, "batch index out of range");
        if (!out) throw Error(BMX_ERR_ARG, "null output pointer");
        const LinearBatch& Bt = *lin_.batches_[(size_t)b];
        double* Z = z_.p;  // (sized by fit)
        double* Zt = zt_.p;
        const int d = it_.d();
        for (int h = 0; h * PL < d; ++h) {
            if (pca_design_) lowrank_image(ut_.p + (size_t)h * PL * nS_);
            centred_product(b, ut_.p + (size_t)h * PL * nS_, Z);
            hipLaunchKernelGGL(transpose64, dim3((unsigned)cdiv(Bt.n, 64)), dim3(256), 0, stream_, (const double*)Z,
                               (int64_t)PL, Bt.n, Zt);
            BMX_LAUNCH_CHECK();
            const int cols = std::min(PL, d - h * PL);
            BMX_HIP(hipMemcpyAsync(out + (size_t)h * PL * Bt.n, Zt, (size_t)Bt.n * cols * sizeof(double),
                                   hipMemcpyDeviceToHost, stream_));
            BMX_HIP(hipStreamSynchronize(stream_));  // Z / Zt are reused by the next half
        }
    }

  private:
    void check_fresh() const {
        if (lin_.generation_ != made_for_) throw Error(BMX_ERR_ARG, "a batch was begun after bmx_residual_pca_create");
        lin_.check_filled();
    }

    // Z [n_b][64] = C_b^T Bq for batch bi and 64 vectors Bq [64][nS_] row-major (a block's Q^T, or rotation rows): the
    // product with the resident x_b less the low-rank term.  With a design T = F^T Bq is left in ts_ (rows [0, pe_)).
    void centred_product(int bi, const double* Bq, double* Z) {
        const LinearBatch& b = *lin_.batches_[(size_t)bi];
        const int G = lin_.G_, nS = nS_;
        if (!pca_design_) {
            double* cq = off_.p;  // c_b . Bq_j
            hipLaunchKernelGGL(gemm_nt64, dim3(1), dim3(256), 0, stream_, (const double*)(c_.p + (size_t)bi * nS), (int64_t)1,
                               nS, (int64_t)nS, Bq, (int64_t)nS, (const double*)nullptr, (const double*)nullptr, cq,
                               (int64_t)PL);
            hipLaunchKernelGGL(gemm_nt64, dim3((unsigned)cdiv(b.n, 64)), dim3(256), 0, stream_, (const double*)b.x.p, b.n, nS,
                               (int64_t)G, Bq, (int64_t)nS, (const double*)nullptr, (const double*)cq, Z, (int64_t)PL);
            BMX_LAUNCH_CHECK();
            return;
        }
        hipLaunchKernelGGL(gemm_nt64, dim3((unsigned)cdiv(b.n, 64)), dim3(256), 0, stream_, (const double*)b.x.p, b.n, nS,
                           (int64_t)G, Bq, (int64_t)nS, (const double*)nullptr, (const double*)nullptr, Z, (int64_t)PL);
        hipLaunchKernelGGL(lowrank_sub_kernel, dim3((unsigned)cdiv(b.n, 4 * RPW)), dim3(256), 0, stream_, Z, (int64_t)PL, b.n,
                           (const double*)(e_.p + (size_t)first_cell_[(size_t)bi] * pe16_), (const double*)ts_.p, pe16_, 1.0);
        BMX_LAUNCH_CHECK();
    }
    // T = F^T Bq into ts_: the rows of F^T are the "cells" of the NT product
    void lowrank_image(const double* Bq) {
        hipLaunchKernelGGL(gemm_nt64, dim3((unsigned)cdiv(pe_, 64)), dim3(256), 0, stream_, (const double*)ft_.p, (int64_t)pe_,
                           nS_, (int64_t)nS_, Bq, (int64_t)nS_, (const double*)nullptr, (const double*)nullptr, ts_.p,
                           (int64_t)PL);
        BMX_LAUNCH_CHECK();
    }

    // the splits of a TN product over a batch's n cells with `tiles` output tiles (Pca::apply_operator's rule); per: the
    // cells of a split
    static int tn_splits(int tiles, int64_t n, int64_t& per) {
        const int ns = (int)std::min<int64_t>(std::max<int64_t>(1, (int64_t)1024 / tiles), std::max<int64_t>(1, n / 2048));
        per = round_up((n + ns - 1) / ns, KC);
        return (int)((n + per - 1) / per);
    }

    // Y = M Q = sum_b (w_b / n_b) C_b C_b^T Q for a block of L vectors over the first nS_ rows, 64 at a time
    void apply_operator(const double* Q, double* Y) {
        const int G = lin_.G_, nS = nS_, L = it_.L();
        double* Qt = qt_.p;
        double* zsum = off_.p + PL;
        BMX_HIP(hipMemsetAsync(Y, 0, (size_t)nS * L * sizeof(double), stream_));
        const int gtiles = cdiv(nS, 64), etiles = cdiv(pe_, 64);
        for (int h = 0; h < L / PL; ++h) {
            hipLaunchKernelGGL(transpose64, dim3((unsigned)cdiv(nS, 64)), dim3(256), 0, stream_, Q + h * PL, (int64_t)L,
                               (int64_t)nS, Qt);
            BMX_LAUNCH_CHECK();
            if (pca_design_) lowrank_image(Qt);
            double* Yh = Y + h * PL;
            for (size_t bi = 0; bi < lin_.batches_.size(); ++bi) {
                const LinearBatch& b = *lin_.batches_[bi];
                const double coef = pca_w_[bi] / (double)b.n;
                int64_t per = 0, per_e = 0;
                const int nsplit = tn_splits(gtiles, b.n, per), nsplit_e = tn_splits(etiles, b.n, per_e);
                double* Z = z_.p;  // (fit has sized z_ and ppart_ for the largest batch)
                double* part = ppart_.p;
                double* spart = part + (size_t)nsplit * nS * PL;
                double* zpart = spart + (size_t)nsplit_e * pe16_ * PL;
                centred_product((int)bi, Qt, Z);
                hipLaunchKernelGGL(gemm_tn64, dim3(gtiles, nsplit), dim3(256), 0, stream_, (const double*)b.x.p, b.n, nS,
                                   (int64_t)G, (const double*)Z, (int64_t)PL, (const double*)nullptr, per, part);
                hipLaunchKernelGGL(reduce_parts, dim3((unsigned)cdiv((int64_t)nS * PL, 256)), dim3(256), 0, stream_,
                                   (const double*)part, nsplit, (int64_t)nS * PL, coef, 1.0, Yh, PL, (int64_t)L);
                BMX_LAUNCH_CHECK();
                if (!pca_design_) {  // Y -= coef c_b (1^T Z)
                    column_sums64(stream_, Z, b.n, zpart, 1.0, 0.0, zsum);
                    hipLaunchKernelGGL(rank1_sub, dim3((unsigned)cdiv((int64_t)nS * PL, 256)), dim3(256), 0, stream_, Yh,
                                       (int64_t)L, (const double*)(c_.p + bi * (size_t)nS), (const double*)zsum, coef, nS);
                    BMX_LAUNCH_CHECK();
                    continue;
                }
                // S_b = E_b^T Z (E_b as an n_b x pe_ row-major "batch"), then Y -= coef F S_b
                double* S = ts_.p + (size_t)pe16_ * PL;
                hipLaunchKernelGGL(gemm_tn64, dim3(etiles, nsplit_e), dim3(256), 0, stream_,
                                   (const double*)(e_.p + (size_t)first_cell_[bi] * pe16_), b.n, pe_, (int64_t)pe16_,
                                   (const double*)Z, (int64_t)PL, (const double*)nullptr, per_e, spart);
                hipLaunchKernelGGL(reduce_parts, dim3((unsigned)cdiv(pe_ * PL, 256)), dim3(256), 0, stream_,
                                   (const double*)spart, nsplit_e, (int64_t)pe_ * PL, 1.0, 0.0, S, PL, (int64_t)PL);
                hipLaunchKernelGGL(lowrank_sub_kernel, dim3((unsigned)cdiv(nS, 4 * RPW)), dim3(256), 0, stream_, Yh, (int64_t)L,
                                   (int64_t)nS, (const double*)fg_.p, (const double*)S, pe16_, coef);
                BMX_LAUNCH_CHECK();
            }
        }
    }

    DevBlockCache cache_;  // first: destroyed after every DevBuf below
    Linear& lin_;
    const unsigned long long made_for_;
    int device_;
    hipStream_t stream_ = nullptr;
    SubspaceIteration it_;
    bool fitted_ = false, pca_design_ = false;
    int nS_, pe_ = 0, pe16_ = 0;  // PCA rows; columns of E_b / F, and padded to whole tiles of PT
    std::vector<double> pca_w_;       // the batches' weights
    std::vector<int64_t> first_cell_;
    // mu_ [nS] the grand centre; c_ [B][nS] (no design); e_ [N][pe16] E of all cells, ft_ [pe][nS] / fg_ [nS][pe16] F both
    // ways round, ts_ [2][pe16][64] T and S_b (design); qt_ / ut_ the block and the rotation transposed; off_ c_b . Q and
    // the column sums of Z; ppart_ the split partials
    DevBuf<double> mu_, c_, e_, ft_, fg_, ts_, qt_, ut_, z_, zt_, off_, ppart_, pdbar_;
    DevBuf<int32_t> pdrop_;
};

}  // namespace bmx

/* ---------------------------------------------------------------- bmx_linear_* ---------------------------------- */
struct bmx_linear final : bmx::Linear {
    using Linear::Linear;
};

struct bmx_residual_pca final : bmx::ResidualPca {
    using ResidualPca::ResidualPca;
};

extern "C" {

int32_t bmx_linear_create(int32_t device, int32_t G, bmx_linear_t** out) {
    return bmx::guarded([&] {
        if (!out) throw bmx::Error(BMX_ERR_ARG, "null output pointer");
        if (G < 1) throw bmx::Error(BMX_ERR_ARG, "the linear corrections need at least one gene");
        *out = new bmx_linear(device, G);
    });
}

void bmx_linear_destroy(bmx_linear_t* h) { delete h; }

int32_t bmx_linear_expect(bmx_linear_t* h, int32_t kind, double log_base, double pseudo_count, int32_t keep_unlogged) {
    return bmx::guarded([&] { bmx::live(h).expect(kind, log_base, pseudo_count, keep_unlogged); });
}

int32_t bmx_linear_begin_batch(bmx_linear_t* h, int64_t n, const int32_t* restrict_idx, int64_t n_restrict) {
    return bmx::guarded([&] { bmx::live(h).begin_batch(n, restrict_idx, n_restrict); });
}

int32_t bmx_linear_add_block(bmx_linear_t* h, const double* x_block, int64_t n_block) {
    return bmx::guarded([&] { bmx::live(h).add_block(x_block, n_block); });
}

int32_t bmx_linear_rescale(bmx_linear_t* h, double log_base, double pseudo_count, double* const* outs, double* avg_out,
                           double* ref_out) {
    return bmx::guarded([&] { bmx::live(h).rescale(log_base, pseudo_count, outs, avg_out, ref_out); });
}

int32_t bmx_linear_regress(bmx_linear_t* h, const double* design, int32_t p, const double* w, const int32_t* keep,
                           int32_t n_keep, double* const* outs, double* coef_out) {
    return bmx::guarded([&] { bmx::live(h).regress(design, p, w, keep, n_keep, outs, coef_out); });
}

int32_t bmx_linear_check_pca(int32_t n_genes, int32_t n_pca_rows, int32_t d, double tol, int32_t max_applies,
                             const double* weights, int32_t n_batches) {
    return bmx::guarded([&] { bmx::linear_check_pca(n_genes, n_pca_rows, d, tol, max_applies, weights, n_batches); });
}

int32_t bmx_linear_fetch(bmx_linear_t* h, double* const* outs) {
    return bmx::guarded([&] { bmx::live(h).fetch(outs); });
}

int32_t bmx_linear_stage_ms(const bmx_linear_t* h, double* out5) {
    return bmx::guarded([&] {
        if (!h || !out5) throw bmx::Error(BMX_ERR_ARG, "null argument");
        h->stage_ms(out5);
    });
}

/* ---------------------------------------------------------------- bmx_residual_pca_* ---------------------------- */
int32_t bmx_residual_pca_create(int32_t n_pca_rows, bmx_linear_t* loaded, bmx_residual_pca_t** out) {
    return bmx::guarded([&] {
        if (!out) throw bmx::Error(BMX_ERR_ARG, "null output pointer");
        *out = new bmx_residual_pca(n_pca_rows, &bmx::live(loaded));
    });
}

void bmx_residual_pca_destroy(bmx_residual_pca_t* h) { delete h; }

int32_t bmx_residual_pca_fit(bmx_residual_pca_t* h, const double* design, int32_t p, const double* w, const int32_t* keep,
                             int32_t n_keep, const double* weights, int32_t d, double tol, int32_t max_applies,
                             double* coef_out, double* centers_out, double* rotation_out,
                             double* sdev_out, int32_t* iters_used, double* residual_out) {
    return bmx::guarded([&] {
        int used = 0;
        double res = 0.0;
        auto write = [&] {
            if (iters_used) *iters_used = used;
            if (residual_out) *residual_out = res;
        };
        try {
            bmx::live(h).fit(design, p, w, keep, n_keep, weights, d, tol, max_applies, coef_out, centers_out,
                             rotation_out, sdev_out, &used, &res);
        } catch (...) {
            write();
            throw;
        }
        write();
    });
}

int32_t bmx_residual_pca_project(bmx_residual_pca_t* h, int32_t batch, double* out) {
    return bmx::guarded([&] { bmx::live(h).project(batch, out); });
}

}  // extern "C"
