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
// All FP64 vector arithmetic, contraction off.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "bmx_ops.hpp"
#include "host_xfer.hpp"
#include "ordered_sums.hpp"
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
        const int G = G_, B = (int)batches_.size();
        if (!design) {
            double* mean = stats_.reserve((size_t)(2 * B + 1) * G);
            means(1, 0.0, 0.0, mean);
            second_pass(outs, [&](int bi, const LinearBatch& b, int64_t c0, int mb, double* out) {
                hipLaunchKernelGGL(subtract_kernel, dim3((unsigned)cdiv(G, 256), (unsigned)cdiv(mb, CPW)), dim3(256), 0,
                                   kstream_, (const double*)(b.x.p + c0 * G), G, mb, (const double*)(mean + (size_t)bi * G),
                                   out);
            });
            fetch_small(coef_out, mean, (size_t)B * G);
            timer_.collect(ms_);
            return;
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
        std::vector<int64_t> cell0((size_t)B + 1, 0);
        for (int bi = 0; bi < B; ++bi) cell0[(size_t)bi + 1] = cell0[(size_t)bi] + batches_[(size_t)bi]->n;
        second_pass(outs, [&](int bi, const LinearBatch& b, int64_t c0, int mb, double* out) {
            hipLaunchKernelGGL(residual_kernel, dim3((unsigned)cdiv(G, 256), (unsigned)cdiv(mb, CPW)), dim3(256), 0, kstream_,
                               (const double*)(b.x.p + c0 * G), G, mb, (const double*)coef, (const int32_t*)dropd,
                               (const double*)(D + (size_t)(cell0[(size_t)bi] + c0) * pd16), pd16, out);
        });
        fetch_small(coef_out, coef, (size_t)p * G);
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
};

}  // namespace bmx

/* ---------------------------------------------------------------- bmx_linear_* ---------------------------------- */
struct bmx_linear final : bmx::Linear {
    using Linear::Linear;
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

int32_t bmx_linear_fetch(bmx_linear_t* h, double* const* outs) {
    return bmx::guarded([&] { bmx::live(h).fetch(outs); });
}

int32_t bmx_linear_stage_ms(const bmx_linear_t* h, double* out5) {
    return bmx::guarded([&] {
        if (!h || !out5) throw bmx::Error(BMX_ERR_ARG, "null argument");
        h->stage_ms(out5);
    });
}

}  // extern "C"
