// multiBatchPCA over sparse batches (bmx_pca_sparse_*): pca.hip's blocked subspace iteration with the operator
//     M Q = sum_b (w_b / n_b) C_b C_b^T Q,   C_b = x_b diag(scale_b) - mu 1^T,
// applied from batches that stay in HBM as CSC (indptr int64 absolute, 0-based int32 rows, FP64 values), with work
// proportional to the stored entries.
//
// Rows: the handle holds all n_rows rows; the first n_rows_pca are the rows the PCA runs on, the others the genes
// outside subset.row.  Rows ascend within a column, so a cell's PCA rows are a prefix of its column: sp_prepare_kernel
// finds the cut per column behind the upload, with the pattern flags and, under cos_norm, 1 / max(1e-8, l2) over the
// prefix.  After a batch's last block a row-major companion is built on the device (rows of scaled values
// scale_c x_gc with their cells ascending) by a counting sort that uses no atomics: cells in chunks of CH, per (chunk,
// tile of GT rows) the chunk's columns are walked in ascending order with the counters in the LDS and a barrier between
// columns, so an entry's place is a function of the pattern alone.
//
// The two products take 64 subspace columns at a time with a lane per column, so every gathered row is one coalesced
// 512-byte read; there is no shared K dimension between two cells' gene sets, hence no MFMA: FP64 on the vector ALUs.
//   sp_by_cell_kernel   one wave a cell over the prefix of its column:  Z[c, :] = scale_c sum_g x_gc Q[g, :] - mu^T Q
//                       (also the projections, Q = the rotation)
//   sp_by_gene_kernel   one wave a SEGMENT of at most SEG entries of a row of the companion:
//                       part[segment, :] = sum_c (scale_c x_gc) Z[c, :];   sp_row_reduce_kernel adds a row's segments in
//                       ascending order:  Y[g, :] += coef_b (sum - mu_g 1^T Z)
// The segments are cut at fixed positions of the row, a segment's terms are added in cell order by one accumulator per
// lane and a row's segments in ascending order: neither the split nor a result depends on scheduling, on the grid or on
// how the batch was cut into blocks.  The per-batch gene sums (centres), the leftover rows' rotation and var.total read
// the same companion.  A row index is compared with its bounds before it addresses anything; a failing entry is skipped.
//
// The iteration (start block, Cholesky QR 2, Rayleigh-Ritz, Chebyshev filter, residual) is SubspaceIteration
// (pca_iteration.hpp), the one the dense handle runs: this file brings the sparse operator and keeps the centre, the
// rotation and the projections.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "bmx_ops.hpp"
#include "csc_device.hpp"
#include "host_xfer.hpp"
#include "pca_iteration.hpp"
#include "resident_batches.hpp"

namespace bmx {

namespace {

constexpr int SEG = PCA_SPARSE_ROW_SEGMENT;  // entries of a row one wave adds
constexpr int CH = 128;                      // cells per chunk of the counting sort
constexpr int GT = 4096;                     // rows per tile of the counting sort (16 KiB of counters in the LDS)

// The cells [c0, c0 + m), one wave a cell: cut[c] = the position after the column's last entry below row Gp (its PCA
// prefix), inv[c] = 1 / max(1e-8, l2 over the prefix) (inv null: not wanted).  flags: the pattern pair (csc_entry_flags).
__global__ __launch_bounds__(256) void sp_prepare_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                         const double* __restrict__ val, int G, int Gp, int64_t c0,
                                                         int64_t m, int64_t* __restrict__ cut, double* __restrict__ inv,
                                                         int32_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int64_t c = c0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= c0 + m) return;  // (a whole wave leaves)
    const int64_t kb = indptr[c], ke = indptr[c + 1];
    double s = 0.0;
    int below = 0, bad_row = 0, bad_order = 0;
    for (int64_t k = kb + lane; k < ke; k += 64) {
        const int32_t r = idx[k];
        if (csc_entry_flags(idx, k, kb, r, G, bad_row, bad_order)) continue;
        if (r < Gp) {
            const double v = val[k];
            ++below;
            s += v * v;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o);
        below += __shfl_xor(below, o);
    }
    if (bad_row) flags[CSC_F_ROW] = 1;
    if (bad_order) flags[CSC_F_ORDER] = 1;
    if (lane == 0) {
        cut[c] = kb + below;
        if (inv) inv[c] = 1.0 / cos_clamp(sqrt(s));
    }
}

// The counting sort's two walks (csc_tile_walk), workgroup (chunk, row tile).  Rows are unique within a canonical
// column, so no two threads meet at a counter (where they do, CSC_F_ORDER has been raised and the fit will refuse).
//   PLACE = false:  cnt[chunk][g] = the chunk's entries of row g
//   PLACE = true:   cnt[chunk][g] holds the row's entries in the chunks before; an entry goes to rowptr[g] + that count
//                   (kept inside the row whatever the pattern), with its cell and its value times scale
template <bool PLACE>
__global__ __launch_bounds__(256) void sp_sort_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                      const double* __restrict__ val, int G, int64_t n,
                                                      int32_t* __restrict__ cnt, const int64_t* __restrict__ rowptr,
                                                      const double* __restrict__ scale, int32_t* __restrict__ rcol,
                                                      double* __restrict__ rval) {
    __shared__ int32_t acc[GT];
    __shared__ int64_t lo[CH], hi[CH];
    const int64_t ch = blockIdx.x;
    const int g0 = blockIdx.y * GT, g1 = min(G, g0 + GT);
    for (int i = threadIdx.x; i < g1 - g0; i += 256) acc[i] = PLACE ? cnt[ch * G + g0 + i] : 0;
    csc_tile_walk<CH>(indptr, idx, n, ch, g0, g1, lo, hi, [&](int64_t c, int64_t k, int r) {
        const int32_t p = acc[r - g0];
        acc[r - g0] = p + 1;
        if (PLACE) {
            const int64_t at = rowptr[r] + p;
            if (at < rowptr[r + 1]) {
                rcol[at] = (int32_t)c;
                rval[at] = scale ? val[k] * scale[c] : val[k];
            }
        }
    });
    if (!PLACE)
        for (int i = threadIdx.x; i < g1 - g0; i += 256) cnt[ch * G + g0 + i] = acc[i];
}

// cnt[chunk][g] -> the row's entries in the chunks before; rowlen[g] = all of them
__global__ __launch_bounds__(256) void sp_chunk_prefix_kernel(int32_t* __restrict__ cnt, int G, int64_t nchunks,
                                                              int32_t* __restrict__ rowlen) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    int32_t run = 0;
    for (int64_t ch = 0; ch < nchunks; ++ch) {
        const int32_t t = cnt[ch * G + g];
        cnt[ch * G + g] = run;
        run += t;
    }
    rowlen[g] = run;
}

// rowptr [G + 1] and segptr [G + 1]: exclusive sums of the row lengths and of the rows' segment counts; one workgroup
__global__ __launch_bounds__(1024) void sp_row_scan_kernel(const int32_t* __restrict__ rowlen, int G,
                                                           int64_t* __restrict__ rowptr, int64_t* __restrict__ segptr) {
    __shared__ int64_t sa[1024], sb[1024];
    const int t = threadIdx.x;
    const int64_t per = ((int64_t)G + 1023) / 1024;
    const int g0 = (int)min((int64_t)G, t * per), g1 = (int)min((int64_t)G, g0 + per);
    int64_t a = 0, b = 0;
    for (int g = g0; g < g1; ++g) {
        a += rowlen[g];
        b += (rowlen[g] + SEG - 1) / SEG;
    }
    sa[t] = a;
    sb[t] = b;
    __syncthreads();
    if (t == 0) {
        int64_t ra = 0, rb = 0;
        for (int i = 0; i < 1024; ++i) {
            const int64_t ta = sa[i], tb = sb[i];
            sa[i] = ra;
            sb[i] = rb;
            ra += ta;
            rb += tb;
        }
    }
    __syncthreads();
    a = sa[t];
    b = sb[t];
    for (int g = g0; g < g1; ++g) {
        rowptr[g] = a;
        segptr[g] = b;
        a += rowlen[g];
        b += (rowlen[g] + SEG - 1) / SEG;
    }
    if (t == 1023) {  // (everything before this thread's rows and its own: the totals)
        rowptr[G] = a;
        segptr[G] = b;
    }
}

// Z[c][j] = rs[c] * sum over the PCA prefix of column c of x_gc Q[g * ldq + j]  -  off[j]      (rs, off nullable)
__global__ __launch_bounds__(256) void sp_by_cell_kernel(const int64_t* __restrict__ indptr, const int64_t* __restrict__ cut,
                                                         const int32_t* __restrict__ idx, const double* __restrict__ val,
                                                         int64_t n, const double* __restrict__ Q, int64_t ldq, int Gp,
                                                         const double* __restrict__ rs, const double* __restrict__ off,
                                                         double* __restrict__ Z) {
    const int lane = threadIdx.x & 63;
    const int64_t c = wave_uniform((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6));
    if (c >= n) return;
    const int64_t kb = wave_uniform(indptr[c]), ke = wave_uniform(cut[c]);
    const double acc = gather_rows64(idx, val, kb, ke, Q, ldq, Gp, lane);
    Z[c * 64 + lane] = (rs ? rs[c] : 1.0) * acc - (off ? off[lane] : 0.0);
}

// part[s - seg0][j] = sum over segment s of its row, in cell order, of rval Z[rcol][j], for the segments [seg0, seg0 +
// nseg) of the rows [g_lo, g_hi) (segptr[g_lo] = seg0, segptr[g_hi] = seg0 + nseg)
__global__ __launch_bounds__(256) void sp_by_gene_kernel(const int64_t* __restrict__ rowptr, const int64_t* __restrict__ segptr,
                                                         const int32_t* __restrict__ rcol, const double* __restrict__ rval,
                                                         int g_lo, int g_hi, int64_t seg0, int64_t nseg, int64_t n,
                                                         const double* __restrict__ Z, double* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int64_t s = wave_uniform((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6));
    if (s >= nseg) return;
    const int64_t sid = seg0 + s;
    int lo = g_lo, hi = g_hi;  // segptr[lo] <= sid < segptr[hi]
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (segptr[mid] <= sid) lo = mid;
        else hi = mid;
    }
    const int64_t kb = wave_uniform(rowptr[lo] + (sid - segptr[lo]) * SEG);
    const int64_t re = rowptr[lo + 1];
    const int64_t ke = wave_uniform(kb + SEG < re ? kb + SEG : re);
    part[s * 64 + lane] = gather_rows64(rcol, rval, kb, ke, Z, 64, n, lane);
}

// Y[(g - g_lo) * ldy + j] = beta Y[..] + coef * (sum of row g's segments, ascending  -  mu[g] * zsum[j]),  g in [g_lo, g_hi)
// (mu null: no rank-one term)
__global__ __launch_bounds__(256) void sp_row_reduce_kernel(const double* __restrict__ part, const int64_t* __restrict__ segptr,
                                                            int g_lo, int g_hi, int64_t seg0, double coef, double beta,
                                                            const double* __restrict__ mu, const double* __restrict__ zsum,
                                                            double* __restrict__ Y, int64_t ldy) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t g = g_lo + (e >> 6);
    const int j = (int)(e & 63);
    if (g >= g_hi) return;
    double s = 0.0;
    for (int64_t sid = segptr[g]; sid < segptr[g + 1]; ++sid) s += part[(sid - seg0) * 64 + j];
    if (mu) s -= mu[g] * zsum[j];
    const int64_t o = (g - g_lo) * ldy + j;
    Y[o] = (beta == 0.0 ? 0.0 : beta * Y[o]) + coef * s;
}

// One wave a row of the companion, lane l its entries l, l + 64, ..., the lanes added in a fixed order.
//   mu null:  out[g] = alpha * (sum of the row's values)                                    (the batch's gene means)
//   else:     out[g] = sum (value - mu[g])^2 + (n - entries) * mu[g]^2                       (the row's centred squares)
__global__ __launch_bounds__(256) void sp_row_stat_kernel(const int64_t* __restrict__ rowptr, const double* __restrict__ rval,
                                                          int G, int64_t n, double alpha, const double* __restrict__ mu,
                                                          double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= G) return;
    const int64_t kb = rowptr[g], ke = rowptr[g + 1];
    const double m = mu ? mu[g] : 0.0;
    double s = 0.0;
    for (int64_t k = kb + lane; k < ke; k += 64) {
        const double v = rval[k] - m;
        s += mu ? v * v : v;
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) out[g] = mu ? s + (double)(n - (ke - kb)) * (m * m) : alpha * s;
}

// part[block][j] = sum over the block's rows g, four strides added in a fixed order, of mu[g] * Q[g * ldq + j]
__global__ __launch_bounds__(256) void mu_dot_partial(const double* __restrict__ Q, int64_t ldq, const double* __restrict__ mu,
                                                      int64_t G, int64_t rows_per_block, double* __restrict__ part) {
    __shared__ double sm[4][64];
    const int j = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block, r1 = min(G, r0 + rows_per_block);
    double s = 0.0;
    for (int64_t r = r0 + q; r < r1; r += 4) s += mu[r] * Q[r * ldq + j];
    sm[q][j] = s;
    __syncthreads();
    if (q == 0) part[(int64_t)blockIdx.x * 64 + j] = (sm[0][j] + sm[1][j]) + (sm[2][j] + sm[3][j]);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------
struct SparsePcaBatch : CscBatch {
    DevBuf<int64_t> cut;  // [n] the end of the column's PCA prefix
    DevBuf<double> inv;   // [n] 1 / max(1e-8, l2 over the prefix), empty without cosine normalisation
    // the row-major companion, built after the last block
    DevBuf<int64_t> rowptr, segptr;  // [n_rows + 1]
    DevBuf<int32_t> rcol;            // [nnz] cells, ascending within a row
    DevBuf<double> rval;             // [nnz] scale_c x_gc
    int64_t segs_pca = 0, segs_all = 0;  // segptr[n_rows_pca], segptr[n_rows]
    double weight = 1.0;
    bool cos_norm = false;
};

class PcaSparse : ResidentBatches<SparsePcaBatch> {
  public:
    PcaSparse(int device, int n_rows, int n_rows_pca)
        : ResidentBatches(device, n_rows, "bmx_pca_sparse_begin_batch"), Gp_(n_rows_pca) {
        CacheScope scope(&cache_);
        BMX_HIP(hipMemsetAsync(flags_.reserve(CSC_F_WORDS), 0, CSC_F_WORDS * sizeof(int32_t), stream_));
        BMX_HIP(hipStreamSynchronize(stream_));
    }
    ~PcaSparse() { retire(); }

    // a batch of n cells with nnz stored entries in all; its columns arrive in one or more blocks (add_block), in order
    void begin_batch(int64_t n, double weight, bool cos_norm, int64_t nnz) {
        check_cell_count(n);
        begin_csc(n, nnz, [&](SparsePcaBatch& b) {
            b.weight = weight;
            b.cos_norm = cos_norm;
            b.cut.reserve((size_t)n);
            if (cos_norm) b.inv.reserve((size_t)n);
        });
        fitted_ = false;
    }

    // the next m cells of the batch begun last: indptr [m + 1] relative to the block, its nnz entries
    void add_block(int64_t m, const int64_t* indptr, const int32_t* indices, const double* data, int64_t nnz) {
        add_csc(m, indptr, indices, data, nnz, [&](SparsePcaBatch& b, int64_t c0) {
            hipLaunchKernelGGL(sp_prepare_kernel, dim3((unsigned)cdiv(m, 4)), dim3(256), 0, stream_,
                               (const int64_t*)b.indptr.p, (const int32_t*)b.indices.p, (const double*)b.data.p, G_, Gp_, c0, m,
                               b.cut.p, b.cos_norm ? b.inv.p : nullptr, flags_.p);
            BMX_LAUNCH_CHECK();
            fitted_ = false;
            if (b.complete()) build_rows(b);
        });
    }

    // Pca::fit over the first n_rows_pca rows: centres [n_rows_pca], rotation [n_rows_pca x d] column-major, sdev [d]
    void fit(int d, double tol, int max_applies, double* centers, double* rotation, double* sdev, int* applies_used,
             double* resid_out) {
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        fitted_ = false;
        if (batches_.empty()) throw Error(BMX_ERR_ARG, "at least one batch must be specified");
        if (!batches_.back()->complete()) throw Error(BMX_ERR_ARG, "the last batch has not received all its cells");
        int64_t ncells = 0;
        for (auto& bp : batches_) ncells += bp->n;
        const int L = SubspaceIteration::width_for(d, Gp_, ncells, max_applies);
        {
            int32_t flags[CSC_F_WORDS] = {0, 0};
            BMX_HIP(hipMemcpyAsync(flags, flags_.p, sizeof(flags), hipMemcpyDeviceToHost, stream_));
            BMX_HIP(hipStreamSynchronize(stream_));
            throw_if_bad_pattern(flags);
        }
        const int G = Gp_;
        // ---- grand centre of ALL rows: weighted mean of the batch means (R/multiBatchPCA.R:268-281)
        double* mu = mu_.reserve((size_t)G_);
        double* mean = mean_.reserve((size_t)G_);
        BMX_HIP(hipMemsetAsync(mu, 0, (size_t)G_ * sizeof(double), stream_));
        double wsum = 0.0;
        for (auto& bp : batches_) wsum += bp->weight;
        for (auto& bp : batches_) {
            SparsePcaBatch& b = *bp;
            hipLaunchKernelGGL(sp_row_stat_kernel, dim3((unsigned)cdiv(G_, 4)), dim3(256), 0, stream_,
                               (const int64_t*)b.rowptr.p, (const double*)b.rval.p, G_, b.n, 1.0 / (double)b.n,
                               (const double*)nullptr, mean);
            hipLaunchKernelGGL(axpy_kernel, dim3((unsigned)cdiv(G_, 256)), dim3(256), 0, stream_, mu, (const double*)mean,
                               b.weight / wsum, (int64_t)G_);
            BMX_LAUNCH_CHECK();
        }
        off_.reserve(4 * (size_t)PL);
        const SubspaceIteration::Outcome outcome =
            it_.run(stream_, G, d, tol, max_applies, [&](const double* Q, double* Y) { apply_operator(Q, Y); });
        // ---- results: rotation = the first d Ritz vectors; the iteration keeps them row-major for the projections' gathers
        const double* R = it_.ritz_vectors();
        double* Ut = ut_.reserve((size_t)G * L);  // [L][G]: the rotation column-major
        double* muU = off_.p + 2 * PL;
        for (int h = 0; h < L / PL; ++h) {
            hipLaunchKernelGGL(transpose64, dim3((unsigned)cdiv(G, 64)), dim3(256), 0, stream_, (const double*)(R + h * PL),
                               (int64_t)L, (int64_t)G, Ut + (size_t)h * PL * G);
            BMX_LAUNCH_CHECK();
            mu_dot(R + h * PL, muU + h * PL);  // mu . u_j for the projection's centring
        }
        if (centers) BMX_HIP(hipMemcpyAsync(centers, mu, (size_t)G * sizeof(double), hipMemcpyDeviceToHost, stream_));
        if (rotation)
            BMX_HIP(hipMemcpyAsync(rotation, Ut, (size_t)G * d * sizeof(double), hipMemcpyDeviceToHost, stream_));
        BMX_HIP(hipStreamSynchronize(stream_));
        fitted_ = true;
        it_.report(tol, outcome, sdev, applies_used, resid_out);
    }

    // crossprod(x_b - centers, rotation) over the PCA rows: [n_b x d] column-major
    void project(int b, double* out) {
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        if (!fitted_) throw Error(BMX_ERR_ARG, "bmx_pca_sparse_fit has not been run");
        if (b < 0 || b >= (int)batches_.size()) throw Error(BMX_ERR_ARG, "batch index out of range");
        if (!out) throw Error(BMX_ERR_ARG, "null output pointer");
        SparsePcaBatch& B = *batches_[(size_t)b];
        double* Z = z_.reserve((size_t)B.n * PL);
        double* Zt = zt_.reserve((size_t)B.n * PL);
        const int d = it_.d();
        for (int h = 0; h * PL < d; ++h) {
            by_cell(B, it_.ritz_vectors() + h * PL, mu_dot_u() + h * PL, Z);
            hipLaunchKernelGGL(transpose64, dim3((unsigned)cdiv(B.n, 64)), dim3(256), 0, stream_, (const double*)Z, (int64_t)PL,
                               B.n, Zt);
            BMX_LAUNCH_CHECK();
            const int cols = std::min(PL, d - h * PL);
            BMX_HIP(hipMemcpyAsync(out + (size_t)h * PL * B.n, Zt, (size_t)B.n * cols * sizeof(double), hipMemcpyDeviceToHost,
                                   stream_));
            BMX_HIP(hipStreamSynchronize(stream_));  // Z / Zt are reused by the next half
        }
    }

    // the rows outside the subset: centers_left [n_rows - n_rows_pca], rotation_left [.. x d] column-major (nullable):
    //   ( sum_b coef_b sum_c scale_c x_gc pcs_b[c][j]  -  center[g] sum_b coef_b sum_c pcs_b[c][j] ) / sdev[j]^2
    void genes(double* centers_left, double* rotation_left) {
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        if (!fitted_) throw Error(BMX_ERR_ARG, "bmx_pca_sparse_fit has not been run");
        const int GL = G_ - Gp_, d = it_.d(), nh = cdiv(d, PL);
        if (GL < 1) return;
        double* acc = acc_.reserve((size_t)nh * GL * PL);
        double* tsum = tsum_.reserve((size_t)nh * PL + 2 * (size_t)PL);
        BMX_HIP(hipMemsetAsync(acc, 0, (size_t)nh * GL * PL * sizeof(double), stream_));
        BMX_HIP(hipMemsetAsync(tsum, 0, (size_t)nh * PL * sizeof(double), stream_));
        for (auto& bp : batches_) {
            SparsePcaBatch& B = *bp;
            const double coef = B.weight / (double)B.n;
            double* Z = z_.reserve((size_t)B.n * PL);
            for (int h = 0; h < nh; ++h) {
                by_cell(B, it_.ritz_vectors() + h * PL, mu_dot_u() + h * PL, Z);
                column_sums(Z, B.n, coef, 1.0, tsum + h * PL);
                by_gene(B, Gp_, G_, Z, coef, 1.0, nullptr, nullptr, acc + (size_t)h * GL * PL, PL);
            }
        }
        double* rot = part_.reserve((size_t)GL * d);
        leftover_rotation(stream_, it_.theta(), d, acc, mu_.p + Gp_, tsum, tsum + (size_t)nh * PL, GL, rot, centers_left,
                          rotation_left);
    }

    // sum_b coef_b |C_b|_F^2 over the PCA rows, per gene in the centred form; the caller divides by the batches
    void total_variance(double* var_total) {
        if (!var_total) throw Error(BMX_ERR_ARG, "null output pointer");
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        if (!fitted_) throw Error(BMX_ERR_ARG, "bmx_pca_sparse_fit has not been run");
        double total = 0.0;
        std::vector<double> h((size_t)Gp_);
        double* per = mean_.reserve((size_t)G_);
        for (auto& bp : batches_) {
            SparsePcaBatch& B = *bp;
            hipLaunchKernelGGL(sp_row_stat_kernel, dim3((unsigned)cdiv(Gp_, 4)), dim3(256), 0, stream_,
                               (const int64_t*)B.rowptr.p, (const double*)B.rval.p, Gp_, B.n, 1.0, (const double*)mu_.p, per);
            BMX_LAUNCH_CHECK();
            BMX_HIP(hipMemcpyAsync(h.data(), per, h.size() * sizeof(double), hipMemcpyDeviceToHost, stream_));
            BMX_HIP(hipStreamSynchronize(stream_));
            double s = 0.0;
            for (double v : h) s += v;
            total += (B.weight / (double)B.n) * s;
        }
        *var_total = total;
    }

  private:
    // the row-major companion of a batch that has all its cells (file head)
    void build_rows(SparsePcaBatch& b) {
        const int G = G_;
        const int64_t nchunks = (b.n + CH - 1) / CH;
        const size_t nz = (size_t)std::max<int64_t>(b.nnz, 1);
        b.rowptr.reserve((size_t)G + 1);
        b.segptr.reserve((size_t)G + 1);
        b.rcol.reserve(nz);
        b.rval.reserve(nz);
        int32_t* cnt = cnt_.reserve((size_t)nchunks * G + (size_t)G);
        int32_t* rowlen = cnt + (size_t)nchunks * G;
        // (a slot that a pattern with repeated rows leaves unwritten holds cell 0 and value 0)
        BMX_HIP(hipMemsetAsync(b.rcol.p, 0, nz * sizeof(int32_t), stream_));
        BMX_HIP(hipMemsetAsync(b.rval.p, 0, nz * sizeof(double), stream_));
        const int gtiles = cdiv(G, GT);
        // (a batch holds fewer than 2^31 cells: at most 2^24 chunks, one launch)
        hipLaunchKernelGGL(sp_sort_kernel<false>, dim3((unsigned)nchunks, (unsigned)gtiles), dim3(256), 0, stream_,
                           (const int64_t*)b.indptr.p, (const int32_t*)b.indices.p, (const double*)b.data.p, G, b.n, cnt,
                           (const int64_t*)nullptr, (const double*)nullptr, (int32_t*)nullptr, (double*)nullptr);
        BMX_LAUNCH_CHECK();
        hipLaunchKernelGGL(sp_chunk_prefix_kernel, dim3((unsigned)cdiv(G, 256)), dim3(256), 0, stream_, cnt, G, nchunks, rowlen);
        hipLaunchKernelGGL(sp_row_scan_kernel, dim3(1), dim3(1024), 0, stream_, (const int32_t*)rowlen, G, b.rowptr.p,
                           b.segptr.p);
        BMX_LAUNCH_CHECK();
        hipLaunchKernelGGL(sp_sort_kernel<true>, dim3((unsigned)nchunks, (unsigned)gtiles), dim3(256), 0, stream_,
                           (const int64_t*)b.indptr.p, (const int32_t*)b.indices.p, (const double*)b.data.p, G, b.n, cnt,
                           (const int64_t*)b.rowptr.p, (const double*)(b.cos_norm ? b.inv.p : nullptr), b.rcol.p, b.rval.p);
        BMX_LAUNCH_CHECK();
        int64_t segs[2] = {0, 0};
        BMX_HIP(hipMemcpyAsync(&segs[0], b.segptr.p + Gp_, sizeof(int64_t), hipMemcpyDeviceToHost, stream_));
        BMX_HIP(hipMemcpyAsync(&segs[1], b.segptr.p + G, sizeof(int64_t), hipMemcpyDeviceToHost, stream_));
        BMX_HIP(hipStreamSynchronize(stream_));
        b.segs_pca = segs[0];
        b.segs_all = segs[1];
    }

    // Z [n][64] = diag(scale) x_S^T Q - 1 off^T for 64 columns of a row-major [n_rows_pca][L_] block at Q
    void by_cell(SparsePcaBatch& b, const double* Q, const double* off, double* Z) {
        hipLaunchKernelGGL(sp_by_cell_kernel, dim3((unsigned)cdiv(b.n, 4)), dim3(256), 0, stream_, (const int64_t*)b.indptr.p,
                           (const int64_t*)b.cut.p, (const int32_t*)b.indices.p, (const double*)b.data.p, b.n, Q, (int64_t)it_.L(),
                           Gp_, (const double*)(b.cos_norm ? b.inv.p : nullptr), off, Z);
        BMX_LAUNCH_CHECK();
    }
    // Y [(g_hi - g_lo)][ldy] = beta Y + coef (x diag(scale) Z - mu 1^T Z) over the rows [g_lo, g_hi), g_lo in {0, Gp_}
    void by_gene(SparsePcaBatch& b, int g_lo, int g_hi, const double* Z, double coef, double beta, const double* mu,
                 const double* zsum, double* Y, int64_t ldy) {
        const int64_t seg0 = g_lo == 0 ? 0 : b.segs_pca;
        const int64_t nseg = (g_hi == Gp_ ? b.segs_pca : b.segs_all) - seg0;
        double* part = seg_part_.reserve((size_t)std::max<int64_t>(nseg, 1) * PL);
        if (nseg > 0) {
            hipLaunchKernelGGL(sp_by_gene_kernel, dim3((unsigned)cdiv(nseg, 4)), dim3(256), 0, stream_,
                               (const int64_t*)b.rowptr.p, (const int64_t*)b.segptr.p, (const int32_t*)b.rcol.p,
                               (const double*)b.rval.p, g_lo, g_hi, seg0, nseg, b.n, Z, part);
            BMX_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(sp_row_reduce_kernel, dim3((unsigned)cdiv((int64_t)(g_hi - g_lo) * PL, 256)), dim3(256), 0, stream_,
                           (const double*)part, (const int64_t*)b.segptr.p, g_lo, g_hi, seg0, coef, beta, mu, zsum, Y, ldy);
        BMX_LAUNCH_CHECK();
    }
    // out[j] = beta out[j] + alpha * sum_c Z[c][j], two stages in a fixed order
    void column_sums(const double* Z, int64_t n, double alpha, double beta, double* out) {
        column_sums64(stream_, Z, n, zpart_.reserve((size_t)4096 * PL), alpha, beta, out);
    }
    // out[j] = mu . Q[:, j] for 64 columns of a row-major [n_rows_pca][L_] block at Q
    void mu_dot(const double* Q, double* out) {
        const int nb = (int)std::min<int64_t>(1024, std::max<int64_t>(1, Gp_ / 256));
        const int64_t rpb = ((int64_t)Gp_ + nb - 1) / nb;
        double* zpart = zpart_.reserve((size_t)4096 * PL);
        hipLaunchKernelGGL(mu_dot_partial, dim3(nb), dim3(256), 0, stream_, Q, (int64_t)it_.L(), (const double*)mu_.p, (int64_t)Gp_,
                           rpb, zpart);
        hipLaunchKernelGGL(reduce_parts, dim3(1), dim3(64), 0, stream_, (const double*)zpart, nb, (int64_t)PL, 1.0, 0.0, out, PL,
                           (int64_t)PL);
        BMX_LAUNCH_CHECK();
    }
    // Y = M Q = sum_b (w_b / n_b) C_b C_b^T Q for a block of L vectors, 64 at a time
    void apply_operator(const double* Q, double* Y) {
        const int G = Gp_, L = it_.L();
        BMX_HIP(hipMemsetAsync(Y, 0, (size_t)G * L * sizeof(double), stream_));
        double* muQ = off_.p;
        double* zsum = off_.p + PL;
        for (int h = 0; h < L / PL; ++h) {
            mu_dot(Q + h * PL, muQ);
            for (auto& bp : batches_) {
                SparsePcaBatch& b = *bp;
                double* Z = z_.reserve((size_t)b.n * PL);
                by_cell(b, Q + h * PL, muQ, Z);
                column_sums(Z, b.n, 1.0, 0.0, zsum);
                by_gene(b, 0, G, Z, b.weight / (double)b.n, 1.0, mu_.p, zsum, Y + h * PL, (int64_t)L);
            }
        }
    }
    const double* mu_dot_u() const { return off_.p + 2 * PL; }  // [L]: mu . u_j of the last fit

    int Gp_;  // the rows the PCA runs on: the first Gp_ of the G_ resident rows
    SubspaceIteration it_;
    // off_: mu . Q of the block being applied [PL], the column sums of Z [PL], mu . u_j [2 PL]
    DevBuf<double> mu_, mean_, ut_, z_, zt_, part_, seg_part_, zpart_, off_, acc_, tsum_;
    DevBuf<int32_t> cnt_, flags_;
    bool fitted_ = false;
};

}  // namespace bmx

/* ---------------------------------------------------------------- bmx_pca_sparse_* ------------------------------ */
struct bmx_pca_sparse final : bmx::PcaSparse {
    using PcaSparse::PcaSparse;
};

extern "C" {

int32_t bmx_pca_sparse_create(int32_t device, int32_t n_rows, int32_t n_rows_pca, bmx_pca_sparse_t** out) {
    return bmx::guarded([&] {
        if (!out) throw bmx::Error(BMX_ERR_ARG, "null output pointer");
        if (n_rows < 1) throw bmx::Error(BMX_ERR_ARG, "the PCA needs at least one gene");
        if (n_rows_pca < 1 || n_rows_pca > n_rows)
            throw bmx::Error(BMX_ERR_ARG, "the PCA rows are the first 1 <= n_rows_pca <= n_rows rows");
        *out = new bmx_pca_sparse(device, n_rows, n_rows_pca);
    });
}

void bmx_pca_sparse_destroy(bmx_pca_sparse_t* h) { delete h; }

int32_t bmx_pca_sparse_check_block(int64_t n, int64_t filled, int64_t n_block, const int64_t* indptr, const int32_t* indices,
                                   const double* data, int64_t nnz) {
    return bmx::guarded([&] { bmx::check_csc_block(n, filled, n_block, indptr, indices, data, nnz); });
}

int32_t bmx_pca_sparse_begin_batch(bmx_pca_sparse_t* h, int64_t n, double weight, int32_t cos_norm, int64_t nnz) {
    return bmx::guarded([&] { bmx::live(h).begin_batch(n, weight, cos_norm != 0, nnz); });
}

int32_t bmx_pca_sparse_add_block(bmx_pca_sparse_t* h, int64_t n_block, const int64_t* indptr, const int32_t* indices,
                                 const double* data, int64_t nnz) {
    return bmx::guarded([&] { bmx::live(h).add_block(n_block, indptr, indices, data, nnz); });
}

int32_t bmx_pca_sparse_fit(bmx_pca_sparse_t* h, int32_t d, int32_t iters, double* centers, double* rotation, double* sdev) {
    return bmx::guarded([&] { bmx::live(h).fit(d, 0.0, iters, centers, rotation, sdev, nullptr, nullptr); });
}

int32_t bmx_pca_sparse_fit_tol(bmx_pca_sparse_t* h, int32_t d, double tol, int32_t max_iters, double* centers,
                               double* rotation, double* sdev, int32_t* iters_used, double* residual) {
    return bmx::guarded([&] {
        bmx::fit_to_tolerance(bmx::live(h), d, tol, max_iters, centers, rotation, sdev, iters_used, residual);
    });
}

int32_t bmx_pca_sparse_project(bmx_pca_sparse_t* h, int32_t batch, double* out) {
    return bmx::guarded([&] { bmx::live(h).project(batch, out); });
}

int32_t bmx_pca_sparse_genes(bmx_pca_sparse_t* h, double* centers_left, double* rotation_left) {
    return bmx::guarded([&] { bmx::live(h).genes(centers_left, rotation_left); });
}

int32_t bmx_pca_sparse_total_variance(bmx_pca_sparse_t* h, double* var_total) {
    return bmx::guarded([&] { bmx::live(h).total_variance(var_total); });
}

}  // extern "C"
