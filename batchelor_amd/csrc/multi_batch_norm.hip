// multiBatchNorm() (R/multiBatchNorm.R:100-280, with scuttle's librarySizeFactors / calculateAverage / logNormCounts as
// include/batchelor_mi355x.h defines them) on the device: genes x cells FP64 counts in R's layout, uploaded once (whole or
// in column blocks) and kept in HBM.  S: the statistic rows (all rows, or the list given to bmx_norm_create).
//   upload  behind the copy of the next block, on a second stream:
//             colsum_kernel        one wave a cell: its sum over S (the library size) in a fixed lane order, and the
//                                  device flag for a negative or non-finite count
//             gene_partial_kernel  lanes along the genes of S, cells cut into chunks of NCH at fixed positions:
//                                  part[chunk][g] = sum of x[g, c] / w[c], w = the library sizes (or the size factors
//                                  given).  A chunk is summed once all its cells are resident.
//   stats   finalize_kernel  mean(w) in a fixed order, sf = w / mean(w), the flag for a size factor that is not positive
//           ave_kernel       ave[g] = (chunk sums) * (mean(w) / n)  [= (1/n) sum x / sf]
//   ratios  ratio_kernel     one workgroup per unordered pair: both sums, the keep rule, both medians by an exact radix
//                            selection on the bit patterns of the (non-negative) ratios; smallest_kernel: the diagonal,
//                            the reference batch and the rescaling; sfout_kernel: sf / rescaling
//   output  norm_out_kernel  log2(x / sf_out + pseudo) (or x / sf_out), in blocks through two device buffers that
//                            download behind the kernels (blocked_output)
// The orders of the sums are those of ordered_sums.hpp.  FP64 vector arithmetic, contraction off.
//
// Sparse counts (NormSparse, bmx_norm_sparse_*): a batch stays in HBM as CSC -- indptr [n + 1] int64 absolute, indices
// int32, data FP64 -- filled in column blocks through the same staging ring.  The reductions and the output pass have
// sparse forms, everything between them is shared with the dense handle:
//   sp_colsum_kernel        one wave a cell over its stored entries; also the flags for a bad count, a row outside
//                           [0, G) and rows that do not ascend strictly within a column
//   sp_gene_partial_kernel  one workgroup per (chunk, tile of GT genes), the tile's sums in the LDS: the chunk's columns
//                           in ascending order, one addition per stored entry, a barrier between columns.  A gene's sum
//                           has one accumulator and takes its terms in cell order, as gene_partial_kernel's does; the
//                           terms left out are x / w = +0, which change no bit of a sum of non-negative terms.
//   sp_out_kernel           one wave a column over the stored entries only; zero_image_kernel: what a zero becomes
// Every entry position comes from an indptr the host has checked (check_csc_block); a row index is compared
// with its bounds before it addresses anything, and an entry that fails is skipped.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "bmx_ops.hpp"
#include "csc_device.hpp"
#include "host_xfer.hpp"
#include "ordered_sums.hpp"
#include "resident_batches.hpp"

namespace bmx {
namespace {

constexpr int NCH = 256;   // cells per chunk of the per-gene sums
constexpr int CPW = 16;    // cells per workgroup in the output pass
constexpr int RT = 1024;   // threads of a pair's workgroup in the ratio stage
constexpr int MAX_GENES = 65535 * 256;
constexpr size_t OUT_BLOCK_BYTES = (size_t)64 << 20;
constexpr double DBL_LARGEST = 1.7976931348623157e308;
// flags (device): a count that is negative or not finite, a size factor that is not positive, a pair without a finite
// median ratio; [3]: the reference batch (0-based)
enum { F_COUNT = 0, F_SF = 1, F_RATIO = 2, F_SMALLEST = 3, F_WORDS = 4 };
// the sparse handle's further words: the pattern pair (CSC_F_ROW, CSC_F_ORDER)
enum { F_PATTERN = 4, F_SPARSE_WORDS = F_PATTERN + CSC_F_WORDS };
constexpr int GT = 4096;  // genes per tile of the sparse per-gene sums (32 KiB of accumulators in the LDS)

__device__ __forceinline__ int invalid_count(double v) { return !(v >= 0.0 && v <= DBL_LARGEST); }

// w[c] = sum over the statistic rows of x[g, c], cells [c0, c0 + m) of the batch at x; one wave a cell, lane l adds rows
// l, l + 64, ... (MODE 1: the row pairs l, l + 64, ..., 16-byte loads, G even; MODE 2: every row times mult[g], how often
// the row is named), then the lanes are added in a fixed order.  w null: the counts are checked only.
template <int MODE>
__global__ __launch_bounds__(256) void colsum_kernel(const double* __restrict__ x, int G, int64_t c0, int64_t m,
                                                     const double* __restrict__ mult, double* __restrict__ w,
                                                     int32_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int64_t c = c0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= c0 + m) return;  // (a whole wave leaves)
    const double* col = x + c * G;
    double sa = 0.0, sb = 0.0;
    int bad = 0;
    if (MODE == 1) {
        const double2* col2 = reinterpret_cast<const double2*>(col);
        const int n2 = G / 2;
        int i = lane;
        for (; i + 192 < n2; i += 256) {  // four 16-byte loads in flight
            const double2 v0 = col2[i], v1 = col2[i + 64], v2 = col2[i + 128], v3 = col2[i + 192];
            bad |= invalid_count(v0.x) | invalid_count(v0.y) | invalid_count(v1.x) | invalid_count(v1.y);
            bad |= invalid_count(v2.x) | invalid_count(v2.y) | invalid_count(v3.x) | invalid_count(v3.y);
            sa += v0.x;
            sb += v0.y;
            sa += v1.x;
            sb += v1.y;
            sa += v2.x;
            sb += v2.y;
            sa += v3.x;
            sb += v3.y;
        }
        for (; i < n2; i += 64) {
            const double2 v = col2[i];
            bad |= invalid_count(v.x) | invalid_count(v.y);
            sa += v.x;
            sb += v.y;
        }
    } else {
        int i = lane;
        for (; i + 192 < G; i += 256) {
            double v0 = col[i], v1 = col[i + 64], v2 = col[i + 128], v3 = col[i + 192];
            bad |= invalid_count(v0) | invalid_count(v1) | invalid_count(v2) | invalid_count(v3);
            if (MODE == 2) {
                v0 *= mult[i];
                v1 *= mult[i + 64];
                v2 *= mult[i + 128];
                v3 *= mult[i + 192];
            }
            sa += v0;
            sb += v1;
            sa += v2;
            sb += v3;
        }
        for (; i < G; i += 64) {
            double v = col[i];
            bad |= invalid_count(v);
            if (MODE == 2) v *= mult[i];
            sa += v;
        }
    }
    double s = sa + sb;
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    if (bad) flags[F_COUNT] = 1;
    if (lane == 0 && w) w[c] = s;
}

// part[ch][g] = sum over the cells [ch * NCH, min(n, (ch + 1) * NCH)), in order, of x[rows[g], cell] / w[cell], g in
// [0, nS) (rows null: the rows themselves).  V2: two genes a thread, 16-byte loads (rows null, G = nS even).
template <bool V2>
__global__ __launch_bounds__(256) void gene_partial_kernel(const double* __restrict__ x, int G,
                                                           const int32_t* __restrict__ rows, int nS,
                                                           const double* __restrict__ w, int64_t n, int ch0,
                                                           double* __restrict__ part) {
    const int t = blockIdx.y * 256 + threadIdx.x;
    if (t >= (V2 ? nS / 2 : nS)) return;
    const int ch = ch0 + blockIdx.x;
    const int64_t b = (int64_t)ch * NCH;
    const int64_t e = b + NCH < n ? b + NCH : n;
    if (V2) {
        const double2* x2 = reinterpret_cast<const double2*>(x);
        const int64_t G2 = G / 2;
        double s0 = 0.0, s1 = 0.0;
        struct Term {
            double2 v;
            double w;
        };
        ordered_walk4(
            b, e, [&](int64_t i) { return Term{x2[i * G2 + t], w[i]}; },
            [&](const Term& q) {
                s0 += q.v.x / q.w;
                s1 += q.v.y / q.w;
            });
        reinterpret_cast<double2*>(part)[(int64_t)ch * (nS / 2) + t] = make_double2(s0, s1);
    } else {
        const int64_t r = rows ? rows[t] : t;
        double s = 0.0;
        struct Term {
            double v, w;
        };
        ordered_walk4(
            b, e, [&](int64_t i) { return Term{x[i * G + r], w[i]}; }, [&](const Term& q) { s += q.v / q.w; });
        part[(int64_t)ch * nS + t] = s;
    }
}

// the sum of a[0, n) by the workgroup's T threads: thread t adds a[t], a[t + T], ..., then a tree over the threads
template <int T>
__device__ double block_sum(const double* __restrict__ a, int64_t n, double* red) {
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += T) s += a[i];
    return block_tree_sum<T>(s, red);
}

// one workgroup a batch: sf = w / mean(w), scale[0] = mean(w) / n
__global__ __launch_bounds__(256) void finalize_kernel(const double* __restrict__ w, int64_t n, double* __restrict__ sf,
                                                       double* __restrict__ scale, int32_t* __restrict__ flags) {
    __shared__ double red[256];
    const double mean = block_sum<256>(w, n, red) / (double)n;
    bool bad = false;
    for (int64_t c = threadIdx.x; c < n; c += 256) {
        const double v = w[c] / mean;
        bad |= !(v > 0.0 && v <= DBL_LARGEST);
        sf[c] = v;
    }
    if (bad) flags[F_SF] = 1;
    if (threadIdx.x == 0) scale[0] = mean / (double)n;
}

// ave[g] = (sum of the chunk sums, ascending chunk) * scale[0]
__global__ __launch_bounds__(256) void ave_kernel(const double* __restrict__ part, int nS, int nchunks,
                                                  const double* __restrict__ scale, double* __restrict__ ave) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= nS) return;
    const auto at = [&](int ch) { return part[(int64_t)ch * nS + g]; };
    ave[g] = fold_ascending(at(0), 1, nchunks, at) * scale[0];
}

// .rescale_size_factors' filter (R/multiBatchNorm.R:253-254), in R's order of evaluation
__device__ __forceinline__ bool kept_gene(double af, double as, double fs, double ss, double min_mean) {
    const double grand = (af / fs + as / ss) / 2 * (fs + ss) / 2;
    return grand >= min_mean;
}

// The bit pattern of the rank-th smallest (0-based) of the kept genes' ratios, as / af (s_over_f) or af / as: eight
// passes of a 256-bin histogram over the patterns that agree with the digits found so far.  The patterns of non-negative
// doubles (+inf included) order as the values do.
__device__ unsigned long long select_ratio(const double* __restrict__ af, const double* __restrict__ as, int n, double fs,
                                           double ss, double min_mean, bool s_over_f, int rank, int* hist,
                                           unsigned long long* sel) {
    unsigned long long prefix = 0, mask = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        if (threadIdx.x < 256) hist[threadIdx.x] = 0;
        __syncthreads();
        for (int g = threadIdx.x; g < n; g += RT) {
            const double a = af[g], b = as[g];
            if (!kept_gene(a, b, fs, ss, min_mean)) continue;
            const unsigned long long key = (unsigned long long)__double_as_longlong(s_over_f ? b / a : a / b);
            if ((key & mask) == prefix) atomicAdd(&hist[(int)((key >> shift) & 255)], 1);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int cum = 0, bin = 0;
            for (; bin < 255; ++bin) {
                if (cum + hist[bin] > rank) break;
                cum += hist[bin];
            }
            sel[0] = prefix | ((unsigned long long)bin << shift);
            sel[1] = (unsigned long long)(rank - cum);
        }
        __syncthreads();
        prefix = sel[0];
        rank = (int)sel[1];
        mask |= 0xffull << shift;
    }
    return prefix;
}

__device__ double median_ratio(const double* af, const double* as, int n, double fs, double ss, double min_mean,
                               bool s_over_f, int kept, int* hist, unsigned long long* sel) {
    const double hi = __longlong_as_double((long long)select_ratio(af, as, n, fs, ss, min_mean, s_over_f, kept / 2, hist, sel));
    if (kept & 1) return hi;
    const double lo =
        __longlong_as_double((long long)select_ratio(af, as, n, fs, ss, min_mean, s_over_f, kept / 2 - 1, hist, sel));
    return (lo + hi) / 2;
}

// Workgroup p: the p-th pair first < second in R's loop order.  ratios [B][B] row-major: ratios[first][second] =
// median(ave_second / ave_first), ratios[second][first] = median(ave_first / ave_second) over the kept genes.
__global__ __launch_bounds__(RT) void ratio_kernel(const double* __restrict__ ave, int nS, int B, double min_mean,
                                                   double* __restrict__ ratios, int32_t* __restrict__ flags) {
    __shared__ double red[RT];
    __shared__ int hist[256];
    __shared__ unsigned long long sel[2];
    int first = 0, p = blockIdx.x;
    while (p >= B - 1 - first) {
        p -= B - 1 - first;
        ++first;
    }
    const int second = first + 1 + p;
    const double* af = ave + (int64_t)first * nS;
    const double* as = ave + (int64_t)second * nS;
    const double fs = block_sum<RT>(af, nS, red);
    const double ss = block_sum<RT>(as, nS, red);
    if (threadIdx.x < 2) hist[threadIdx.x] = 0;
    __syncthreads();
    int mine = 0, nan = 0;
    for (int g = threadIdx.x; g < nS; g += RT) {
        const double a = af[g], b = as[g];
        if (!kept_gene(a, b, fs, ss, min_mean)) continue;
        ++mine;
        const double r = b / a;  // (a / b is NaN exactly when b / a is: 0 / 0 or inf / inf)
        nan |= r != r;
    }
    if (mine) atomicAdd(&hist[0], mine);
    if (nan) atomicAdd(&hist[1], 1);
    __syncthreads();
    const int kept = hist[0];
    const bool any_nan = hist[1] != 0;
    __syncthreads();
    if (kept == 0 || any_nan) {
        if (threadIdx.x == 0) flags[F_RATIO] = 1;
        return;
    }
    const double r1 = median_ratio(af, as, nS, fs, ss, min_mean, true, kept, hist, sel);
    const double r2 = median_ratio(af, as, nS, fs, ss, min_mean, false, kept, hist, sel);
    if (threadIdx.x == 0) {
        ratios[(int64_t)first * B + second] = r1;
        ratios[(int64_t)second * B + first] = r2;
        if (!(r1 > 0.0 && r1 <= DBL_LARGEST) || !(r2 > 0.0 && r2 <= DBL_LARGEST)) flags[F_RATIO] = 1;
    }
}

// the diagonal, smallest = the first column with the smallest minimum (NaN skipped, as min(na.rm=TRUE)), rescaling =
// that column.  One thread: B is the number of batches.
__global__ void smallest_kernel(double* __restrict__ ratios, int B, double* __restrict__ rescaling,
                                int32_t* __restrict__ flags) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int i = 0; i < B; ++i) ratios[(int64_t)i * B + i] = 1.0;
    int best = 0;
    double best_min = 0.0;
    for (int j = 0; j < B; ++j) {
        double m = 1.0;  // (the diagonal)
        for (int i = 0; i < B; ++i) {
            const double v = ratios[(int64_t)i * B + j];
            if (v < m) m = v;
        }
        if (j == 0 || m < best_min) {
            best = j;
            best_min = m;
        }
    }
    for (int i = 0; i < B; ++i) rescaling[i] = ratios[(int64_t)i * B + best];
    flags[F_SMALLEST] = best;
}

__global__ __launch_bounds__(256) void sfout_kernel(const double* __restrict__ sf, int64_t n,
                                                    const double* __restrict__ rescaling, double* __restrict__ sfo) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < n) sfo[c] = sf[c] / rescaling[0];
}

// out[g, c] = log2(x[g, c] / sfo[c] + pseudo) (LOG) or x[g, c] / sfo[c], cells [0, mb) of the block at x / sfo / out.
// V2: two genes a thread, 16-byte loads and stores (G even).
template <bool V2, bool LOG>
__global__ __launch_bounds__(256) void norm_out_kernel(const double* __restrict__ x, int G, int mb,
                                                       const double* __restrict__ sfo, double pseudo,
                                                       double* __restrict__ out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= (V2 ? G / 2 : G)) return;
    const int c0 = blockIdx.y * CPW, c1 = min(mb, c0 + CPW);
    for (int c = c0; c < c1; ++c) {
        const double so = sfo[c];
        if (V2) {
            const int64_t at = (int64_t)c * (G / 2) + t;
            const double2 v = reinterpret_cast<const double2*>(x)[at];
            const double a = v.x / so, b = v.y / so;
            reinterpret_cast<double2*>(out)[at] = LOG ? make_double2(log2(a + pseudo), log2(b + pseudo)) : make_double2(a, b);
        } else {
            const int64_t at = (int64_t)c * G + t;
            const double a = x[at] / so;
            out[at] = LOG ? log2(a + pseudo) : a;
        }
    }
}

// ---- sparse counts: a batch as CSC, indptr [n + 1] absolute positions into idx / val.  indptr has been checked on the
// host (non-decreasing, within the arrays), idx and val have not.

// The library sizes of the cells [c0, c0 + m), one wave a cell: lane l adds the column's entries l, l + 64, ..., then
// the lanes are added in a fixed order.  mult (nullable): every value times mult[row].  w null: the entries are checked
// only.  The pattern flags (csc_entry_flags) go to flags + F_PATTERN; an entry whose row is outside [0, G) is left out.
__global__ __launch_bounds__(256) void sp_colsum_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                        const double* __restrict__ val, int G, int64_t c0, int64_t m,
                                                        const double* __restrict__ mult, double* __restrict__ w,
                                                        int32_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int64_t c = c0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= c0 + m) return;  // (a whole wave leaves)
    const int64_t kb = indptr[c], ke = indptr[c + 1];
    double s = 0.0;
    int bad = 0, bad_row = 0, bad_order = 0;
    for (int64_t k = kb + lane; k < ke; k += 64) {
        const int32_t r = idx[k];
        double v = val[k];
        bad |= invalid_count(v);
        if (csc_entry_flags(idx, k, kb, r, G, bad_row, bad_order)) continue;
        if (mult) v *= mult[r];
        s += v;
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    if (bad) flags[F_COUNT] = 1;
    if (bad_row) flags[F_PATTERN + CSC_F_ROW] = 1;
    if (bad_order) flags[F_PATTERN + CSC_F_ORDER] = 1;
    if (lane == 0 && w) w[c] = s;
}

// part[ch][g] = sum over the cells [ch * NCH, min(n, (ch + 1) * NCH)), in order, of x[g, cell] / w[cell] for the genes g
// of tile blockIdx.y, all G rows (part is [nchunks][G]), by csc_tile_walk: no two threads meet at an accumulator (on a
// column that is not canonical they may, CSC_F_ORDER has been raised for it, and the addresses stay inside the tile).
__global__ __launch_bounds__(256) void sp_gene_partial_kernel(const int64_t* __restrict__ indptr,
                                                              const int32_t* __restrict__ idx,
                                                              const double* __restrict__ val, int G,
                                                              const double* __restrict__ w, int64_t n, int ch0,
                                                              double* __restrict__ part) {
    __shared__ double acc[GT];
    __shared__ int64_t lo[NCH], hi[NCH];
    const int ch = ch0 + blockIdx.x;
    const int g0 = blockIdx.y * GT, g1 = min(G, g0 + GT);
    for (int i = threadIdx.x; i < g1 - g0; i += 256) acc[i] = 0.0;
    double wc = 0.0;
    csc_tile_walk<NCH>(
        indptr, idx, n, ch, g0, g1, lo, hi, [&](int64_t c) { wc = w[c]; },
        [&](int64_t, int64_t k, int r) { acc[r - g0] += val[k] / wc; });
    for (int i = threadIdx.x; i < g1 - g0; i += 256) part[(int64_t)ch * G + g0 + i] = acc[i];
}

// ave[g] = (sum over the chunks, ascending, of part[chunk][rows[g]]) * scale[0], part [nchunks][G]: ave_kernel for sums
// kept by row
__global__ __launch_bounds__(256) void ave_rows_kernel(const double* __restrict__ part, int G,
                                                       const int32_t* __restrict__ rows, int nS, int nchunks,
                                                       const double* __restrict__ scale, double* __restrict__ ave) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= nS) return;
    const int r = rows[g];
    const auto at = [&](int ch) { return part[(int64_t)ch * G + r]; };
    ave[g] = fold_ascending(at(0), 1, nchunks, at) * scale[0];
}

// out[k - k0] = log2(val[k] / sfo[c] + pseudo) (LOG) or val[k] / sfo[c] for the stored entries k of the cells c in
// [c0, c0 + mb), k0 = indptr[c0]; one wave a cell
template <bool LOG>
__global__ __launch_bounds__(256) void sp_out_kernel(const int64_t* __restrict__ indptr, const double* __restrict__ val,
                                                     int64_t c0, int mb, const double* __restrict__ sfo, double pseudo,
                                                     double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t c = c0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= c0 + mb) return;
    const int64_t k0 = indptr[c0], ke = indptr[c + 1];
    const double so = sfo[c];
    for (int64_t k = indptr[c] + lane; k < ke; k += 64) {
        const double a = val[k] / so;
        out[k - k0] = LOG ? log2(a + pseudo) : a;
    }
}

// what norm_out_kernel makes of a count of zero (its quotient by any size factor is +0), by the same log2
template <bool LOG>
__global__ void zero_image_kernel(double pseudo, double* __restrict__ zero) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double a = 0.0 / 1.0;
    zero[0] = LOG ? log2(a + pseudo) : a;
}

}  // namespace

// argument checks of the handles' constructors / begin_batch / run without a device (throw Error(BMX_ERR_ARG))
void norm_check_create(int G, const int32_t* stat_rows, int64_t n_stat) {
    if (G < 1) throw Error(BMX_ERR_ARG, "multiBatchNorm needs at least one gene");
    if (G > MAX_GENES) throw Error(BMX_ERR_ARG, "at most 16 776 960 genes");
    if (!stat_rows || n_stat < 0) return;
    if (n_stat == 0) throw Error(BMX_ERR_ARG, "the statistic rows select no genes");
    if (n_stat > MAX_GENES) throw Error(BMX_ERR_ARG, "at most 16 776 960 statistic rows");
    for (int64_t i = 0; i < n_stat; ++i)
        if (stat_rows[i] < 1 || stat_rows[i] > G) throw Error(BMX_ERR_ARG, "subset indices out of range");
}

void norm_check_batch(int64_t n, const double* size_factors) {
    check_cell_count(n);
    if (!size_factors) return;
    for (int64_t i = 0; i < n; ++i)
        if (!(size_factors[i] > 0.0 && size_factors[i] <= DBL_LARGEST))
            throw Error(BMX_ERR_ARG, "size factors should be positive");
}

void norm_check_run(double min_mean, int log, double pseudo_count) {
    if (min_mean != min_mean) throw Error(BMX_ERR_ARG, "'min_mean' must be a number");
    if (log != 0 && log != 1) throw Error(BMX_ERR_ARG, "'log' is 0 or 1");
    if (!std::isfinite(pseudo_count)) throw Error(BMX_ERR_ARG, "'pseudo_count' must be finite");
}

// what both handles keep for a batch beside its counts
struct NormStats : ChunkProgress {
    DevBuf<double> w;     // [n] library sizes, or the size factors given
    DevBuf<double> sf;    // [n] w / mean(w)
    DevBuf<double> sfo;   // [n] sf / rescaling
    DevBuf<double> part;  // [nchunks][nS] (sparse counts: [nchunks][G])
    bool given = false;
};
struct NormBatch : ResidentBatch, NormStats {};

namespace {

struct StatPointers {
    double *ave, *ratios, *rescaling;
};

// The stages between the reductions and the output pass, on kstream, for either handle: size factors and averages
// (launch_ave(batch, scale, ave) queues a batch's averaging kernel), the ratios and the reference, the size factors the
// values are divided by.  flags: the words from F_SF on are cleared first.
template <class Batch, class F>
StatPointers launch_stat_stages(const std::vector<std::unique_ptr<Batch>>& batches, int nS, double min_mean,
                                DevBuf<double>& stats, int32_t* flags, hipStream_t kstream, SpanTimer& timer,
                                F&& launch_ave) {
    const int B = (int)batches.size();
    const int64_t npairs = (int64_t)B * (B - 1) / 2;
    if (npairs > 0x7fffffffll) throw Error(BMX_ERR_ARG, "too many batches");
    double* ave = stats.reserve((size_t)B * nS + (size_t)B * B + 2 * (size_t)B);  // ave [B][nS], ratios [B][B],
    double* ratios = ave + (size_t)B * nS;                                        // rescaling [B], scale [B]
    double* rescaling = ratios + (size_t)B * B;
    double* scale = rescaling + B;
    BMX_HIP(hipMemsetAsync(flags + F_SF, 0, (F_WORDS - F_SF) * sizeof(int32_t), kstream));
    BMX_HIP(hipMemsetAsync(ratios, 0, (size_t)B * B * sizeof(double), kstream));
    int ea = timer.mark(kstream);
    for (int bi = 0; bi < B; ++bi) {
        Batch& b = *batches[(size_t)bi];
        hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(256), 0, kstream, (const double*)b.w.p, b.n, b.sf.p, scale + bi,
                           flags);
        BMX_LAUNCH_CHECK();
        launch_ave(b, (const double*)(scale + bi), ave + (size_t)bi * nS);
        BMX_LAUNCH_CHECK();
    }
    timer.span(1, ea, timer.mark(kstream));
    ea = timer.mark(kstream);
    if (npairs > 0) {
        hipLaunchKernelGGL(ratio_kernel, dim3((unsigned)npairs), dim3(RT), 0, kstream, (const double*)ave, nS, B, min_mean,
                           ratios, flags);
        BMX_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(smallest_kernel, dim3(1), dim3(64), 0, kstream, ratios, B, rescaling, flags);
    BMX_LAUNCH_CHECK();
    for (int bi = 0; bi < B; ++bi) {
        Batch& b = *batches[(size_t)bi];
        hipLaunchKernelGGL(sfout_kernel, dim3((unsigned)cdiv(b.n, 256)), dim3(256), 0, kstream, (const double*)b.sf.p, b.n,
                           (const double*)(rescaling + bi), b.sfo.p);
        BMX_LAUNCH_CHECK();
    }
    timer.span(2, ea, timer.mark(kstream));
    return {ave, ratios, rescaling};
}

// The small results and the first nflags flag words, behind everything else on kstream; waits for the stream.
template <class Batch>
void fetch_small_results(const std::vector<std::unique_ptr<Batch>>& batches, int nS, const StatPointers& st,
                         const int32_t* flags_dev, int nflags, int32_t* flags, hipStream_t kstream, double* sf_out,
                         double* ave_out, double* ratios_out) {
    const size_t B = batches.size();
    BMX_HIP(hipMemcpyAsync(flags, flags_dev, (size_t)nflags * sizeof(int32_t), hipMemcpyDeviceToHost, kstream));
    if (ave_out) BMX_HIP(hipMemcpyAsync(ave_out, st.ave, B * nS * sizeof(double), hipMemcpyDeviceToHost, kstream));
    if (ratios_out) BMX_HIP(hipMemcpyAsync(ratios_out, st.ratios, B * B * sizeof(double), hipMemcpyDeviceToHost, kstream));
    if (sf_out) {
        int64_t at = 0;
        for (auto& b : batches) {
            BMX_HIP(hipMemcpyAsync(sf_out + at, b->sfo.p, (size_t)b->n * sizeof(double), hipMemcpyDeviceToHost, kstream));
            at += b->n;
        }
    }
    BMX_HIP(hipStreamSynchronize(kstream));
}

void throw_if_flagged(const int32_t* flags) {
    if (flags[F_COUNT]) throw Error(BMX_ERR_ARG, "counts should be finite and non-negative");
    if (flags[F_SF]) throw Error(BMX_ERR_ARG, "size factors should be positive");
    if (flags[F_RATIO]) throw Error(BMX_ERR_ARG, "median ratio of averages between batches is not finite");
}

// The statistic rows of a handle on the device: 0-based rows, and how often every one of the G rows is named.
void upload_stat_rows(const int32_t* stat_rows, int64_t n_stat, int G, DevBuf<int32_t>& rows_dev, DevBuf<double>& mult_dev,
                      hipStream_t stream) {
    std::vector<int32_t> rows(stat_rows, stat_rows + n_stat);
    std::vector<double> mult((size_t)G, 0.0);
    for (int32_t& r : rows) {
        r -= 1;
        mult[(size_t)r] += 1.0;
    }
    BMX_HIP(hipMemcpyAsync(rows_dev.reserve(rows.size()), rows.data(), rows.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                           stream));
    BMX_HIP(hipMemcpyAsync(mult_dev.reserve(mult.size()), mult.data(), mult.size() * sizeof(double), hipMemcpyHostToDevice,
                           stream));
    BMX_HIP(hipStreamSynchronize(stream));
}

}  // namespace

// The count batches stay resident between the passes that need every cell (library sizes, per-gene averages), the ratio
// stage and the pass that writes the normalized values.
class Norm : ResidentBatches<NormBatch> {
  public:
    // stat_rows: 1-based rows the size factors, averages and ratios are taken over (in the order given, a row named twice
    // counts twice), n_stat of them; null / n_stat < 0: all G rows.  The values are written for all G rows either way.
    // (the caller has checked them: norm_check_create)
    Norm(int device, int G, const int32_t* stat_rows, int64_t n_stat) : ResidentBatches(device, G, "bmx_norm_begin_batch") {
        CacheScope scope(&cache_);
        BMX_HIP(hipStreamCreateWithFlags(&kstream_, hipStreamNonBlocking));
        BMX_HIP(hipEventCreateWithFlags(&landed_, hipEventDisableTiming));
        nS_ = G;
        if (stat_rows && n_stat >= 0) {
            nS_ = (int)n_stat;
            upload_stat_rows(stat_rows, n_stat, G, rows_, mult_, stream_);
            subset_ = true;
        }
        BMX_HIP(hipMemsetAsync(flags_.reserve(F_WORDS), 0, F_WORDS * sizeof(int32_t), stream_));
        BMX_HIP(hipStreamSynchronize(stream_));
    }
    ~Norm() {
        retire({kstream_});
        if (landed_) (void)hipEventDestroy(landed_);
    }

    // a batch of n cells, size_factors [n] (any scale; null: library sizes over the statistic rows); its columns follow
    // in blocks, in order
    void begin_batch(int64_t n, const double* size_factors) {
        norm_check_batch(n, size_factors);
        begin(n, [&](NormBatch& b) {
            b.nchunks = cdiv(n, NCH);
            b.part.reserve((size_t)b.nchunks * nS_);
            b.w.reserve((size_t)n);
            b.sf.reserve((size_t)n);
            b.sfo.reserve((size_t)n);
            b.given = size_factors != nullptr;
            if (b.given) {
                BMX_HIP(hipMemcpyAsync(b.w.p, size_factors, (size_t)n * sizeof(double), hipMemcpyHostToDevice, stream_));
                BMX_HIP(hipStreamSynchronize(stream_));
            }
        });
    }

    void add_block(const double* x_block, int64_t m) {
        const double t0 = now_ms();
        add(x_block, m, [&](NormBatch& b, double*) {
            BMX_HIP(hipEventRecord(landed_, stream_));
            BMX_HIP(hipStreamWaitEvent(kstream_, landed_, 0));
            launch_sums(b, b.filled - m, m);
            if (b.complete()) {
                BMX_HIP(hipStreamSynchronize(stream_));
                BMX_HIP(hipStreamSynchronize(kstream_));
                timer_.collect(ms_);
            }
        });
        ms_[0] += now_ms() - t0;
    }

    // outs[b]: [G x n_b] column-major host memory.  Nullable: sf_out [cells of all batches in upload order] the size
    // factors the values were divided by, ave_out [n_stat x B] column-major, ratios_out [B x B] row-major
    // (ratios_out[i * B + j] is the median over the kept genes of ave_j / ave_i), smallest_out the 1-based reference batch.
    void run(double min_mean, int log, double pseudo, double* const* outs, double* sf_out, double* ave_out,
             double* ratios_out, int32_t* smallest_out) {
        norm_check_run(min_mean, log, pseudo);
        if (batches_.empty()) throw Error(BMX_ERR_ARG, "no batch has been added");
        if (!outs) throw Error(BMX_ERR_ARG, "'outs' is missing");
        for (size_t i = 0; i < batches_.size(); ++i) {
            if (!batches_[i]->complete()) throw Error(BMX_ERR_ARG, "a batch has not received all its cells");
            if (!outs[i]) throw Error(BMX_ERR_ARG, "an output matrix is missing");
        }
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        const int G = G_, nS = nS_;
        const StatPointers st = launch_stat_stages(
            batches_, nS, min_mean, stats_, flags_.p, kstream_, timer_, [&](NormBatch& b, const double* scale, double* ave) {
                hipLaunchKernelGGL(ave_kernel, dim3((unsigned)cdiv(nS, 256)), dim3(256), 0, kstream_, (const double*)b.part.p,
                                   nS, b.nchunks, scale, ave);
            });

        const double t0 = now_ms();
        // (the second grid dimension holds at most 65 535 workgroups of CPW cells)
        const int64_t per = std::min<int64_t>(
            65535 * (int64_t)CPW, std::max<int64_t>(1, (int64_t)(OUT_BLOCK_BYTES / (sizeof(double) * (size_t)G))));
        const bool v2 = G % 2 == 0;
        blocked_output(batches_, G, per, kstream_, stream_, timer_, 3, out_, outs,
                       [&](int, const NormBatch& b, int64_t c0, int mb, double* out) {
                           const dim3 grid((unsigned)cdiv(v2 ? G / 2 : G, 256), (unsigned)cdiv(mb, CPW));
                           const double* src = b.x.p + c0 * G;
                           const double* so = b.sfo.p + c0;
#define BMX_NORM_OUT(V2, LOG) \
    hipLaunchKernelGGL((norm_out_kernel<V2, LOG>), grid, dim3(256), 0, kstream_, src, G, mb, so, pseudo, out)
                           switch ((v2 ? 2 : 0) + (log ? 1 : 0)) {
                               case 0: BMX_NORM_OUT(false, false); break;
                               case 1: BMX_NORM_OUT(false, true); break;
                               case 2: BMX_NORM_OUT(true, false); break;
                               default: BMX_NORM_OUT(true, true); break;
                           }
#undef BMX_NORM_OUT
                       });
        ms_[4] += now_ms() - t0;

        int32_t flags[F_WORDS] = {0, 0, 0, 0};
        fetch_small_results(batches_, nS, st, flags_.p, F_WORDS, flags, kstream_, sf_out, ave_out, ratios_out);
        timer_.collect(ms_);
        if (smallest_out) *smallest_out = flags[F_SMALLEST] + 1;
        throw_if_flagged(flags);
    }

    // milliseconds since the handle was made: upload (host wall time), HIP-event time of the statistics passes (column
    // sums, per-gene sums, size factors, averages), of the ratio stage, of the output kernels, and the host wall time of
    // the output pass with its downloads
    using ResidentBatches::stage_ms;

  private:
    int mark() { return timer_.mark(kstream_); }

    // on the kernel stream: the column sums of the cells [c0, c0 + m) of b, which have just been queued for upload, then
    // the chunks of b that are complete with the cells resident so far and not summed yet
    void launch_sums(NormBatch& b, int64_t c0, int64_t m) {
        const int G = G_, nS = nS_;
        const int ea = mark();
        const dim3 cgrid((unsigned)cdiv(m, 4));
        double* w = b.given ? nullptr : b.w.p;
        if (subset_)
            hipLaunchKernelGGL(colsum_kernel<2>, cgrid, dim3(256), 0, kstream_, (const double*)b.x.p, G, c0, m,
                               (const double*)mult_.p, w, flags_.p);
        else if (G % 2 == 0)
            hipLaunchKernelGGL(colsum_kernel<1>, cgrid, dim3(256), 0, kstream_, (const double*)b.x.p, G, c0, m,
                               (const double*)nullptr, w, flags_.p);
        else
            hipLaunchKernelGGL(colsum_kernel<0>, cgrid, dim3(256), 0, kstream_, (const double*)b.x.p, G, c0, m,
                               (const double*)nullptr, w, flags_.p);
        BMX_LAUNCH_CHECK();
        const int complete = b.chunks_complete(b.filled, b.n, NCH);
        if (complete > b.sum_done) {
            const unsigned nch = (unsigned)(complete - b.sum_done);
            if (!subset_ && G % 2 == 0)
                hipLaunchKernelGGL(gene_partial_kernel<true>, dim3(nch, (unsigned)cdiv(nS / 2, 256)), dim3(256), 0, kstream_,
                                   (const double*)b.x.p, G, (const int32_t*)nullptr, nS, (const double*)b.w.p, b.n, b.sum_done,
                                   b.part.p);
            else
                hipLaunchKernelGGL(gene_partial_kernel<false>, dim3(nch, (unsigned)cdiv(nS, 256)), dim3(256), 0, kstream_,
                                   (const double*)b.x.p, G, (const int32_t*)(subset_ ? rows_.p : nullptr), nS,
                                   (const double*)b.w.p, b.n, b.sum_done, b.part.p);
            BMX_LAUNCH_CHECK();
            b.sum_done = complete;
        }
        timer_.span(1, ea, mark());
    }

    hipStream_t kstream_ = nullptr;  // kernels (the store's stream_ takes the copies)
    hipEvent_t landed_ = nullptr;
    DevBuf<double> stats_, mult_, out_[2];
    DevBuf<int32_t> rows_, flags_;
    int nS_ = 0;
    bool subset_ = false;
};

// ---- the same for sparse counts: a batch is kept as CSC (indptr int64, 0-based int32 rows, FP64 values), its cells
// arrive in column blocks, and the values are written for the stored entries only.
struct SparseNormBatch : CscBatch, NormStats {};

class NormSparse : ResidentBatches<SparseNormBatch> {
  public:
    NormSparse(int device, int G, const int32_t* stat_rows, int64_t n_stat)
        : ResidentBatches(device, G, "bmx_norm_sparse_begin_batch") {
        CacheScope scope(&cache_);
        BMX_HIP(hipStreamCreateWithFlags(&kstream_, hipStreamNonBlocking));
        BMX_HIP(hipEventCreateWithFlags(&landed_, hipEventDisableTiming));
        nS_ = G;
        if (stat_rows && n_stat >= 0) {
            nS_ = (int)n_stat;
            upload_stat_rows(stat_rows, n_stat, G, rows_, mult_, stream_);
            subset_ = true;
        }
        BMX_HIP(hipMemsetAsync(flags_.reserve(F_SPARSE_WORDS), 0, F_SPARSE_WORDS * sizeof(int32_t), stream_));
        zero_.reserve(1);
        BMX_HIP(hipStreamSynchronize(stream_));
    }
    ~NormSparse() {
        retire({kstream_});
        if (landed_) (void)hipEventDestroy(landed_);
    }

    // a batch of n cells with nnz stored entries in all; size_factors as for Norm::begin_batch
    void begin_batch(int64_t n, const double* size_factors, int64_t nnz) {
        norm_check_batch(n, size_factors);
        begin_csc(n, nnz, [&](SparseNormBatch& b) {
            b.nchunks = cdiv(n, NCH);
            b.part.reserve((size_t)b.nchunks * G_);
            b.w.reserve((size_t)n);
            b.sf.reserve((size_t)n);
            b.sfo.reserve((size_t)n);
            b.given = size_factors != nullptr;
            if (b.given) {
                BMX_HIP(hipMemcpyAsync(b.w.p, size_factors, (size_t)n * sizeof(double), hipMemcpyHostToDevice, stream_));
                BMX_HIP(hipStreamSynchronize(stream_));
            }
        });
    }

    // the next m cells of the batch begun last: indptr [m + 1] relative to the block, its nnz entries
    void add_block(int64_t m, const int64_t* indptr, const int32_t* indices, const double* data, int64_t nnz) {
        const double t0 = now_ms();
        add_csc(m, indptr, indices, data, nnz, [&](SparseNormBatch& b, int64_t c0) {
            BMX_HIP(hipEventRecord(landed_, stream_));
            BMX_HIP(hipStreamWaitEvent(kstream_, landed_, 0));
            launch_sums(b, c0, m);
            if (b.complete()) {
                BMX_HIP(hipStreamSynchronize(stream_));
                BMX_HIP(hipStreamSynchronize(kstream_));
                timer_.collect(ms_);
            }
        });
        ms_[0] += now_ms() - t0;
    }

    // outs[b]: [nnz_b] the values of batch b's stored entries, in their order.  zero_out (nullable): what the same pass
    // makes of a count of zero, log2(pseudo) by the device's log2 or 0.  The rest as for Norm::run.
    void run(double min_mean, int log, double pseudo, double* const* outs, double* sf_out, double* ave_out,
             double* ratios_out, int32_t* smallest_out, double* zero_out) {
        norm_check_run(min_mean, log, pseudo);
        if (batches_.empty()) throw Error(BMX_ERR_ARG, "no batch has been added");
        if (!outs) throw Error(BMX_ERR_ARG, "'outs' is missing");
        for (size_t i = 0; i < batches_.size(); ++i) {
            if (!batches_[i]->complete()) throw Error(BMX_ERR_ARG, "a batch has not received all its cells");
            if (!outs[i] && batches_[i]->nnz > 0) throw Error(BMX_ERR_ARG, "an output array is missing");
        }
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        const int G = G_, nS = nS_;
        const StatPointers st = launch_stat_stages(
            batches_, nS, min_mean, stats_, flags_.p, kstream_, timer_,
            [&](SparseNormBatch& b, const double* scale, double* ave) {
                if (subset_)
                    hipLaunchKernelGGL(ave_rows_kernel, dim3((unsigned)cdiv(nS, 256)), dim3(256), 0, kstream_,
                                       (const double*)b.part.p, G, (const int32_t*)rows_.p, nS, b.nchunks, scale, ave);
                else
                    hipLaunchKernelGGL(ave_kernel, dim3((unsigned)cdiv(nS, 256)), dim3(256), 0, kstream_,
                                       (const double*)b.part.p, nS, b.nchunks, scale, ave);
            });

        const double t0 = now_ms();
        if (log)
            hipLaunchKernelGGL(zero_image_kernel<true>, dim3(1), dim3(64), 0, kstream_, pseudo, zero_.p);
        else
            hipLaunchKernelGGL(zero_image_kernel<false>, dim3(1), dim3(64), 0, kstream_, pseudo, zero_.p);
        BMX_LAUNCH_CHECK();
        // a block: whole cells of a batch with at most OUT_BLOCK_BYTES of stored entries (one cell if it alone has more)
        std::vector<OutBlock> blocks;
        for (size_t bi = 0; bi < batches_.size(); ++bi)
            for (OutBlock k : plan_csc_output_blocks(batches_[bi]->hindptr.data(), batches_[bi]->n,
                                                     (int64_t)(OUT_BLOCK_BYTES / sizeof(double)))) {
                k.bi = (int)bi;
                blocks.push_back(k);
            }
        run_output_blocks(blocks, kstream_, stream_, timer_, 3, out_, outs, [&](const OutBlock& k, double* out) {
            const SparseNormBatch& b = *batches_[(size_t)k.bi];
            const dim3 grid((unsigned)cdiv(k.mb, 4));
            if (log)
                hipLaunchKernelGGL(sp_out_kernel<true>, grid, dim3(256), 0, kstream_, (const int64_t*)b.indptr.p,
                                   (const double*)b.data.p, k.c0, k.mb, (const double*)b.sfo.p, pseudo, out);
            else
                hipLaunchKernelGGL(sp_out_kernel<false>, grid, dim3(256), 0, kstream_, (const int64_t*)b.indptr.p,
                                   (const double*)b.data.p, k.c0, k.mb, (const double*)b.sfo.p, pseudo, out);
        });
        ms_[4] += now_ms() - t0;

        int32_t flags[F_SPARSE_WORDS] = {0, 0, 0, 0, 0, 0};
        double zero = 0.0;
        BMX_HIP(hipMemcpyAsync(&zero, zero_.p, sizeof(double), hipMemcpyDeviceToHost, kstream_));
        fetch_small_results(batches_, nS, st, flags_.p, F_SPARSE_WORDS, flags, kstream_, sf_out, ave_out, ratios_out);
        timer_.collect(ms_);
        if (smallest_out) *smallest_out = flags[F_SMALLEST] + 1;
        if (zero_out) *zero_out = zero;
        throw_if_bad_pattern(flags + F_PATTERN);
        throw_if_flagged(flags);
    }

    using ResidentBatches::stage_ms;  // the stages of Norm

  private:
    int mark() { return timer_.mark(kstream_); }

    // on the kernel stream: the library sizes of the cells [c0, c0 + m) of b, which have just been queued for upload, then
    // the chunks of b that are complete with the cells resident so far and not summed yet (Norm::launch_sums)
    void launch_sums(SparseNormBatch& b, int64_t c0, int64_t m) {
        const int ea = mark();
        hipLaunchKernelGGL(sp_colsum_kernel, dim3((unsigned)cdiv(m, 4)), dim3(256), 0, kstream_, (const int64_t*)b.indptr.p,
                           (const int32_t*)b.indices.p, (const double*)b.data.p, G_, c0, m,
                           (const double*)(subset_ ? mult_.p : nullptr), b.given ? nullptr : b.w.p, flags_.p);
        BMX_LAUNCH_CHECK();
        const int complete = b.chunks_complete(b.filled, b.n, NCH);
        for (int ch = b.sum_done; ch < complete; ch += 65535) {  // (a grid dimension holds at most 65 535 workgroups)
            const unsigned nch = (unsigned)std::min(65535, complete - ch);
            hipLaunchKernelGGL(sp_gene_partial_kernel, dim3(nch, (unsigned)cdiv(G_, GT)), dim3(256), 0, kstream_,
                               (const int64_t*)b.indptr.p, (const int32_t*)b.indices.p, (const double*)b.data.p, G_,
                               (const double*)b.w.p, b.n, ch, b.part.p);
            BMX_LAUNCH_CHECK();
        }
        b.sum_done = std::max(b.sum_done, complete);
        timer_.span(1, ea, mark());
    }

    hipStream_t kstream_ = nullptr;  // kernels (the store's stream_ takes the copies)
    hipEvent_t landed_ = nullptr;
    DevBuf<double> stats_, mult_, zero_, out_[2];
    DevBuf<int32_t> rows_, flags_;
    int nS_ = 0;
    bool subset_ = false;
};

}  // namespace bmx

/* ---------------------------------------------------------------- bmx_norm_*, bmx_norm_sparse_* ----------------- */
struct bmx_norm final : bmx::Norm {
    using Norm::Norm;
};
struct bmx_norm_sparse final : bmx::NormSparse {
    using NormSparse::NormSparse;
};

extern "C" {

int32_t bmx_norm_create(int32_t device, int32_t G, const int32_t* stat_rows, int64_t n_stat, bmx_norm_t** out) {
    return bmx::guarded([&] {
        if (!out) throw bmx::Error(BMX_ERR_ARG, "null output pointer");
        bmx::norm_check_create(G, stat_rows, n_stat);
        *out = new bmx_norm(device, G, stat_rows, n_stat);
    });
}

void bmx_norm_destroy(bmx_norm_t* h) { delete h; }

int32_t bmx_norm_check_create(int32_t G, const int32_t* stat_rows, int64_t n_stat) {
    return bmx::guarded([&] { bmx::norm_check_create(G, stat_rows, n_stat); });
}

int32_t bmx_norm_check_batch(int64_t n, const double* size_factors) {
    return bmx::guarded([&] { bmx::norm_check_batch(n, size_factors); });
}

int32_t bmx_norm_check_run(double min_mean, int32_t log, double pseudo_count) {
    return bmx::guarded([&] { bmx::norm_check_run(min_mean, log, pseudo_count); });
}

int32_t bmx_norm_begin_batch(bmx_norm_t* h, int64_t n, const double* size_factors) {
    return bmx::guarded([&] { bmx::live(h).begin_batch(n, size_factors); });
}

int32_t bmx_norm_add_block(bmx_norm_t* h, const double* x_block, int64_t n_block) {
    return bmx::guarded([&] { bmx::live(h).add_block(x_block, n_block); });
}

int32_t bmx_norm_run(bmx_norm_t* h, double min_mean, int32_t log, double pseudo_count, double* const* outs, double* sf_out,
                     double* ave_out, double* ratios_out, int32_t* smallest_out) {
    return bmx::guarded([&] {
        bmx::live(h).run(min_mean, log, pseudo_count, outs, sf_out, ave_out, ratios_out, smallest_out);
    });
}

int32_t bmx_norm_stage_ms(const bmx_norm_t* h, double* out5) {
    return bmx::guarded([&] {
        if (!h || !out5) throw bmx::Error(BMX_ERR_ARG, "null argument");
        h->stage_ms(out5);
    });
}

int32_t bmx_norm_sparse_create(int32_t device, int32_t G, const int32_t* stat_rows, int64_t n_stat,
                               bmx_norm_sparse_t** out) {
    return bmx::guarded([&] {
        if (!out) throw bmx::Error(BMX_ERR_ARG, "null output pointer");
        bmx::norm_check_create(G, stat_rows, n_stat);
        *out = new bmx_norm_sparse(device, G, stat_rows, n_stat);
    });
}

void bmx_norm_sparse_destroy(bmx_norm_sparse_t* h) { delete h; }

int32_t bmx_norm_check_sparse_block(int64_t n, int64_t filled, int64_t n_block, const int64_t* indptr,
                                    const int32_t* indices, const double* data, int64_t nnz) {
    return bmx::guarded([&] { bmx::check_csc_block(n, filled, n_block, indptr, indices, data, nnz); });
}

int32_t bmx_norm_sparse_begin_batch(bmx_norm_sparse_t* h, int64_t n, const double* size_factors, int64_t nnz) {
    return bmx::guarded([&] { bmx::live(h).begin_batch(n, size_factors, nnz); });
}

int32_t bmx_norm_sparse_add_block(bmx_norm_sparse_t* h, int64_t n_block, const int64_t* indptr, const int32_t* indices,
                                  const double* data, int64_t nnz) {
    return bmx::guarded([&] { bmx::live(h).add_block(n_block, indptr, indices, data, nnz); });
}

int32_t bmx_norm_sparse_run(bmx_norm_sparse_t* h, double min_mean, int32_t log, double pseudo_count, double* const* outs,
                            double* sf_out, double* ave_out, double* ratios_out, int32_t* smallest_out, double* zero_out) {
    return bmx::guarded([&] {
        bmx::live(h).run(min_mean, log, pseudo_count, outs, sf_out, ave_out, ratios_out, smallest_out, zero_out);
    });
}

int32_t bmx_norm_sparse_stage_ms(const bmx_norm_sparse_t* h, double* out5) {
    return bmx::guarded([&] {
        if (!h || !out5) throw bmx::Error(BMX_ERR_ARG, "null argument");
        h->stage_ms(out5);
    });
}

}  // extern "C"
