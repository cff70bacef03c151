// clusterMNN() on the device (R/clusterMNN.R:101-312): the two per-cell stages around the centroid-level merge.
//   a. .compute_centroids (:231-244): the mean of every cluster's restricted cells, of cosineNorm(x) when asked for.
//      The host sorts the restricted cells by cluster (a counting sort, ascending cell within a cluster) and cuts every
//      cluster's list into chunks of CCH cells.  centroid_partial_kernel: one workgroup per (chunk, tile of 256 genes),
//      lanes along the genes so that every cell's column is read coalesced; centroid_reduce_kernel adds a cluster's
//      chunk sums and divides by the count.  The orders of both are those of ordered_sums.hpp.  x is read once.
//   b. .propagate_to_cells (:262-282) + .smooth_gaussian_from_centroids (:286-312) for one batch:
//      cur = crossprod(cosineNorm(x)[subset,], rotation) - centers %*% rotation through cosnorm_project_device (the
//      rotation scattered to all genes, zero outside the subset, so that x is again read once);
//      nearest_kernel: every squared distance ||cur_i - centroid_j||^2 by differences, added over the columns in
//      ascending order (contraction is off: each is the double a plain loop gives), kept as D2 [C][n], and the distance
//      to the nearest centroid; median_select_kernel: sigma = median of those over the restricted cells by an exact
//      radix selection on the doubles' bit patterns (the two middle values' mean for an even count, as numpy.median);
//      smooth_kernel: w_ij = -D2_ij / sigma^2, softmax over j with the row maximum taken off, cur_i += sum_j w_ij delta_j
//      in ascending j, the deltas staged through LDS sixteen columns at a time.
// All FP64 vector arithmetic: the work is n C d multiply-adds, small next to the two streaming reads of x.
//
// ClusterSparse (bmx_cluster_sparse_*) is the same handle over batches kept as CSC (resident_batches.hpp: CscBatch); only
// the two streaming reads differ, everything from centroid_reduce_kernel / finish_projection_kernel on is shared.
//   prepare  csp_prepare_kernel behind every uploaded block, one wave a cell: the pattern flags of every stored entry
//            and, under cos_norm, the cell's l2 over the subset rows (a G-long multiplicity mask stands for the list).
//   a.       csp_centroid_partial_kernel: one workgroup per (chunk of the sorted restricted list, tile of
//            CLUSTER_SPARSE_GENE_TILE genes), the tile's accumulators in the LDS; the chunk's cells one after the other
//            in list order (csc_tile_walk over the list), every stored entry adding val (/ pmax(1e-8, l2[cell])) to its
//            row -- the dense kernel's terms with the zeros left out, which changes no bit of a sum: without cos_norm the
//            centroids equal the dense handle's bit for bit.  part has the dense layout, the reduction is the dense one.
//   b.       csp_project_kernel: one wave a cell, 64 of the d columns at a time with a lane per column (gather_rows64):
//            acc[c, :] = sum over the cell's stored entries of val * R[row, :], R the rotation scattered to all genes
//            (row-major, zero outside the subset), so the column is read whole and needs no cut.  No two cells share a K
//            dimension, hence no MFMA.  A workgroup's 32 cells leave through an LDS tile, 256 bytes a column.
// A row index is compared with [0, G) before it addresses anything, a failing entry is skipped, and both passes refuse a
// handle whose flags are raised.  No floating-point atomics: no result depends on the grid or on the upload blocks.
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

constexpr int CCH = 256;  // cells per chunk of the centroid pass
constexpr int JT = 16;    // centroids (nearest_kernel) / columns (smooth_kernel) per LDS tile
constexpr int DMAX = 256;  // columns cosnorm_project_device and the merge engine take
constexpr int MSEL_T = 1024;
constexpr int SGT = CLUSTER_SPARSE_GENE_TILE;  // genes per LDS tile of the CSC centroid pass (32 KiB of accumulators)
constexpr int PCELLS = 32;                     // cells a workgroup of the CSC projection takes (eight a wave)

// part[chunk][g] = sum over the chunk's cells, in list order, of x[g, cell] (/ pmax(1e-8, l2[cell]))
__global__ __launch_bounds__(256) void centroid_partial_kernel(const double* __restrict__ x, int G,
                                                               const double* __restrict__ l2,
                                                               const int32_t* __restrict__ order,
                                                               const int32_t* __restrict__ chunk_begin,
                                                               double* __restrict__ part) {
    const int g = blockIdx.y * 256 + threadIdx.x;
    if (g >= G) return;
    const int ch = blockIdx.x;
    const int b = chunk_begin[ch], e = chunk_begin[ch + 1];
    struct Cell {
        double v, L;
    };
    double s = 0.0;
    ordered_walk4(
        b, e,
        [&](int i) {
            const int c = order[i];
            return Cell{x[(int64_t)c * G + g], l2 ? l2[c] : 1.0};
        },
        [&](const Cell& q) { s += l2 ? q.v / cos_clamp(q.L) : q.v; });
    part[(int64_t)ch * G + g] = s;
}

// out[g, cl] = (sum of the cluster's chunk sums, ascending chunk) / count
__global__ __launch_bounds__(256) void centroid_reduce_kernel(const double* __restrict__ part, int G, int C,
                                                              const int32_t* __restrict__ cluster_chunk0,
                                                              const int32_t* __restrict__ count,
                                                              double* __restrict__ out) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int cl = blockIdx.y;
    if (g >= G || cl >= C) return;
    const int f = cluster_chunk0[cl], l = cluster_chunk0[cl + 1];
    const auto at = [&](int ch) { return part[(int64_t)ch * G + g]; };
    out[(int64_t)cl * G + g] = fold_ascending(at(f), f + 1, l, at) / (double)count[cl];
}

// cur[c, t] = acc[c, t] / pmax(1e-8, l2[c]) - cu[t], in place ([n x d] column-major)
__global__ void finish_projection_kernel(double* __restrict__ cur, int n, int d, const double* __restrict__ l2,
                                         const double* __restrict__ cu) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)n * d) return;
    const int t = (int)(e / n);
    const int c = (int)(e - (int64_t)t * n);
    double v = cur[e];
    if (l2) v = v / cos_clamp(l2[c]);
    cur[e] = v - cu[t];
}

// ---- the CSC batches' two streaming reads
// The cells [c0, c0 + m), one wave a cell: flags is the pattern pair (csc_entry_flags); l2[c] (l2 null: not wanted) over the
// rows of the subset, mult [G] (null: all rows, once each) how often a row is in it.  A row outside [0, G) addresses
// nothing.
__global__ __launch_bounds__(256) void csp_prepare_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                          const double* __restrict__ val, int G, int64_t c0, int64_t m,
                                                          const int32_t* __restrict__ mult, double* __restrict__ l2,
                                                          int32_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int64_t c = c0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= c0 + m) return;  // (a whole wave leaves)
    const int64_t kb = indptr[c], ke = indptr[c + 1];
    double s = 0.0;
    int bad_row = 0, bad_order = 0;
    for (int64_t k = kb + lane; k < ke; k += 64) {
        const int32_t r = idx[k];
        if (csc_entry_flags(idx, k, kb, r, G, bad_row, bad_order)) continue;
        if (!l2) continue;
        const double v = val[k];
        if (!mult) s += v * v;
        else if (mult[r] > 0) s += (double)mult[r] * (v * v);
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (bad_row) flags[CSC_F_ROW] = 1;
    if (bad_order) flags[CSC_F_ORDER] = 1;
    if (l2 && lane == 0) l2[c] = sqrt(s);
}

// centroid_partial_kernel over CSC: workgroup (chunk, tile of SGT genes).  part[chunk][g] = the sum over the chunk's cells,
// in list order, of the stored x[g, cell] (/ pmax(1e-8, l2[cell])): one accumulator a gene, in the LDS.  Rows are unique
// within a canonical column, so no two threads meet at one (where they do, CSC_F_ORDER has been raised and the handle
// refuses the pass's result).
__global__ __launch_bounds__(256) void csp_centroid_partial_kernel(const int64_t* __restrict__ indptr,
                                                                   const int32_t* __restrict__ idx,
                                                                   const double* __restrict__ val, int G,
                                                                   const double* __restrict__ l2,
                                                                   const int32_t* __restrict__ order,
                                                                   const int32_t* __restrict__ chunk_begin,
                                                                   double* __restrict__ part) {
    __shared__ double acc[SGT];
    __shared__ int64_t lo[CCH], hi[CCH];
    const int ch = blockIdx.x;
    const int g0 = blockIdx.y * SGT, g1 = min(G, g0 + SGT);
    for (int i = threadIdx.x; i < g1 - g0; i += 256) acc[i] = 0.0;  // (the walk's first barrier comes before any entry)
    const int b = chunk_begin[ch], e = chunk_begin[ch + 1];
    double L = 1.0;
    csc_tile_walk<CCH>(
        indptr, idx, 0, 0, g0, g1, lo, hi,
        [&](int64_t c) {
            if (l2) L = l2[c];
        },
        [&](int64_t, int64_t k, int r) { acc[r - g0] += l2 ? val[k] / cos_clamp(L) : val[k]; }, order, b, e - b);
    for (int i = threadIdx.x; i < g1 - g0; i += 256) part[(int64_t)ch * G + g0 + i] = acc[i];
}

// cur[c, h0 + j] = sum over cell c's stored entries, in order, of val * R[row][h0 + j] for the 64 columns at h0 (R [G][ldr]
// row-major, ldr a multiple of 64 with zeros beyond d), cur [n x d] column-major.  A workgroup takes PCELLS cells, a wave
// eight of them one after the other; the 64 x PCELLS results leave through the LDS so that a column's cells are written
// side by side.
__global__ __launch_bounds__(256) void csp_project_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                          const double* __restrict__ val, int64_t n, int G,
                                                          const double* __restrict__ R, int64_t ldr, int d,
                                                          double* __restrict__ cur) {
    __shared__ double tile[64][PCELLS + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t c0 = (int64_t)blockIdx.x * PCELLS;
    for (int h0 = 0; h0 < d; h0 += 64) {
        for (int q = 0; q < PCELLS / 4; ++q) {
            const int cl = w * (PCELLS / 4) + q;
            const int64_t c = c0 + cl;
            if (c < n) {  // (the same in every lane)
                const int64_t kb = wave_uniform(indptr[c]), ke = wave_uniform(indptr[c + 1]);
                tile[lane][cl] = gather_rows64(idx, val, kb, ke, R + h0, ldr, G, lane);
            }
        }
        __syncthreads();
        for (int e = threadIdx.x; e < 64 * PCELLS; e += 256) {
            const int j = e / PCELLS, cl = e - j * PCELLS;
            if (h0 + j < d && c0 + cl < n) cur[(int64_t)(h0 + j) * n + c0 + cl] = tile[j][cl];
        }
        __syncthreads();  // (the tile is free for the next 64 columns)
    }
}

// One thread per cell, 256 cells a workgroup, JT centroids staged in LDS at a time (every lane reads the same words: a
// broadcast).  D2[j][c] = sum_t (cur[c, t] - cp[j, t])^2 with t ascending; dist[c] = sqrt(min_j D2[j][c]).
__global__ __launch_bounds__(256) void nearest_kernel(const double* __restrict__ cur, int n, int d,
                                                      const double* __restrict__ cp, int C, double* __restrict__ D2,
                                                      double* __restrict__ dist) {
    __shared__ double ps[DMAX * JT];  // [t][jj]
    const int c = blockIdx.x * 256 + threadIdx.x;
    const int cc = c < n ? c : n - 1;
    double best = 0.0;
    for (int j0 = 0; j0 < C; j0 += JT) {
        const int jn = min(JT, C - j0);
        for (int e = threadIdx.x; e < d * JT; e += 256) {
            const int t = e / JT, jj = e - t * JT;
            ps[e] = jj < jn ? cp[(int64_t)t * C + j0 + jj] : 0.0;
        }
        __syncthreads();
        double acc[JT];
#pragma unroll
        for (int jj = 0; jj < JT; ++jj) acc[jj] = 0.0;
        for (int t = 0; t < d; ++t) {
            const double xv = cur[(int64_t)t * n + cc];
            const double* p = ps + t * JT;
#pragma unroll
            for (int jj = 0; jj < JT; ++jj) {
                const double df = xv - p[jj];
                acc[jj] += df * df;
            }
        }
        if (c < n) {
#pragma unroll
            for (int jj = 0; jj < JT; ++jj)
                if (jj < jn) {
                    D2[(int64_t)(j0 + jj) * n + c] = acc[jj];
                    if ((j0 == 0 && jj == 0) || acc[jj] < best) best = acc[jj];
                }
        }
        __syncthreads();
    }
    if (c < n) dist[c] = sqrt(best);
}

// out[0] = numpy.median of dist[rows[i]] (rows null: dist[i]), i < m: one workgroup, eight passes of an 8-bit radix
// selection over the bit patterns (non-negative doubles order as their unsigned patterns; a NaN, whose pattern sorts above
// +Inf, makes the result NaN as numpy does), then one pass for the upper middle value of an even count.  Integer LDS
// counters only: exact and the same from run to run.
__global__ __launch_bounds__(MSEL_T) void median_select_kernel(const double* __restrict__ dist,
                                                               const int32_t* __restrict__ rows, int64_t m,
                                                               double* __restrict__ out) {
    __shared__ unsigned int hist[256];
    __shared__ unsigned long long s_prefix, s_k, s_cnt_le, s_min_gt;
    __shared__ int s_nan;
    const int tid = threadIdx.x;
    const int64_t klo = (m - 1) / 2;  // 0-based rank of the lower middle value
    if (tid == 0) {
        s_prefix = 0ull;
        s_k = (unsigned long long)klo;
        s_cnt_le = 0ull;
        s_min_gt = ~0ull;
        s_nan = 0;
    }
    for (int shift = 56; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        const unsigned long long prefix = s_prefix;
        int last = -1;
        unsigned int run = 0u;  // a run of keys in one bucket costs one atomic
        for (int64_t i = tid; i < m; i += MSEL_T) {
            const double v = dist[rows ? rows[i] : i];
            const unsigned long long key = (unsigned long long)__double_as_longlong(v);
            if (shift == 56 && v != v) s_nan = 1;
            if (shift == 56 || ((key ^ prefix) >> (shift + 8)) == 0ull) {
                const int bkt = (int)((key >> shift) & 255ull);
                if (bkt == last) {
                    ++run;
                } else {
                    if (run) atomicAdd(&hist[last], run);
                    last = bkt;
                    run = 1u;
                }
            }
        }
        if (run) atomicAdd(&hist[last], run);
        __syncthreads();
        if (tid == 0) {
            unsigned long long k = s_k;
            int b = 0;
            for (; b < 255; ++b) {
                if (k < hist[b]) break;
                k -= hist[b];
            }
            s_k = k;
            s_prefix = prefix | ((unsigned long long)b << shift);
        }
        __syncthreads();
    }
    const unsigned long long lo = s_prefix;
    unsigned long long cnt = 0ull, mn = ~0ull;
    for (int64_t i = tid; i < m; i += MSEL_T) {
        const unsigned long long key = (unsigned long long)__double_as_longlong(dist[rows ? rows[i] : i]);
        if (key <= lo)
            ++cnt;
        else if (key < mn)
            mn = key;
    }
    atomicAdd(&s_cnt_le, cnt);
    atomicMin(&s_min_gt, mn);
    __syncthreads();
    if (tid == 0) {
        const double a = __longlong_as_double((long long)lo);
        double r = a;
        if ((m & 1) == 0) {
            const unsigned long long hi = s_cnt_le >= (unsigned long long)(klo + 2) ? lo : s_min_gt;
            r = (a + __longlong_as_double((long long)hi)) / 2.0;
        }
        if (s_nan) r = __longlong_as_double(0x7ff8000000000000ll);
        out[0] = r;
    }
}

// .smooth_gaussian_from_centroids (R/clusterMNN.R:286-312), one thread per cell.  W [C][n] holds the squared distances on
// entry and the normalised weights on exit; cur [n x d] column-major is updated in place.
__global__ __launch_bounds__(256) void smooth_kernel(double* __restrict__ cur, int n, int d, double* __restrict__ W, int C,
                                                     const double* __restrict__ cp, const double* __restrict__ corr,
                                                     const double* __restrict__ sigma) {
    extern __shared__ __attribute__((aligned(16))) char smem_s[];
    double* ds = reinterpret_cast<double*>(smem_s);  // [C][JT]
    const int c = blockIdx.x * 256 + threadIdx.x;
    const int cc = c < n ? c : n - 1;
    const double sg = sigma[0];
    const double s2 = sg * sg;
    double top = 0.0;
    for (int j = 0; j < C; ++j) {
        const double w = -W[(int64_t)j * n + cc] / s2;
        if (j == 0 || w > top) top = w;
    }
    double sum = 0.0;
    if (c < n) {
        for (int j = 0; j < C; ++j) {
            const double e = exp(-W[(int64_t)j * n + c] / s2 - top);
            W[(int64_t)j * n + c] = e;
            sum += e;
        }
        for (int j = 0; j < C; ++j) W[(int64_t)j * n + c] = W[(int64_t)j * n + c] / sum;
    }
    for (int t0 = 0; t0 < d; t0 += JT) {
        const int tn = min(JT, d - t0);
        __syncthreads();  // (the previous tile has been read)
        for (int e = threadIdx.x; e < C * JT; e += 256) {
            const int j = e / JT, tt = e - j * JT;
            const int64_t at = (int64_t)(t0 + tt) * C + j;
            ds[e] = tt < tn ? corr[at] - cp[at] : 0.0;
        }
        __syncthreads();
        double acc[JT];
#pragma unroll
        for (int tt = 0; tt < JT; ++tt) acc[tt] = tt < tn ? cur[(int64_t)(t0 + tt) * n + cc] : 0.0;
        for (int j = 0; j < C; ++j) {
            const double w = W[(int64_t)j * n + cc];
            const double* p = ds + j * JT;
#pragma unroll
            for (int tt = 0; tt < JT; ++tt) acc[tt] += w * p[tt];
        }
        if (c < n) {
#pragma unroll
            for (int tt = 0; tt < JT; ++tt)
                if (tt < tn) cur[(int64_t)(t0 + tt) * n + c] = acc[tt];
        }
    }
}

}  // namespace

// argument checks of Cluster::begin_batch, without a device (throws Error(BMX_ERR_ARG))
void cluster_check_batch(int64_t n, const int32_t* clusters0, int C, const int32_t* restrict_idx, int64_t n_restrict) {
    check_cell_count(n);
    if (C < 1) throw Error(BMX_ERR_ARG, "every batch needs at least one cluster");
    if (C > 65535) throw Error(BMX_ERR_ARG, "a batch holds at most 65 535 clusters");
    if (!clusters0) throw Error(BMX_ERR_ARG, "'clusters' is missing");
    for (int64_t i = 0; i < n; ++i)
        if (clusters0[i] < 0 || clusters0[i] >= C) throw Error(BMX_ERR_ARG, "cluster ids out of range");
    check_restriction(n, restrict_idx, n_restrict);
    std::vector<char> seen((size_t)C, 0);
    if (is_restricted(restrict_idx, n_restrict)) {
        for (int64_t i = 0; i < n_restrict; ++i) seen[(size_t)clusters0[restrict_idx[i] - 1]] = 1;
    } else {
        for (int64_t i = 0; i < n; ++i) seen[(size_t)clusters0[i]] = 1;
    }
    for (int cl = 0; cl < C; ++cl)
        if (!seen[(size_t)cl]) throw Error(BMX_ERR_ARG, "a cluster has no cells remaining after restriction");
}

// argument checks of bmx_cluster_create / bmx_cluster_sparse_create, without a device
void check_cluster_create(int G, const int32_t* subset_row, int n_subset_row, const void* out) {
    if (!out) throw Error(BMX_ERR_ARG, "null output pointer");
    if (G < 1) throw Error(BMX_ERR_ARG, "clusterMNN needs at least one gene");
    if (n_subset_row < 0 || (n_subset_row > 0 && !subset_row)) throw Error(BMX_ERR_ARG, "invalid 'subset_row'");
    for (int32_t i = 0; i < n_subset_row; ++i)
        if (subset_row[i] < 1 || subset_row[i] > G) throw Error(BMX_ERR_SUBSET, "subset indices out of range");
}

// The host half of begin_batch, the same for dense and CSC batches: the checks above, the counting sort of the restricted
// cells by cluster (a cell named twice counts twice, as R's subsetting would) and the cuts into chunks of CCH cells.
struct ClusterPlan {
    std::vector<int32_t> cells;  // restricted cells (0-based) in the caller's order, empty without restriction
    std::vector<int32_t> order;  // restricted cells (0-based) sorted by cluster, ascending within a cluster
    std::vector<int32_t> chunk_begin, cluster_chunk0, count;
    int64_t n_rows = 0;  // restricted cells, 0 without restriction
};
ClusterPlan cluster_plan_batch(int64_t n, const int32_t* clusters0, int C, const int32_t* restrict_idx, int64_t nr) {
    cluster_check_batch(n, clusters0, C, restrict_idx, nr);
    const bool restricted = is_restricted(restrict_idx, nr);
    ClusterPlan p;
    if (restricted) {
        p.cells.assign(restrict_idx, restrict_idx + nr);
        for (int32_t& v : p.cells) v -= 1;
    }
    std::vector<int32_t> sorted_cells = p.cells;
    std::sort(sorted_cells.begin(), sorted_cells.end());
    const int64_t m = restricted ? nr : n;
    std::vector<int32_t> start((size_t)C + 1, 0);
    p.count.assign((size_t)C, 0);
    for (int64_t i = 0; i < m; ++i) ++p.count[(size_t)clusters0[restricted ? sorted_cells[i] : i]];
    for (int cl = 0; cl < C; ++cl) start[cl + 1] = start[cl] + p.count[cl];
    std::vector<int32_t> fill(start.begin(), start.end() - 1);
    p.order.resize((size_t)m);
    for (int64_t i = 0; i < m; ++i) {
        const int32_t cell = restricted ? sorted_cells[i] : (int32_t)i;
        p.order[(size_t)fill[(size_t)clusters0[cell]]++] = cell;
    }
    p.cluster_chunk0.assign((size_t)C + 1, 0);
    for (int cl = 0; cl < C; ++cl) {
        p.cluster_chunk0[cl] = (int32_t)p.chunk_begin.size();
        for (int32_t b = start[cl]; b < start[cl + 1]; b += CCH) p.chunk_begin.push_back(b);
    }
    p.cluster_chunk0[C] = (int32_t)p.chunk_begin.size();
    p.chunk_begin.push_back(start[C]);
    p.n_rows = restricted ? nr : 0;
    return p;
}

// what a batch keeps on the device besides its cells, dense or CSC
struct ClusterLists {
    DevBuf<double> l2;        // [n] column norms over the handle's genes, empty without cosine normalisation
    DevBuf<int32_t> order;    // restricted cells (0-based) sorted by cluster, ascending within a cluster
    DevBuf<int32_t> chunk_begin, cluster_chunk0, count;
    DevBuf<int32_t> rows;     // restricted cells (0-based) in the caller's order, empty without restriction
    int64_t n_rows = 0;
    int C = 0, nchunks = 0;
    bool cos_norm = false;

    // the plan of a batch of n cells goes up on `stream`, which is idle on return (the plan may go out of scope)
    void put(const ClusterPlan& p, int64_t n, int n_clusters, bool cos, hipStream_t stream) {
        C = n_clusters;
        cos_norm = cos;
        nchunks = p.cluster_chunk0[(size_t)n_clusters];
        n_rows = p.n_rows;
        if (cos_norm) l2.reserve((size_t)n);
        auto up = [&](DevBuf<int32_t>& dst, const std::vector<int32_t>& src) {
            if (src.empty()) return;
            BMX_HIP(hipMemcpyAsync(dst.reserve(src.size()), src.data(), src.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                                   stream));
        };
        up(order, p.order);
        up(chunk_begin, p.chunk_begin);
        up(cluster_chunk0, p.cluster_chunk0);
        up(count, p.count);
        up(rows, p.cells);
        BMX_HIP(hipStreamSynchronize(stream));
    }
};
struct ClusterBatch : ResidentBatch, ClusterLists {};
struct ClusterSparseBatch : CscBatch, ClusterLists {};

// What Cluster and ClusterSparse share: everything but the two kernels that read the cells.  The batches stay resident
// between the centroid pass and the propagation of the centroids' corrections to the cells.
template <class Batch>
class ClusterBase : protected ResidentBatches<Batch> {
  protected:
    using Store = ResidentBatches<Batch>;
    using Store::batches_;
    using Store::cache_;
    using Store::device_;
    using Store::G_;
    using Store::ms_;
    using Store::stream_;
    using Store::timer_;

    // subset: 1-based genes (subset.row) the cosine norms and the projection are taken over, or null / ns = 0 for all
    ClusterBase(int device, int G, const int32_t* subset, int ns, const char* begin_entry) : Store(device, G, begin_entry) {
        if (subset && ns > 0) sub0_host_.assign(subset, subset + ns);
        for (int32_t& s : sub0_host_) s -= 1;
    }
    ~ClusterBase() = default;  // (the handle's own destructor has called retire())

    // part [nchunks][G] = the chunks' sums of batch b (file head, a.), queued on stream_
    virtual void launch_centroid_partial(Batch& b, double* part) = 0;
    // the rotation [nrot() x d] column-major goes to the device in the form the projection reads, before its clock starts
    virtual void stage_rotation(const double* rotation, int d) = 0;
    // cur [n x d] column-major = crossprod(x[subset,], rotation), neither normalised nor centred yet, queued on stream_
    virtual void launch_projection(Batch& b, int d, double* cur) = 0;

  public:
    Batch& batch(int bi) {
        if (bi < 0 || bi >= (int)batches_.size()) throw Error(BMX_ERR_ARG, "batch index out of range");
        Batch& b = *batches_[bi];
        if (b.filled != b.n) throw Error(BMX_ERR_ARG, "the batch has not received all its cells");
        return b;
    }
    int nrot() const { return sub0_host_.empty() ? G_ : (int)sub0_host_.size(); }

    // .compute_centroids (R/clusterMNN.R:231-244): out [G x C_b] column-major host memory
    void centroids(int bi, double* out) {
        Batch& b = batch(bi);
        if (!out) throw Error(BMX_ERR_ARG, "'out' is missing");
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        const int G = G_;
        double* part = part_.reserve((size_t)b.nchunks * G);
        double* cen = cen_.reserve((size_t)b.C * G);
        const int e0 = timer_.mark(stream_);
        launch_centroid_partial(b, part);
        BMX_LAUNCH_CHECK();
        hipLaunchKernelGGL(centroid_reduce_kernel, dim3((unsigned)cdiv(G, 256), (unsigned)b.C), dim3(256), 0, stream_,
                           (const double*)part, G, b.C, (const int32_t*)b.cluster_chunk0.p, (const int32_t*)b.count.p, cen);
        BMX_LAUNCH_CHECK();
        const int e1 = timer_.mark(stream_);
        BMX_HIP(hipMemcpyAsync(out, cen, (size_t)b.C * G * sizeof(double), hipMemcpyDeviceToHost, stream_));
        BMX_HIP(hipStreamSynchronize(stream_));
        timer_.span(1, e0, e1);
        timer_.collect(ms_);
    }

    // .propagate_to_cells for one batch (R/clusterMNN.R:262-282): rotation [rows x d] column-major and centers [rows] over
    // the handle's genes (the subset's, in its order), cpcs / corr (the centroids' coordinates before and after the merge)
    // [C_b x d] column-major, out [n_b x d]
    void propagate(int bi, const double* rotation, int d, const double* centers, const double* cpcs, const double* corr,
                   double* out, double* sigma_out) {
        Batch& b = batch(bi);
        if (d < 1 || d > DMAX) throw Error(BMX_ERR_ARG, "the propagation takes 1 <= d <= 256 columns");
        if (!rotation || !centers || !cpcs || !corr || !out)
            throw Error(BMX_ERR_ARG, "'rotation', 'centers', the centroids' coordinates and 'out' must be given");
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        const int n = (int)b.n, C = b.C;
        const int ns = nrot();
        // pca.center %*% pca.rotation (:271), on the host
        std::vector<double> cu((size_t)d, 0.0);
        for (int j = 0; j < d; ++j) {
            double s = 0.0;
            for (int i = 0; i < ns; ++i) s += centers[i] * rotation[(size_t)j * ns + i];
            cu[(size_t)j] = s;
        }
        stage_rotation(rotation, d);
        double* small = small_.reserve((size_t)d + 2 * (size_t)C * d + 8);
        double* cu_dev = small;       // [d]
        double* cp_dev = cu_dev + d;  // [C x d]
        double* corr_dev = cp_dev + (size_t)C * d;
        double* sigma_dev = corr_dev + (size_t)C * d;
        BMX_HIP(hipMemcpyAsync(cu_dev, cu.data(), (size_t)d * sizeof(double), hipMemcpyHostToDevice, stream_));
        BMX_HIP(hipMemcpyAsync(cp_dev, cpcs, (size_t)C * d * sizeof(double), hipMemcpyHostToDevice, stream_));
        BMX_HIP(hipMemcpyAsync(corr_dev, corr, (size_t)C * d * sizeof(double), hipMemcpyHostToDevice, stream_));
        double* cur = cur_.reserve((size_t)n * d);
        double* W = w_.reserve((size_t)n * C);
        double* dist = dist_.reserve((size_t)n);

        const int e0 = timer_.mark(stream_);
        launch_projection(b, d, cur);
        const int64_t total = (int64_t)n * d;
        hipLaunchKernelGGL(finish_projection_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream_, cur, n, d,
                           (const double*)(b.cos_norm ? b.l2.p : nullptr), (const double*)cu_dev);
        BMX_LAUNCH_CHECK();
        const int e1 = timer_.mark(stream_);
        hipLaunchKernelGGL(nearest_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, stream_, (const double*)cur, n, d,
                           (const double*)cp_dev, C, W, dist);
        BMX_LAUNCH_CHECK();
        hipLaunchKernelGGL(median_select_kernel, dim3(1), dim3(MSEL_T), 0, stream_, (const double*)dist,
                           (const int32_t*)(b.n_rows ? b.rows.p : nullptr), b.n_rows ? b.n_rows : b.n, sigma_dev);
        BMX_LAUNCH_CHECK();
        const int e2 = timer_.mark(stream_);
        const size_t lds = (size_t)C * JT * sizeof(double);
        ensure_dynamic_lds(reinterpret_cast<const void*>(&smooth_kernel), lds);
        hipLaunchKernelGGL(smooth_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), lds, stream_, cur, n, d, W, C,
                           (const double*)cp_dev, (const double*)corr_dev, (const double*)sigma_dev);
        BMX_LAUNCH_CHECK();
        const int e3 = timer_.mark(stream_);
        double sigma = 0.0;
        BMX_HIP(hipMemcpyAsync(&sigma, sigma_dev, sizeof(double), hipMemcpyDeviceToHost, stream_));
        download_pageable(out, cur, (size_t)n * d * sizeof(double), stream_);
        BMX_HIP(hipStreamSynchronize(stream_));
        if (sigma_out) *sigma_out = sigma;
        timer_.span(2, e0, e1);
        timer_.span(3, e1, e2);
        timer_.span(4, e2, e3);
        timer_.collect(ms_);
    }

    // milliseconds since the handle was made: upload (host wall time of the staged copies), then HIP-event time of the
    // centroid pass, the projection, nearest centroid + median, the smoothing
    using Store::stage_ms;

  protected:
    std::vector<int32_t> sub0_host_;  // the subset's genes, 0-based, in its order; empty: all genes

  private:
    DevBuf<double> part_, cen_, small_, cur_, w_, dist_;
};

class Cluster : public ClusterBase<ClusterBatch> {
  public:
    Cluster(int device, int G, const int32_t* subset, int ns) : ClusterBase(device, G, subset, ns, "bmx_cluster_begin_batch") {
        if (!sub0_host_.empty()) {
            CacheScope scope(&cache_);
            BMX_HIP(hipMemcpyAsync(sub0_.reserve(sub0_host_.size()), sub0_host_.data(), sub0_host_.size() * sizeof(int32_t),
                                   hipMemcpyHostToDevice, stream_));
            BMX_HIP(hipStreamSynchronize(stream_));
        }
    }
    ~Cluster() { retire(); }

    // a batch of n cells: clusters0 [n] 0-based cluster ids below C, restrict_idx 1-based cells (null / nr < 0: all);
    // its columns follow in one or more blocks, in order
    void begin_batch(int64_t n, const int32_t* clusters0, int C, const int32_t* restrict_idx, int64_t nr, bool cos_norm) {
        const ClusterPlan plan = cluster_plan_batch(n, clusters0, C, restrict_idx, nr);
        begin(n, [&](ClusterBatch& b) { b.put(plan, n, C, cos_norm, stream_); });
    }

    void add_block(const double* x_block, int64_t m) {
        const double t0 = now_ms();
        add(x_block, m, [&](ClusterBatch& b, double* p) {
            if (b.cos_norm) {
                double* l2 = b.l2.p + (b.filled - m);
                cell_l2_device(stream_, p, G_, m, sub0_host_.empty() ? nullptr : sub0_.p, (int)sub0_host_.size(), false, l2);
            }
            if (b.complete()) BMX_HIP(hipStreamSynchronize(stream_));
        });
        ms_[0] += now_ms() - t0;
    }

  private:
    void launch_centroid_partial(ClusterBatch& b, double* part) override {
        hipLaunchKernelGGL(centroid_partial_kernel, dim3((unsigned)b.nchunks, (unsigned)cdiv(G_, 256)), dim3(256), 0, stream_,
                           (const double*)b.x.p, G_, (const double*)(b.cos_norm ? b.l2.p : nullptr),
                           (const int32_t*)b.order.p, (const int32_t*)b.chunk_begin.p, part);
    }
    // the rotation over all genes (zero outside the subset), column-major, and what cosnorm_project_device wants besides
    void stage_rotation(const double* rotation, int d) override {
        const int G = G_, ns = nrot();
        std::vector<double> ufull((size_t)G * d, 0.0);
        for (int j = 0; j < d; ++j)
            for (int i = 0; i < ns; ++i) {
                const int g = sub0_host_.empty() ? i : sub0_host_[(size_t)i];
                ufull[(size_t)j * G + g] += rotation[(size_t)j * ns + i];
            }
        double* U = u_.reserve((size_t)G * d);
        double* zero = zero_.reserve((size_t)G + (size_t)d);  // [G] centres of 0: the centring follows; [d] scratch
        upload_pageable(U, ufull.data(), ufull.size() * sizeof(double), stream_);
        BMX_HIP(hipMemsetAsync(zero, 0, (size_t)G * sizeof(double), stream_));
    }
    void launch_projection(ClusterBatch& b, int d, double* cur) override {
        cosnorm_project_device(stream_, b.x.p, G_, (int)b.n, u_.p, d, zero_.p, 0, cur, nullptr, zero_.p + G_);
    }

    DevBuf<int32_t> sub0_;
    DevBuf<double> u_, zero_;
};

// The same over batches kept as CSC (file head).
class ClusterSparse : public ClusterBase<ClusterSparseBatch> {
  public:
    ClusterSparse(int device, int G, const int32_t* subset, int ns)
        : ClusterBase(device, G, subset, ns, "bmx_cluster_sparse_begin_batch") {
        CacheScope scope(&cache_);
        BMX_HIP(hipMemsetAsync(flags_.reserve(CSC_F_WORDS), 0, CSC_F_WORDS * sizeof(int32_t), stream_));
        if (!sub0_host_.empty()) {  // how often every gene is in the subset: what the cells' norms take instead of the list
            std::vector<int32_t> mult((size_t)G, 0);
            for (int32_t g : sub0_host_) ++mult[(size_t)g];
            BMX_HIP(hipMemcpyAsync(mult_.reserve((size_t)G), mult.data(), (size_t)G * sizeof(int32_t), hipMemcpyHostToDevice,
                                   stream_));
        }
        BMX_HIP(hipStreamSynchronize(stream_));
    }
    ~ClusterSparse() { retire(); }

    // Cluster::begin_batch for a batch with nnz stored entries in all
    void begin_batch(int64_t n, int64_t nnz, const int32_t* clusters0, int C, const int32_t* restrict_idx, int64_t nr,
                     bool cos_norm) {
        const ClusterPlan plan = cluster_plan_batch(n, clusters0, C, restrict_idx, nr);
        begin_csc(n, nnz, [&](ClusterSparseBatch& b) { b.put(plan, n, C, cos_norm, stream_); });
    }

    // the next m cells of the batch begun last: indptr [m + 1] relative to the block, its nnz entries
    void add_block(int64_t m, const int64_t* indptr, const int32_t* indices, const double* data, int64_t nnz) {
        const double t0 = now_ms();
        add_csc(m, indptr, indices, data, nnz, [&](ClusterSparseBatch& b, int64_t c0) {
            hipLaunchKernelGGL(csp_prepare_kernel, dim3((unsigned)cdiv(m, 4)), dim3(256), 0, stream_,
                               (const int64_t*)b.indptr.p, (const int32_t*)b.indices.p, (const double*)b.data.p, G_, c0, m,
                               (const int32_t*)(sub0_host_.empty() ? nullptr : mult_.p), b.cos_norm ? b.l2.p : nullptr,
                               flags_.p);
            BMX_LAUNCH_CHECK();
            if (b.complete()) BMX_HIP(hipStreamSynchronize(stream_));
        });
        ms_[0] += now_ms() - t0;
    }

    void centroids(int bi, double* out) {
        refuse_bad_pattern();
        ClusterBase::centroids(bi, out);
    }
    void propagate(int bi, const double* rotation, int d, const double* centers, const double* cpcs, const double* corr,
                   double* out, double* sigma_out) {
        refuse_bad_pattern();
        ClusterBase::propagate(bi, rotation, d, centers, cpcs, corr, out, sigma_out);
    }

  private:
    // what csp_prepare_kernel has seen of the patterns uploaded so far
    void refuse_bad_pattern() {
        BMX_HIP(hipSetDevice(device_));
        int32_t flags[CSC_F_WORDS] = {0, 0};
        BMX_HIP(hipMemcpyAsync(flags, flags_.p, sizeof(flags), hipMemcpyDeviceToHost, stream_));
        BMX_HIP(hipStreamSynchronize(stream_));
        throw_if_bad_pattern(flags);
    }
    void launch_centroid_partial(ClusterSparseBatch& b, double* part) override {
        hipLaunchKernelGGL(csp_centroid_partial_kernel, dim3((unsigned)b.nchunks, (unsigned)cdiv(G_, SGT)), dim3(256), 0,
                           stream_, (const int64_t*)b.indptr.p, (const int32_t*)b.indices.p, (const double*)b.data.p, G_,
                           (const double*)(b.cos_norm ? b.l2.p : nullptr), (const int32_t*)b.order.p,
                           (const int32_t*)b.chunk_begin.p, part);
    }
    // the rotation over all genes (zero outside the subset), row-major with the columns filled up to a multiple of 64
    void stage_rotation(const double* rotation, int d) override {
        const int G = G_, ns = nrot();
        ldr_ = (int64_t)cdiv(d, 64) * 64;
        std::vector<double> rfull((size_t)G * ldr_, 0.0);
        for (int j = 0; j < d; ++j)
            for (int i = 0; i < ns; ++i) {
                const int g = sub0_host_.empty() ? i : sub0_host_[(size_t)i];
                rfull[(size_t)g * ldr_ + j] += rotation[(size_t)j * ns + i];
            }
        upload_pageable(r_.reserve(rfull.size()), rfull.data(), rfull.size() * sizeof(double), stream_);
    }
    void launch_projection(ClusterSparseBatch& b, int d, double* cur) override {
        hipLaunchKernelGGL(csp_project_kernel, dim3((unsigned)cdiv(b.n, PCELLS)), dim3(256), 0, stream_,
                           (const int64_t*)b.indptr.p, (const int32_t*)b.indices.p, (const double*)b.data.p, b.n, G_,
                           (const double*)r_.p, ldr_, d, cur);
        BMX_LAUNCH_CHECK();
    }

    DevBuf<int32_t> mult_, flags_;
    DevBuf<double> r_;
    int64_t ldr_ = 0;
};

}  // namespace bmx

/* ---------------------------------------------------------------- bmx_cluster_* --------------------------------- */
struct bmx_cluster final : bmx::Cluster {
    using Cluster::Cluster;
};

extern "C" {

int32_t bmx_cluster_create(int32_t device, int32_t G, const int32_t* subset_row, int32_t n_subset_row, bmx_cluster_t** out) {
    return bmx::guarded([&] {
        bmx::check_cluster_create(G, subset_row, n_subset_row, out);
        *out = new bmx_cluster(device, G, subset_row, n_subset_row);
    });
}

void bmx_cluster_destroy(bmx_cluster_t* h) { delete h; }

int32_t bmx_cluster_begin_batch(bmx_cluster_t* h, int64_t n, const int32_t* clusters0, int32_t n_clusters,
                                const int32_t* restrict_idx, int64_t n_restrict, int32_t cos_norm) {
    return bmx::guarded([&] {
        bmx::live(h).begin_batch(n, clusters0, n_clusters, restrict_idx, n_restrict, cos_norm != 0);
    });
}

int32_t bmx_cluster_add_block(bmx_cluster_t* h, const double* x_block, int64_t n_block) {
    return bmx::guarded([&] { bmx::live(h).add_block(x_block, n_block); });
}

int32_t bmx_cluster_add_batch(bmx_cluster_t* h, const double* x, int64_t n, const int32_t* clusters0, int32_t n_clusters,
                              const int32_t* restrict_idx, int64_t n_restrict, int32_t cos_norm) {
    return bmx::guarded([&] {
        if (!x) throw bmx::Error(BMX_ERR_ARG, "the batch is missing");
        bmx::live(h).begin_batch(n, clusters0, n_clusters, restrict_idx, n_restrict, cos_norm != 0);
        h->add_block(x, n);
    });
}

int32_t bmx_cluster_centroids(bmx_cluster_t* h, int32_t batch, double* out) {
    return bmx::guarded([&] { bmx::live(h).centroids(batch, out); });
}

int32_t bmx_cluster_propagate(bmx_cluster_t* h, int32_t batch, const double* rotation, int32_t d, const double* centers,
                              const double* centroid_pcs, const double* corrected_pcs, double* out, double* sigma_out) {
    return bmx::guarded([&] {
        bmx::live(h).propagate(batch, rotation, d, centers, centroid_pcs, corrected_pcs, out, sigma_out);
    });
}

int32_t bmx_cluster_stage_ms(const bmx_cluster_t* h, double* out5) {
    return bmx::guarded([&] {
        if (!h || !out5) throw bmx::Error(BMX_ERR_ARG, "null argument");
        h->stage_ms(out5);
    });
}

}  // extern "C"

/* ---------------------------------------------------------------- bmx_cluster_sparse_* -------------------------- */
struct bmx_cluster_sparse final : bmx::ClusterSparse {
    using ClusterSparse::ClusterSparse;
};

extern "C" {

int32_t bmx_cluster_sparse_create(int32_t device, int32_t G, const int32_t* subset_row, int32_t n_subset_row,
                                  bmx_cluster_sparse_t** out) {
    return bmx::guarded([&] {
        bmx::check_cluster_create(G, subset_row, n_subset_row, out);
        *out = new bmx_cluster_sparse(device, G, subset_row, n_subset_row);
    });
}

void bmx_cluster_sparse_destroy(bmx_cluster_sparse_t* h) { delete h; }

int32_t bmx_cluster_sparse_begin_batch(bmx_cluster_sparse_t* h, int64_t n, int64_t nnz, const int32_t* clusters0,
                                       int32_t n_clusters, const int32_t* restrict_idx, int64_t n_restrict, int32_t cos_norm) {
    return bmx::guarded([&] {
        bmx::live(h).begin_batch(n, nnz, clusters0, n_clusters, restrict_idx, n_restrict, cos_norm != 0);
    });
}

int32_t bmx_cluster_sparse_add_block(bmx_cluster_sparse_t* h, int64_t n_block, const int64_t* indptr, const int32_t* indices,
                                     const double* data, int64_t nnz) {
    return bmx::guarded([&] { bmx::live(h).add_block(n_block, indptr, indices, data, nnz); });
}

int32_t bmx_cluster_sparse_centroids(bmx_cluster_sparse_t* h, int32_t batch, double* out) {
    return bmx::guarded([&] { bmx::live(h).centroids(batch, out); });
}

int32_t bmx_cluster_sparse_propagate(bmx_cluster_sparse_t* h, int32_t batch, const double* rotation, int32_t d,
                                     const double* centers, const double* centroid_pcs, const double* corrected_pcs,
                                     double* out, double* sigma_out) {
    return bmx::guarded([&] {
        bmx::live(h).propagate(batch, rotation, d, centers, centroid_pcs, corrected_pcs, out, sigma_out);
    });
}

int32_t bmx_cluster_sparse_stage_ms(const bmx_cluster_sparse_t* h, double* out5) {
    return bmx::guarded([&] {
        if (!h || !out5) throw bmx::Error(BMX_ERR_ARG, "null argument");
        h->stage_ms(out5);
    });
}

}  // extern "C"
