// The exact FP64 paths of the kNN (knn.hip) for what the candidate tiers leave over, or do not take at all:
//   the bounded sweep  knn_exact_filter + knn_exact_pick (launch_bounded_sweep): the references within each listed query's
//                      k-th candidate distance, a handful per query;
//   the full scan      knn_exact_dist + knn_exact_select / knn_exact_select_big (launch_full_scan);
//   exact_search       the first, then the second for what overflowed -- or the second alone.
#include "knn_fp64.hpp"
#include "knn_internal.hpp"

#include <algorithm>

namespace bmx {
namespace {

// ---------------------------------------------------------------------------------------------------
// 4. exact FP64 scan for flagged queries (or every query when the MFMA path does not apply), in batches:
//    knn_exact_dist   -- grid (tiles of 64 references, tiles of 64 queries of the batch): all exact squared distances, spread
//                        over the whole chip even when only a handful of queries are flagged;
//    knn_exact_select -- one workgroup per query: k rounds of block-wide (distance, index) minimum.
// ---------------------------------------------------------------------------------------------------
// A tile of 64 references x 64 queries of the batch per workgroup, the rows staged through the LDS 32 columns at a time; a thread
// holds 4 x 4 pairs.  Every pair's sum runs over the columns left to right, one subtraction, one product, one addition each
// (compiled with -ffp-contract=off): exact_d2's value bit for bit.  (Until late in round 6 a thread took ONE pair and read both
// its rows itself: 1.2 KB of L2 traffic a pair at 150 columns, 555 ms for 20 000 queries against 100 000 cells.)
constexpr int XDT = 64;   // rows of a tile, both ways
constexpr int XDC = 32;   // columns staged at a time
__global__ __launch_bounds__(256) void knn_exact_dist(const double* __restrict__ X, const int32_t* __restrict__ ref_rows,
                                                      int nr, const double* __restrict__ Q,
                                                      const int32_t* __restrict__ q_rows, int d,
                                                      const int32_t* __restrict__ flagged, int f0, int nb,
                                                      double* __restrict__ drow, int dev_cap = 0) {
    // (dev_cap > 0: the number of listed queries is on the device -- flagged[0], at most dev_cap of them are taken --, the grid
    // is made for dev_cap and the tiles beyond the count end here)
    if (dev_cap > 0) nb = min(flagged[0], dev_cap);
    const int q0 = blockIdx.y * XDT, r0 = blockIdx.x * XDT;
    if (q0 >= nb) return;
    __shared__ double Qs_[XDT][XDC + 1], Xs_[XDT][XDC + 1];
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int lr = tid >> 2, lc = (tid & 3) * 8;  // this thread stages 8 columns of row lr of either tile
    const double* qp = nullptr;
    const double* xp = nullptr;
    if (q0 + lr < nb) {
        const int f = f0 + q0 + lr;
        const int q = flagged ? flagged[1 + f] : f;
        qp = Q + (int64_t)(q_rows ? q_rows[q] : q) * d;
    }
    if (r0 + lr < nr) xp = X + (int64_t)(ref_rows ? ref_rows[r0 + lr] : r0 + lr) * d;
    double s[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j2 = 0; j2 < 4; ++j2) s[i][j2] = 0.0;
    for (int c0 = 0; c0 < d; c0 += XDC) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = c0 + lc + e;
            Qs_[lr][lc + e] = (qp && c < d) ? qp[c] : 0.0;
            Xs_[lr][lc + e] = (xp && c < d) ? xp[c] : 0.0;
        }
        __syncthreads();
        const int cmax = d - c0 < XDC ? d - c0 : XDC;
        for (int c = 0; c < cmax; ++c) {
            double qv[4], xv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) qv[i] = Qs_[ty * 4 + i][c];
#pragma unroll
            for (int j2 = 0; j2 < 4; ++j2) xv[j2] = Xs_[tx * 4 + j2][c];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j2 = 0; j2 < 4; ++j2) {
                    const double t = qv[i] - xv[j2];
                    s[i][j2] += t * t;
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int qi = q0 + ty * 4 + i;
        if (qi >= nb) continue;
#pragma unroll
        for (int j2 = 0; j2 < 4; ++j2) {
            const int r = r0 + tx * 4 + j2;
            if (r < nr) drow[(int64_t)qi * nr + r] = s[i][j2];
        }
    }
}

// k <= 256: TWO sweeps of the row instead of k.  The k-th smallest of the 256 threads' own minima bounds the k-th smallest of the
// row from above (k different entries lie at or below it); the entries at or below that bound -- about k (1 + k / 256) of them --
// are collected in the LDS and sorted by (distance, position).  More than XS2_CAP of them (a row of equal distances): the k
// rounds below.
constexpr int XS2_CAP = 2048;
__device__ __forceinline__ void knn_exact_select_rounds(const double* __restrict__ row, int nr, int k, int q,
                                                        int32_t* __restrict__ idx_out, double* __restrict__ dist_out, int sq,
                                                        double* rd, int* ri);

__global__ __launch_bounds__(256) void knn_exact_select(const double* __restrict__ drow, int nr, int k,
                                                        const int32_t* __restrict__ flagged, int f0,
                                                        int32_t* __restrict__ idx_out, double* __restrict__ dist_out,
                                                        int dev_cap = 0, int sq = 0) {
    __shared__ double sd[XS2_CAP];
    __shared__ int si[XS2_CAP];
    __shared__ double tau_sh;
    __shared__ int cnt_sh;
    if (dev_cap > 0 && (int)blockIdx.x >= min(flagged[0], dev_cap)) return;  // (see knn_exact_dist)
    const int tid = threadIdx.x;
    const int f = f0 + blockIdx.x;
    const int q = flagged ? flagged[1 + f] : f;
    const double* row = drow + (int64_t)blockIdx.x * nr;
    if (k <= 256) {
        double m = __builtin_inf();
        for (int r = tid; r < nr; r += 256) m = fmin(m, row[r]);
        sd[tid] = m;
        if (tid == 0) cnt_sh = 0;
        __syncthreads();
        int rank = 0;
        for (int t = 0; t < 256; ++t) rank += (sd[t] < m || (sd[t] == m && t < tid)) ? 1 : 0;
        if (rank == k - 1) tau_sh = m;  // (k <= nr: at least k threads hold an entry)
        __syncthreads();
        const double tau = tau_sh;
        __syncthreads();  // (sd is reused)
        for (int r = tid; r < nr; r += 256) {
            const double v = row[r];
            if (v <= tau) {
                const int at = atomicAdd(&cnt_sh, 1);
                if (at < XS2_CAP) {
                    sd[at] = v;
                    si[at] = r;
                }
            }
        }
        __syncthreads();
        const int n = cnt_sh;
        if (n <= XS2_CAP) {
            int np2 = 64;
            while (np2 < n) np2 <<= 1;
            for (int i = n + tid; i < np2; i += 256) {
                sd[i] = __builtin_inf();
                si[i] = 0x7FFFFFFF;
            }
            __syncthreads();
            block_bitonic_sort<256>(sd, si, np2);
            for (int j = tid; j < k; j += 256) {
                idx_out[(int64_t)q * k + j] = si[j];
                if (dist_out) dist_out[(int64_t)q * k + j] = sq ? sd[j] : sqrt(sd[j]);
            }
            return;
        }
        __syncthreads();
    }
    knn_exact_select_rounds(row, nr, k, q, idx_out, dist_out, sq, sd, si);
}

__device__ __forceinline__ void knn_exact_select_rounds(const double* __restrict__ row, int nr, int k, int q,
                                                        int32_t* __restrict__ idx_out, double* __restrict__ dist_out, int sq,
                                                        double* rd, int* ri) {
    const int tid = threadIdx.x;
    double last_d = -1.0;  // squared distances are >= 0
    int last_i = -1;
    for (int jdx = 0; jdx < k; ++jdx) {
        double bd = __builtin_inf();
        int bi = 0x7FFFFFFF;
        for (int r = tid; r < nr; r += 256) {
            const double v = row[r];
            if (key_less(last_d, last_i, v, r) && key_less(v, r, bd, bi)) {
                bd = v;
                bi = r;
            }
        }
        rd[tid] = bd;
        ri[tid] = bi;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o && key_less(rd[tid + o], ri[tid + o], rd[tid], ri[tid])) {
                rd[tid] = rd[tid + o];
                ri[tid] = ri[tid + o];
            }
            __syncthreads();
        }
        last_d = rd[0];
        last_i = ri[0];
        if (tid == 0) {
            idx_out[(int64_t)q * k + jdx] = last_i;
            if (dist_out) dist_out[(int64_t)q * k + jdx] = sq ? last_d : sqrt(last_d);
        }
        __syncthreads();
    }
}

// The same selection for k > 64 (prop.k runs; the k rounds above are 69 ms a query at k = 1 000 over 100 000 references,
// however few queries there are -- a query is one workgroup).  Squared distances are >= 0, so they order like their bit
// patterns: a bisection over the patterns finds the k-th smallest value T (<= 63 counting sweeps of the row, which stays in
// L2), a bisection over the positions finds how far into the references equal to T the list reaches (ties rank by position,
// as above), the k chosen entries are compacted into LDS and sorted by (distance, position).
constexpr int XSB_T = 1024;
constexpr int XSB_MAXK = 8192;

__device__ __forceinline__ int xsb_block_sum(int v, int* sh_part) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();  // (sh_part is read by everyone at the end of the previous call)
    if ((threadIdx.x & 63) == 0) sh_part[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
    for (int w = 0; w < XSB_T / 64; ++w) s += sh_part[w];
    return s;
}

__global__ __launch_bounds__(XSB_T) void knn_exact_select_big(const double* __restrict__ drow, int nr, int k, int np2,
                                                              const int32_t* __restrict__ flagged, int f0,
                                                              int32_t* __restrict__ idx_out, double* __restrict__ dist_out,
                                                              int dev_cap = 0, int sq = 0) {
    extern __shared__ double xsb_d[];       // [np2] distances, then [np2] positions
    if (dev_cap > 0 && (int)blockIdx.x >= min(flagged[0], dev_cap)) return;  // (see knn_exact_dist)
    int* xsb_i = reinterpret_cast<int*>(xsb_d + np2);
    __shared__ int sh_part[XSB_T / 64];
    __shared__ int sh_fill;
    const int tid = threadIdx.x;
    const int f = f0 + blockIdx.x;
    const int q = flagged ? flagged[1 + f] : f;
    const double* row = drow + (int64_t)blockIdx.x * nr;
    // the k-th smallest pattern (NaN patterns lie above +inf's and are never counted; the caller has k <= nr finite rows)
    unsigned long long lo = 0, hi = 0x7FF0000000000000ull;
    while (lo < hi) {
        const unsigned long long mid = lo + ((hi - lo) >> 1);
        int c = 0;
        for (int r = tid; r < nr; r += XSB_T) c += (unsigned long long)__double_as_longlong(row[r]) <= mid ? 1 : 0;
        if (xsb_block_sum(c, sh_part) >= k) hi = mid;
        else lo = mid + 1;
    }
    const unsigned long long T = lo;
    int c = 0;
    for (int r = tid; r < nr; r += XSB_T) c += (unsigned long long)__double_as_longlong(row[r]) < T ? 1 : 0;
    const int need = k - xsb_block_sum(c, sh_part);  // >= 1 entries equal to T, the first in position order
    int plo = 0, phi = nr - 1;  // smallest position P with `need` entries equal to T at or before it
    while (plo < phi) {
        const int mid = plo + ((phi - plo) >> 1);
        int e = 0;
        for (int r = tid; r <= mid; r += XSB_T) e += (unsigned long long)__double_as_longlong(row[r]) == T ? 1 : 0;
        if (xsb_block_sum(e, sh_part) >= need) phi = mid;
        else plo = mid + 1;
    }
    const int P = plo;
    if (tid == 0) sh_fill = 0;
    for (int i = tid; i < np2; i += XSB_T) {
        xsb_d[i] = __builtin_inf();
        xsb_i[i] = 0x7FFFFFFF;
    }
    __syncthreads();
    for (int r = tid; r < nr; r += XSB_T) {
        const double v = row[r];
        const unsigned long long b = (unsigned long long)__double_as_longlong(v);
        if (b < T || (b == T && r <= P)) {
            const int at = atomicAdd(&sh_fill, 1);
            if (at < np2) {
                xsb_d[at] = v;
                xsb_i[at] = r;
            }
        }
    }
    __syncthreads();
    block_bitonic_sort<XSB_T>(xsb_d, xsb_i, np2);
    for (int j = tid; j < k; j += XSB_T) {
        idx_out[(int64_t)q * k + j] = xsb_i[j];
        if (dist_out) dist_out[(int64_t)q * k + j] = sq ? xsb_d[j] : sqrt(xsb_d[j]);
    }
}

// ---------------------------------------------------------------------------------------------------
// 4b. fast exact path for a FEW flagged queries: the k-th candidate distance bounds the true k-th neighbour from
//     above, so one pass that stages each reference tile once in LDS, evaluates it against every flagged query in
//     FP64 and keeps the references within that bound (a handful per query) replaces the full per-query rescan.
//     A query whose list overflows (massive exact ties) is handed to the full scan.
// ---------------------------------------------------------------------------------------------------
constexpr int XF_TILE = 64;    // reference rows per staged tile
constexpr int XF_QCH = 16;     // flagged queries staged at a time
constexpr int XF_CAP = 256;    // kept references per flagged query

__global__ __launch_bounds__(256) void knn_exact_filter(const double* __restrict__ X,
                                                        const int32_t* __restrict__ ref_rows, int nr,
                                                        const double* __restrict__ Q,
                                                        const int32_t* __restrict__ q_rows, int d,
                                                        const int32_t* __restrict__ flagged,
                                                        const double* __restrict__ flag_bound, int nflag, int dev_cap,
                                                        int32_t* __restrict__ xcnt, double* __restrict__ xd,
                                                        int32_t* __restrict__ xi) {
    extern __shared__ __attribute__((aligned(16))) char smem_x[];
    if (dev_cap > 0) {  // launched without the host knowing the count: nothing flagged (the rule) -> nothing staged
        nflag = flagged[0];
        if (nflag <= 0 || nflag > dev_cap) return;  // (more than the cap: knn_exact_pick raises the run's invalid flag)
    }
    // Tiles of 64 reference rows through the LDS: a wave copies a row per instruction (lanes along the row: 16-byte pieces
    // where the rows allow, one coalesced read of its 8 d bytes), then every thread takes one row of the tile against every
    // flagged query -- exact_d2's sum, left to right.  (Round 3 staged element by element with an integer division per
    // double: 380 us for a sweep of 700 000 rows that moves 280 MB; a thread per row straight from global memory: worse,
    // 64 cache lines per load instruction.)
    double* xs = reinterpret_cast<double*>(smem_x);  // [XF_TILE][d + 1]  (+1: breaks the bank stride)
    const int ld = d + 1;
    double* qs = xs + XF_TILE * ld;                  // [XF_QCH][d + 1] flagged queries
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const bool wide = (d & 1) == 0;
    const int np = wide ? d >> 1 : d;  // pieces per row
    for (int r0 = blockIdx.x * XF_TILE; r0 < nr; r0 += gridDim.x * XF_TILE) {
        const int rows_here = min(XF_TILE, nr - r0);
        if (wide && np <= 64) {
            // all 16 rows of this wave asked for before the first is stored: their round trips overlap
            typedef double d2 __attribute__((ext_vector_type(2)));
            d2 v[XF_TILE / 4];
#pragma unroll
            for (int i = 0; i < XF_TILE / 4; ++i) {
                const int rr = w + 4 * i;
                v[i] = d2{0.0, 0.0};
                if (rr < rows_here && lane < np)
                    v[i] = reinterpret_cast<const d2*>(X + (int64_t)(ref_rows ? ref_rows[r0 + rr] : r0 + rr) * d)[lane];
            }
#pragma unroll
            for (int i = 0; i < XF_TILE / 4; ++i) {
                const int rr = w + 4 * i;
                if (rr < rows_here && lane < np) {
                    xs[rr * ld + 2 * lane] = v[i][0];
                    xs[rr * ld + 2 * lane + 1] = v[i][1];
                }
            }
        } else {
            for (int rr = w; rr < rows_here; rr += 4) {
                const double* src = X + (int64_t)(ref_rows ? ref_rows[r0 + rr] : r0 + rr) * d;
                for (int p = lane; p < np; p += 64) {
                    if (wide) {
                        typedef double d2 __attribute__((ext_vector_type(2)));
                        const d2 v = reinterpret_cast<const d2*>(src)[p];
                        xs[rr * ld + 2 * p] = v[0];
                        xs[rr * ld + 2 * p + 1] = v[1];
                    } else {
                        xs[rr * ld + p] = src[p];
                    }
                }
            }
        }
        __syncthreads();
        const int rr = tid & (XF_TILE - 1);
        const double* xr = xs + rr * ld;
        // the flagged queries, XF_QCH at a time, through the LDS as well: read from global memory inside the sum, every one of
        // the d steps of every thread's chain waited for an L2 round trip (0.8 ms per config-3 step for ~25 queries)
        for (int f0 = 0; f0 < nflag; f0 += XF_QCH) {
            const int nq_here = min(XF_QCH, nflag - f0);
            for (int e = tid; e < nq_here * d; e += 256) {
                const int fq = e / d, c = e - fq * d;
                const int q = flagged[1 + f0 + fq];
                qs[fq * ld + c] = Q[(int64_t)(q_rows ? q_rows[q] : q) * d + c];
            }
            __syncthreads();
            for (int fq = tid / XF_TILE; fq < nq_here && rr < rows_here; fq += 256 / XF_TILE) {
                const double* qv = qs + fq * ld;
                double s = 0.0;
                for (int c = 0; c < d; ++c) {
                    const double t = qv[c] - xr[c];
                    s += t * t;
                }
                const int f = f0 + fq;
                if (s <= flag_bound[f]) {
                    const int pos = atomicAdd(&xcnt[f], 1);
                    if (pos < XF_CAP) {
                        xd[(int64_t)f * XF_CAP + pos] = s;
                        xi[(int64_t)f * XF_CAP + pos] = r0 + rr;
                    }
                }
            }
            __syncthreads();
        }
        __syncthreads();  // the tile is restaged
    }
}

// one wave per flagged query: exact (distance, index) ranking of its short list; overflowed lists go to `slow`.
// dev_cap > 0: launched without the host knowing the count (optimistic run): the count is flagged[0]; a count beyond the
// cap or a list that overflowed cannot be handled here and raises opt[0] (the engine then repeats the run with host-checked
// searches); opt[1] accumulates the queries that came this way; the counters of the lists are left zeroed for the next use.
__global__ __launch_bounds__(256) void knn_exact_pick(const int32_t* __restrict__ flagged, int nflag, int dev_cap, int k,
                                                      int seeded, int32_t* __restrict__ xcnt, const double* __restrict__ xd,
                                                      const int32_t* __restrict__ xi, int32_t* __restrict__ idx_out,
                                                      double* __restrict__ dist_out, int32_t* __restrict__ slow,
                                                      int32_t* __restrict__ opt, int sq = 0) {
    const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (dev_cap > 0) {
        nflag = flagged[0];
        if (blockIdx.x == 0 && threadIdx.x == 0 && nflag > 0) {
            atomicAdd(&opt[1], nflag);
            if (nflag > dev_cap) opt[0] = 1;
        }
        if (nflag > dev_cap) {
            // (the run is given up -- but the searches queued behind this one still run, and their sweeps count into these
            // slots: left as they are, a later row would hold a reference twice, its merge (lk_merge_wave) two candidates of one
            // rank and an entry nobody wrote)
            if (f < dev_cap && lane == 0) xcnt[f] = 0;
            return;
        }
    }
    if (f >= nflag) return;
    const int q = flagged[1 + f];
    const int n = xcnt[f];
    if (dev_cap > 0 && lane == 0) xcnt[f] = 0;
    // fewer than k within the bound: only a seeded row (exactly the references within its seed distance: a short row,
    // padded with -1, is what the caller asked for); otherwise it cannot happen (the k candidates themselves qualify)
    const bool short_ok = seeded && n < k && n <= XF_CAP;
    if (n > XF_CAP || (n < k && !short_ok)) {
        if (lane == 0) {
            if (dev_cap > 0) {
                opt[0] = 1;
            } else {
                const int pos = atomicAdd(&slow[0], 1);
                slow[1 + pos] = q;
            }
        }
        return;
    }
    const double* dd = xd + (int64_t)f * XF_CAP;
    const int32_t* ii = xi + (int64_t)f * XF_CAP;
    for (int m = lane; m < n; m += 64) {
        const double dm = dd[m];
        const int im = ii[m];
        int rank = 0;
        for (int t = 0; t < n; ++t) rank += key_less(dd[t], ii[t], dm, im) ? 1 : 0;
        if (rank < k) {
            idx_out[(int64_t)q * k + rank] = im;
            if (dist_out) dist_out[(int64_t)q * k + rank] = sq ? dm : sqrt(dm);
        }
    }
    if (short_ok)
        for (int m = n + lane; m < k; m += 64) idx_out[(int64_t)q * k + m] = -1;
}

}  // namespace

int32_t* launch_bounded_sweep(hipStream_t stream, KnnWorkspace& ws, const double* X, const int32_t* ref_rows, int nr,
                              const double* Qs, const int32_t* qrs, int d, int k, int32_t* io, double* dout,
                              const int32_t* list, const double* bounds, int count, int dev_cap, bool seeded, int32_t* opt) {
    const int n = dev_cap > 0 ? dev_cap : count;  // lists to hold, and what the grid of the pick is made for
    int32_t* xcnt = ws.xcnt.reserve((size_t)n);
    double* xd = ws.xd.reserve((size_t)n * XF_CAP);
    int32_t* xi = ws.xi.reserve((size_t)n * XF_CAP);
    int32_t* slow = nullptr;
    if (dev_cap > 0) {  // (knn_exact_pick leaves the counters it used zeroed)
        if (!ws.xcnt_clear) {
            BMX_HIP(hipMemsetAsync(xcnt, 0, (size_t)n * sizeof(int32_t), stream));
            ws.xcnt_clear = true;
        }
    } else {
        slow = ws.slow.reserve((size_t)count + 1);
        ws.xcnt_clear = false;  // (the lists' counters are left as the sweep filled them)
        BMX_HIP(hipMemsetAsync(xcnt, 0, (size_t)count * sizeof(int32_t), stream));
        BMX_HIP(hipMemsetAsync(slow, 0, sizeof(int32_t), stream));
    }
    const int nflag = dev_cap > 0 ? 0 : count;
    const size_t lds = (size_t)(XF_TILE + XF_QCH) * (d + 1) * sizeof(double);
    ensure_dynamic_lds(reinterpret_cast<const void*>(&knn_exact_filter), lds);
    hipLaunchKernelGGL(knn_exact_filter, dim3(std::min(cdiv(nr, XF_TILE), 2048)), dim3(256), lds, stream, X, ref_rows, nr, Qs, qrs,
                       d, list, bounds, nflag, dev_cap, xcnt, xd, xi);
    BMX_LAUNCH_CHECK();
    hipLaunchKernelGGL(knn_exact_pick, dim3(cdiv(n, 4)), dim3(256), 0, stream, list, nflag, dev_cap, k, seeded ? 1 : 0, xcnt, xd,
                       xi, io, dout, slow, opt, ws.dist_squared ? 1 : 0);
    BMX_LAUNCH_CHECK();
    return slow;
}

void launch_full_scan(hipStream_t stream, KnnWorkspace& ws, const double* X, const int32_t* ref_rows, int nr,
                      const double* Qs, const int32_t* qrs, int d, int k, int32_t* io, double* dout, const int32_t* list,
                      int f0, int nb, int dev_cap, double* drow) {
    const int n = dev_cap > 0 ? dev_cap : nb;  // what the grids are made for
    const int nb_arg = dev_cap > 0 ? 0 : nb;
    const int sq = ws.dist_squared ? 1 : 0;
    hipLaunchKernelGGL(knn_exact_dist, dim3(cdiv(nr, XDT), cdiv(n, XDT)), dim3(256), 0, stream, X, ref_rows, nr, Qs, qrs, d, list,
                       f0, nb_arg, drow, dev_cap);
    BMX_LAUNCH_CHECK();
    if (k > 256 && k <= XSB_MAXK) {
        int np2 = 128;
        while (np2 < k) np2 <<= 1;
        const size_t lds = (size_t)np2 * (sizeof(double) + sizeof(int));
        ensure_dynamic_lds(reinterpret_cast<const void*>(&knn_exact_select_big), lds);
        hipLaunchKernelGGL(knn_exact_select_big, dim3(n), dim3(XSB_T), lds, stream, (const double*)drow, nr, k, np2, list, f0, io,
                           dout, dev_cap, sq);
    } else {
        hipLaunchKernelGGL(knn_exact_select, dim3(n), dim3(256), 0, stream, (const double*)drow, nr, k, list, f0, io, dout, dev_cap,
                           sq);
    }
    BMX_LAUNCH_CHECK();
}

void exact_search(hipStream_t stream, KnnWorkspace& ws, const double* X, const int32_t* ref_rows, int nr, const double* Qs,
                  const int32_t* qrs, int d, int k, int32_t* io, double* dout, const int32_t* list, const double* bounds,
                  int count, bool seeded) {
    if (count <= 0) return;
    ws.last_exact += count;
    const int32_t* scan_list = list;
    if (list && bounds) {
        scan_list = launch_bounded_sweep(stream, ws, X, ref_rows, nr, Qs, qrs, d, k, io, dout, list, bounds, count, 0, seeded,
                                         nullptr);
        count = read_count(stream, ws, scan_list);
    }
    if (count > 0) {
        const size_t budget = (size_t)512 << 20;
        // grid.y carries the queries of a batch: at most 65535 of them
        const int batch =
            (int)std::min<size_t>({std::max<size_t>(1, budget / ((size_t)nr * 8)), (size_t)count, (size_t)65535});
        double* drow = ws.drow.reserve((size_t)batch * nr);
        for (int f0 = 0; f0 < count; f0 += batch)
            launch_full_scan(stream, ws, X, ref_rows, nr, Qs, qrs, d, k, io, dout, scan_list, f0, std::min(batch, count - f0), 0,
                             drow);
    }
}

}  // namespace bmx
