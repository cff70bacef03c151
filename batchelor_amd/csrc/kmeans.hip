// kmeans() on the device: R's kmeans(x, centers = <matrix>, algorithm = "Lloyd") from a given K x d matrix of initial
// centres, behind the resident handle bmx_kmeans_t.  The observations (n x d, every observation's d values contiguous) are
// uploaded once and stay in HBM for every start and every iteration.  One iteration is
//   a. centre_norm_kernel: |c_j|^2, the squares added over the dimensions in ascending order.
//   b. assign_kernel: a workgroup owns TM = 64 observations (16 per wave) and sweeps the centres in tiles of TN = 64; the
//      products x . c of a tile run on the FP64 matrix cores (v_mfma_f64_16x16x4_f64, four 16 x 16 accumulators a wave),
//      the dimensions staged through LDS KC = 32 at a time (zeros beyond d, n and K), so d and K are unbounded by the
//      tile.  The distance is taken as |c|^2 - 2 x.c (|x|^2 is common to an observation's candidates); every lane keeps the
//      running (minimum, index) of its four observations in registers, a strict `<` over ascending centres, and the
//      sixteen lanes that share an observation then settle it with the lower index on equal values: R's scan.  The
//      n x K distances never leave the registers.  The lane that writes a label compares it with the one before and
//      raises one flag word: "did any label change" is four bytes per iteration.
//   c. the centre update, without floating-point atomics: the observations are bucketed by label with a stable counting
//      sort (rank_kernel: every observation's rank among the equal labels of its chunk and the chunk's label counts;
//      chunk_scan_kernel: the chunks' offsets per label and `size`; cluster_scan_kernel: the clusters' starts, their
//      pieces of PIECE = 256 members, the empty-cluster flag; scatter_kernel: the index list), so every cluster's
//      members stand in ascending order.  update_partial_kernel adds a piece's members (each wave a quarter, the
//      quarters then in order), update_reduce_kernel a cluster's pieces, and divides by the size: the orders are those
//      of ordered_sums.hpp.
// withinss is taken directly as sum (x - c)^2 over the same pieces (wss_partial_kernel / wss_reduce_kernel).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <numeric>
#include <vector>

#include "host_xfer.hpp"
#include "ordered_sums.hpp"
#include "resident_batches.hpp"

namespace bmx {
namespace {

typedef double d4 __attribute__((ext_vector_type(4)));
constexpr int TM = 64;      // observations a workgroup of the assignment owns (16 a wave)
constexpr int TN = 64;      // centres of a tile (four 16-wide MFMA sub-tiles)
constexpr int KC = 32;      // dimensions staged per step
constexpr int LP = KC + 2;  // LDS pitch in doubles: lanes (row 0..15, k 0..1) hit 32 different 8-byte bank pairs
constexpr int RB = 256;     // observations the ranking pass compares among themselves
constexpr int PIECE = 256;  // members of a cluster one workgroup of the update adds
constexpr int KMAX = 1024;  // centres at most
constexpr int MAX_CHUNKS = 4096;  // chunks of the ranking pass at most (their label counts are [chunks][K] words)

__global__ __launch_bounds__(256) void centre_norm_kernel(const double* __restrict__ c, int K, int d,
                                                          double* __restrict__ c2) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= K) return;
    const double* p = c + (int64_t)j * d;
    double s = 0.0;
    for (int k = 0; k < d; ++k) s += p[k] * p[k];
    c2[j] = s;
}

// labels[r] = the nearest centre of observation r (0-based; on equal distances the lowest index), flags[0] = 1 if that
// differs from labels[r] on entry.  A operand of the MFMA: lane l holds A[row = l & 15][k = l >> 4], B: B[k = l >> 4]
// [col = l & 15]; C/D: four doubles a lane, col = l & 15, row = (l >> 4) + 4 * reg.
__global__ __launch_bounds__(256) void assign_kernel(const double* __restrict__ x, int64_t n, int d,
                                                     const double* __restrict__ c, const double* __restrict__ c2, int K,
                                                     int32_t* __restrict__ labels, int32_t* __restrict__ flags) {
    __shared__ __attribute__((aligned(16))) double xs[TM * LP];
    __shared__ __attribute__((aligned(16))) double cs[TN * LP];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * TM;
    const int lr = tid >> 2, seg = (tid & 3) * 8;  // a step of either operand is 64 rows x 32 doubles: 8 a thread
    const int64_t xr = r0 + lr;
    double best[4];
    int bidx[4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        best[reg] = __longlong_as_double(0x7ff0000000000000ll);
        bidx[reg] = 0;
    }
    for (int j0 = 0; j0 < K; j0 += TN) {
        d4 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
        const int cj = j0 + lr;
        for (int k0 = 0; k0 < d; k0 += KC) {
            __syncthreads();  // (the step before has been multiplied)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = k0 + seg + e;
                xs[lr * LP + seg + e] = (xr < n && k < d) ? x[xr * d + k] : 0.0;
                cs[lr * LP + seg + e] = (cj < K && k < d) ? c[(int64_t)cj * d + k] : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < KC / 4; ++kk) {
                const double a = xs[(16 * w + (lane & 15)) * LP + 4 * kk + (lane >> 4)];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const double b = cs[(16 * t + (lane & 15)) * LP + 4 * kk + (lane >> 4)];
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {  // this lane's centres in ascending order
            const int j = j0 + 16 * t + (lane & 15);
            if (j < K) {
                const double cn = c2[j];
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const double dist = cn - 2.0 * acc[t][reg];
                    if (dist < best[reg]) {
                        best[reg] = dist;
                        bidx[reg] = j;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {  // the sixteen lanes of an observation: the smaller value, then the lower index
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            const double v = __shfl_xor(best[reg], o);
            const int i = __shfl_xor(bidx[reg], o);
            if (v < best[reg] || (v == best[reg] && i < bidx[reg])) {
                best[reg] = v;
                bidx[reg] = i;
            }
        }
    }
    if ((lane & 15) == 0) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t r = r0 + 16 * w + (lane >> 4) + 4 * reg;
            if (r < n && labels[r] != bidx[reg]) {
                labels[r] = bidx[reg];
                flags[0] = 1;
            }
        }
    }
}

// One workgroup per chunk of chunk_obs observations (a multiple of RB), walked RB at a time: rank[i] = how many
// observations before i in the chunk carry i's label, hist[chunk][j] = how many of the chunk carry label j.  Integer
// work only; the last observation of a label within a step is the one that moves the label's count on.
__global__ __launch_bounds__(RB) void rank_kernel(const int32_t* __restrict__ labels, int64_t n, int K, int64_t chunk_obs,
                                                  int32_t* __restrict__ rank, int32_t* __restrict__ hist) {
    __shared__ int32_t lab[RB];
    __shared__ int32_t cnt[KMAX];
    const int tid = threadIdx.x;
    for (int j = tid; j < K; j += RB) cnt[j] = 0;
    const int64_t b = (int64_t)blockIdx.x * chunk_obs;
    const int64_t e = min(n, b + chunk_obs);
    for (int64_t s = b; s < e; s += RB) {
        __syncthreads();  // (the counts stand, lab is free)
        const int64_t i = s + tid;
        const int my = i < e ? labels[i] : -1;
        lab[tid] = my;
        __syncthreads();
        int before = 0, base = 0;
        bool last = true;
        if (my >= 0) {
            for (int q = 0; q < RB; ++q) {
                if (lab[q] == my) {
                    if (q < tid) ++before;
                    if (q > tid) last = false;
                }
            }
            base = cnt[my];
            rank[i] = base + before;
        }
        __syncthreads();
        if (my >= 0 && last) cnt[my] = base + before + 1;
    }
    __syncthreads();
    for (int j = tid; j < K; j += RB) hist[(int64_t)blockIdx.x * K + j] = cnt[j];
}

// hist[chunk][j] becomes the number of label-j observations in the chunks before; size[j] their total
__global__ __launch_bounds__(256) void chunk_scan_kernel(int32_t* __restrict__ hist, int nchunks, int K,
                                                         int32_t* __restrict__ size) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= K) return;
    int32_t run = 0;
    for (int ch = 0; ch < nchunks; ++ch) {
        const int32_t v = hist[(int64_t)ch * K + j];
        hist[(int64_t)ch * K + j] = run;
        run += v;
    }
    size[j] = run;
}

// start[j] = where cluster j's members begin in the index list, piece0[j] = its first piece of PIECE members (K + 1
// entries each); flags[1] = 1 if a cluster is empty.  K <= 1024 words: one thread.
__global__ void cluster_scan_kernel(const int32_t* __restrict__ size, int K, int32_t* __restrict__ start,
                                    int32_t* __restrict__ piece0, int32_t* __restrict__ flags) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int32_t s = 0, p = 0;
    int empty = 0;
    for (int j = 0; j < K; ++j) {
        const int32_t m = size[j];
        start[j] = s;
        piece0[j] = p;
        s += m;
        p += (m + PIECE - 1) / PIECE;
        if (m == 0) empty = 1;
    }
    start[K] = s;
    piece0[K] = p;
    if (empty) flags[1] = 1;
}

__global__ __launch_bounds__(256) void scatter_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ rank,
                                                      const int32_t* __restrict__ hist, const int32_t* __restrict__ start,
                                                      int64_t n, int K, int64_t chunk_obs, int32_t* __restrict__ order) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int l = labels[i];
    const int64_t ch = i / chunk_obs;
    order[start[l] + hist[ch * K + l] + rank[i]] = (int32_t)i;
}

// the cluster piece p belongs to: piece0[j] <= p < piece0[j + 1] (clusters without members own no piece)
__device__ inline int piece_cluster(const int32_t* __restrict__ piece0, int K, int p) {
    int lo = 0, hi = K;  // the answer lies in [lo, hi)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (piece0[mid] <= p)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// part[p][g] = the sum over piece p's members, in list order within each quarter and the quarters in order, of x[., g]:
// grid (pieces at most, tiles of 64 dimensions), wave w takes the piece's members [64 w, 64 w + 64), lanes along g
__global__ __launch_bounds__(256) void update_partial_kernel(const double* __restrict__ x, int d,
                                                             const int32_t* __restrict__ order,
                                                             const int32_t* __restrict__ start,
                                                             const int32_t* __restrict__ piece0, int K,
                                                             double* __restrict__ part) {
    __shared__ double sh[4][64];
    const int p = blockIdx.x;
    if (p >= piece0[K]) return;
    const int j = piece_cluster(piece0, K, p);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int g = blockIdx.y * 64 + lane;
    const int pb = start[j] + (p - piece0[j]) * PIECE;
    const int pe = min(start[j + 1], pb + PIECE);
    const int b = min(pe, pb + 64 * w), e = min(pe, pb + 64 * w + 64);
    double s = 0.0;
    if (g < d)
        ordered_walk4(
            b, e, [&](int i) { return x[(int64_t)order[i] * d + g]; }, [&](double v) { s += v; });
    sh[w][lane] = s;
    __syncthreads();
    if (w == 0 && g < d) part[(int64_t)p * d + g] = ((sh[0][lane] + sh[1][lane]) + sh[2][lane]) + sh[3][lane];
}

// centres[j][g] = (cluster j's pieces, ascending) / size[j]; an empty cluster keeps its centre (the run ends in an error)
__global__ __launch_bounds__(256) void update_reduce_kernel(const double* __restrict__ part, int d, int K,
                                                            const int32_t* __restrict__ piece0,
                                                            const int32_t* __restrict__ size,
                                                            double* __restrict__ centres) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int j = blockIdx.y;
    if (g >= d || j >= K) return;
    const int f = piece0[j], l = piece0[j + 1];
    if (f == l) return;
    const auto at = [&](int p) { return part[(int64_t)p * d + g]; };
    centres[(int64_t)j * d + g] = fold_ascending(at(f), f + 1, l, at) / (double)size[j];
}

// wpart[p] = sum over piece p's members and all dimensions of (x - c)^2: every lane its dimensions g = lane, lane + 64, ...
// of its wave's members in order, then the lanes by a fixed tree and the waves in order
__global__ __launch_bounds__(256) void wss_partial_kernel(const double* __restrict__ x, int d,
                                                          const int32_t* __restrict__ order,
                                                          const int32_t* __restrict__ start,
                                                          const int32_t* __restrict__ piece0, int K,
                                                          const double* __restrict__ centres, double* __restrict__ wpart) {
    __shared__ double sh[4];
    const int p = blockIdx.x;
    if (p >= piece0[K]) return;
    const int j = piece_cluster(piece0, K, p);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int pb = start[j] + (p - piece0[j]) * PIECE;
    const int pe = min(start[j + 1], pb + PIECE);
    const int b = min(pe, pb + 64 * w), e = min(pe, pb + 64 * w + 64);
    const double* cj = centres + (int64_t)j * d;
    double s = 0.0;
    for (int i = b; i < e; ++i) {
        const double* row = x + (int64_t)order[i] * d;
        for (int g = lane; g < d; g += 64) {
            const double df = row[g] - cj[g];
            s += df * df;
        }
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) sh[w] = s;
    __syncthreads();
    if (threadIdx.x == 0) wpart[p] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ __launch_bounds__(256) void wss_reduce_kernel(const double* __restrict__ wpart, int K,
                                                         const int32_t* __restrict__ piece0, double* __restrict__ withinss) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= K) return;
    withinss[j] = fold_ascending(0.0, piece0[j], piece0[j + 1], [&](int p) { return wpart[p]; });
}

}  // namespace

// argument checks of Kmeans::run, without a device (throws Error(BMX_ERR_ARG)): centers [K][d], every centre contiguous
static void kmeans_check_run(int64_t n, int d, const double* centers, int K, int iter_max) {
    if (K < 1 || K > KMAX || K > n) throw Error(BMX_ERR_ARG, "kmeans takes 1 <= K <= min(n, 1024) centers");
    if (iter_max < 1) throw Error(BMX_ERR_ARG, "'iter_max' must be positive");
    if (!centers) throw Error(BMX_ERR_ARG, "'centers' is missing");
    for (size_t i = 0; i < (size_t)K * d; ++i)
        if (!std::isfinite(centers[i])) throw Error(BMX_ERR_ARG, "'centers' must be finite");
    // any(duplicated(centers)): the rows sorted lexicographically, then neighbours compared
    std::vector<int> idx((size_t)K);
    std::iota(idx.begin(), idx.end(), 0);
    auto row = [&](int j) { return centers + (size_t)j * d; };
    std::sort(idx.begin(), idx.end(),
              [&](int a, int b) { return std::lexicographical_compare(row(a), row(a) + d, row(b), row(b) + d); });
    for (int i = 1; i < K; ++i)
        if (std::equal(row(idx[i - 1]), row(idx[i - 1]) + d, row(idx[i])))
            throw Error(BMX_ERR_ARG, "initial centers are not distinct");
}

// The observations stay resident for every start (run) and every iteration.
class Kmeans : ResidentBatches<ResidentBatch> {
  public:
    Kmeans(int device, int d) : ResidentBatches(device, d, "bmx_kmeans_begin") {}
    ~Kmeans() { retire(); }

    // n observations follow in one or more blocks, in order; a handle holds one set of observations
    void begin_data(int64_t n) {
        if (!batches_.empty()) throw Error(BMX_ERR_ARG, "the handle already holds its observations");
        if (n < 1) throw Error(BMX_ERR_ARG, "kmeans needs at least one observation");
        if (n > 0x7fffffffll) throw Error(BMX_ERR_ARG, "kmeans takes at most 2^31 - 1 observations");
        begin(n, [](ResidentBatch&) {});
    }

    void add_block(const double* x_block, int64_t m) {
        const double t0 = now_ms();
        add(x_block, m, [&](ResidentBatch& b, double*) {
            if (b.complete()) BMX_HIP(hipStreamSynchronize(stream_));
        });
        ms_[0] += now_ms() - t0;
    }

    // Lloyd from centers [K][d]: labels_out [n] 1-based, centers_out [K][d], size_out [K], withinss_out [K]
    void run(const double* centers, int K, int iter_max, int32_t* labels_out, double* centers_out, int32_t* size_out,
             double* withinss_out, double* tot_withinss, int32_t* iter_out, int32_t* converged_out) {
        if (batches_.empty() || !batches_[0]->complete())
            throw Error(BMX_ERR_ARG, "the observations have not all been received");
        const ResidentBatch& xb = *batches_[0];
        const int64_t n = xb.n;
        const int d = G_;
        kmeans_check_run(n, d, centers, K, iter_max);
        if (!labels_out || !centers_out || !size_out || !withinss_out || !tot_withinss || !iter_out || !converged_out)
            throw Error(BMX_ERR_ARG, "every output of kmeans must be given");
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        const int64_t chunk_obs = std::max<int64_t>(RB, round_up((n + MAX_CHUNKS - 1) / MAX_CHUNKS, RB));
        const int nchunks = cdiv(n, chunk_obs);
        const int max_pieces = cdiv(n, PIECE) + K;
        double* cen = cen_.reserve((size_t)K * d);
        double* c2 = c2_.reserve((size_t)K);
        double* part = part_.reserve((size_t)max_pieces * d);
        double* wpart = wpart_.reserve((size_t)max_pieces);
        double* wss = wss_.reserve((size_t)K);
        int32_t* labels = labels_.reserve((size_t)n);
        int32_t* rank = rank_.reserve((size_t)n);
        int32_t* order = order_.reserve((size_t)n);
        int32_t* hist = hist_.reserve((size_t)nchunks * K);
        int32_t* small = small_.reserve(3 * (size_t)K + 4);
        int32_t* size = small;              // [K]
        int32_t* start = size + K;          // [K + 1]
        int32_t* piece0 = start + K + 1;    // [K + 1]
        int32_t* flags = piece0 + K + 1;    // [2]: a label changed, a cluster is empty

        BMX_HIP(hipMemcpyAsync(cen, centers, (size_t)K * d * sizeof(double), hipMemcpyHostToDevice, stream_));
        BMX_HIP(hipMemsetAsync(labels, 0xff, (size_t)n * sizeof(int32_t), stream_));  // "none"
        const unsigned kblocks = (unsigned)cdiv(K, 256);
        int iter = 0, converged = 0;
        while (iter < iter_max) {
            ++iter;
            int32_t host_flags[2] = {0, 0};
            BMX_HIP(hipMemsetAsync(flags, 0, 2 * sizeof(int32_t), stream_));
            const int e0 = timer_.mark(stream_);
            hipLaunchKernelGGL(centre_norm_kernel, dim3(kblocks), dim3(256), 0, stream_, (const double*)cen, K, d, c2);
            BMX_LAUNCH_CHECK();
            hipLaunchKernelGGL(assign_kernel, dim3((unsigned)cdiv(n, TM)), dim3(256), 0, stream_, (const double*)xb.x.p, n, d,
                               (const double*)cen, (const double*)c2, K, labels, flags);
            BMX_LAUNCH_CHECK();
            const int e1 = timer_.mark(stream_);
            BMX_HIP(hipMemcpyAsync(host_flags, flags, sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
            BMX_HIP(hipStreamSynchronize(stream_));
            timer_.span(1, e0, e1);
            timer_.collect(ms_);
            if (!host_flags[0]) {
                converged = 1;
                break;
            }
            const int e2 = timer_.mark(stream_);
            bucket(labels, n, K, chunk_obs, nchunks, rank, hist, size, start, piece0, flags, order);
            hipLaunchKernelGGL(update_partial_kernel, dim3((unsigned)max_pieces, (unsigned)cdiv(d, 64)), dim3(256), 0, stream_,
                               (const double*)xb.x.p, d, (const int32_t*)order, (const int32_t*)start,
                               (const int32_t*)piece0, K, part);
            BMX_LAUNCH_CHECK();
            hipLaunchKernelGGL(update_reduce_kernel, dim3((unsigned)cdiv(d, 256), (unsigned)K), dim3(256), 0, stream_,
                               (const double*)part, d, K, (const int32_t*)piece0, (const int32_t*)size, cen);
            BMX_LAUNCH_CHECK();
            const int e3 = timer_.mark(stream_);
            BMX_HIP(hipMemcpyAsync(host_flags + 1, flags + 1, sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
            BMX_HIP(hipStreamSynchronize(stream_));
            timer_.span(2, e2, e3);
            timer_.collect(ms_);
            if (host_flags[1]) throw Error(BMX_ERR_ARG, "empty cluster: try a better set of initial centers");
        }
        // (the index list and the pieces are those of the returned labels: the last update's, which a converged
        // assignment left as they were)
        const int e4 = timer_.mark(stream_);
        hipLaunchKernelGGL(wss_partial_kernel, dim3((unsigned)max_pieces), dim3(256), 0, stream_, (const double*)xb.x.p, d,
                           (const int32_t*)order, (const int32_t*)start, (const int32_t*)piece0, K, (const double*)cen, wpart);
        BMX_LAUNCH_CHECK();
        hipLaunchKernelGGL(wss_reduce_kernel, dim3(kblocks), dim3(256), 0, stream_, (const double*)wpart, K,
                           (const int32_t*)piece0, wss);
        BMX_LAUNCH_CHECK();
        const int e5 = timer_.mark(stream_);
        const double t0 = now_ms();
        BMX_HIP(hipMemcpyAsync(centers_out, cen, (size_t)K * d * sizeof(double), hipMemcpyDeviceToHost, stream_));
        BMX_HIP(hipMemcpyAsync(size_out, size, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
        BMX_HIP(hipMemcpyAsync(withinss_out, wss, (size_t)K * sizeof(double), hipMemcpyDeviceToHost, stream_));
        download_pageable(labels_out, labels, (size_t)n * sizeof(int32_t), stream_);
        BMX_HIP(hipStreamSynchronize(stream_));
        ms_[4] += now_ms() - t0;
        timer_.span(3, e4, e5);
        timer_.collect(ms_);
        for (int64_t i = 0; i < n; ++i) labels_out[i] += 1;
        double tot = 0.0;
        for (int j = 0; j < K; ++j) tot += withinss_out[j];
        *tot_withinss = tot;
        *iter_out = iter;
        *converged_out = converged;
    }

    // milliseconds since the handle was made: upload (host wall time of the staged copies), then HIP-event time of the
    // assignments, the centre updates, withinss, and the host wall time of the downloads
    using ResidentBatches::stage_ms;

  private:
    // the observations' indices sorted by label, ascending within a label: `order`, with `size`, `start` and `piece0`
    void bucket(const int32_t* labels, int64_t n, int K, int64_t chunk_obs, int nchunks, int32_t* rank, int32_t* hist,
                int32_t* size, int32_t* start, int32_t* piece0, int32_t* flags, int32_t* order) {
        hipLaunchKernelGGL(rank_kernel, dim3((unsigned)nchunks), dim3(RB), 0, stream_, labels, n, K, chunk_obs, rank, hist);
        BMX_LAUNCH_CHECK();
        hipLaunchKernelGGL(chunk_scan_kernel, dim3((unsigned)cdiv(K, 256)), dim3(256), 0, stream_, hist, nchunks, K, size);
        BMX_LAUNCH_CHECK();
        hipLaunchKernelGGL(cluster_scan_kernel, dim3(1), dim3(64), 0, stream_, (const int32_t*)size, K, start, piece0, flags);
        BMX_LAUNCH_CHECK();
        hipLaunchKernelGGL(scatter_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, stream_, labels, (const int32_t*)rank,
                           (const int32_t*)hist, (const int32_t*)start, n, K, chunk_obs, order);
        BMX_LAUNCH_CHECK();
    }

    DevBuf<double> cen_, c2_, part_, wpart_, wss_;
    DevBuf<int32_t> labels_, rank_, order_, hist_, small_;
};

}  // namespace bmx

/* ---------------------------------------------------------------- bmx_kmeans_* ---------------------------------- */
struct bmx_kmeans final : bmx::Kmeans {
    using Kmeans::Kmeans;
};

extern "C" {

int32_t bmx_kmeans_create(int32_t device, int32_t d, bmx_kmeans_t** out) {
    return bmx::guarded([&] {
        if (!out) throw bmx::Error(BMX_ERR_ARG, "null output pointer");
        if (d < 1) throw bmx::Error(BMX_ERR_ARG, "kmeans needs at least one dimension");
        *out = new bmx_kmeans(device, d);
    });
}

void bmx_kmeans_destroy(bmx_kmeans_t* h) { delete h; }

int32_t bmx_kmeans_begin(bmx_kmeans_t* h, int64_t n) {
    return bmx::guarded([&] { bmx::live(h).begin_data(n); });
}

int32_t bmx_kmeans_add_block(bmx_kmeans_t* h, const double* x_block, int64_t n_block) {
    return bmx::guarded([&] { bmx::live(h).add_block(x_block, n_block); });
}

int32_t bmx_kmeans_run(bmx_kmeans_t* h, const double* centers, int32_t n_centers, int32_t iter_max, int32_t* cluster_out,
                       double* centers_out, int32_t* size_out, double* withinss_out, double* tot_withinss_out,
                       int32_t* iter_out, int32_t* converged_out) {
    return bmx::guarded([&] {
        bmx::live(h).run(centers, n_centers, iter_max, cluster_out, centers_out, size_out, withinss_out, tot_withinss_out,
                         iter_out, converged_out);
    });
}

int32_t bmx_kmeans_stage_ms(const bmx_kmeans_t* h, double* out5) {
    return bmx::guarded([&] {
        if (!h || !out5) throw bmx::Error(BMX_ERR_ARG, "null argument");
        h->stage_ms(out5);
    });
}

}  // extern "C"
