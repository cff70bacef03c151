// makeSNNGraph on the device: the shared-nearest-neighbour graph of a k-nearest-neighbour index ("The SNN graph").
// idx [n][k]: each row's k nearest OTHER rows, 0-based, distinct, never the row itself.  L(c) = (c, idx[c][0..k)) with ranks
// 0..k; cells a > b share an edge when L(a) and L(b) meet; per edge the smallest rank sum over the shared cells and their
// number.  Integer work throughout; the only floating-point operations are the three weight formulas, one per edge.
//   1. check_count_kernel: the three input faults into a flag word, the in-degree of every cell (integer adds).
//   2. the reverse ("host") lists by a counting sort: exclusive_scan_i32 of the in-degrees, fill_kernel drops every
//      (host, rank) into its cell's range through a cursor, order_kernel puts each range in ascending host order (every entry
//      counts the smaller ones: hosts are distinct within a range), so the lists hold the same bytes in every run.
//   3. cell_kernel, once to count and once to write: a wave a cell j.  The partners h < j of j are the hosts below j of the
//      reverse lists of the k + 1 members of L(j), and the members below j themselves.  A window [h0, h1) of hosts whose
//      candidates fit the LDS budget is gathered as keys (host << 9 | rank sum), sorted in the LDS, and every run of one host
//      is an edge: its first key carries the smallest rank sum, its length is the count.  Windows ascend, so edges leave in
//      ascending h.  A cell whose candidates fit at once has one window; the others ("spilled") look for each window's end
//      by bisection over the hosts.  Between the two runs the 64-bit offsets of the cells' edges are scanned.
#include <algorithm>

#include "bmx_ops.hpp"

namespace bmx {

namespace {

constexpr int SNN_LISTS = SNN_MAX_K + 1;  // members of L(j) at most
constexpr int SNN_PER_LANE = (SNN_LISTS + 63) / 64;
constexpr int SUM_BITS = 9;            // rank sums are at most 2 k = 256
constexpr int SNN_DEFAULT_BUDGET = 2048;
constexpr int SNN_MAX_BUDGET = 4096;
constexpr int ORDER_CHUNK = 512;       // entries of a reverse list order_kernel compares against at a time
constexpr int SCAN_ITEMS = 4;          // counts a thread of the 64-bit scan owns

enum : int { FLAG_RANGE = 1, FLAG_SELF = 2, FLAG_REPEAT = 4 };

struct Stats {
    int64_t spilled = 0;
    int64_t graph_us = 0;
};
Stats& stats() {
    static thread_local Stats s;
    return s;
}

// [n x k] column-major 1-based (R) -> [n][k] row-major 0-based; nothing is judged here (0 becomes -1, check_count_kernel's business)
__global__ __launch_bounds__(256) void from_r_layout_kernel(const int32_t* __restrict__ cm, int n, int k, int32_t* __restrict__ rm) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)n * k) return;
    const int r = (int)(t / n), i = (int)(t % n);
    rm[(int64_t)i * k + r] = (int32_t)((uint32_t)cm[t] - 1u);
}

// A wave a row: entries outside [0, n), the row itself, repeats; deg[c] += 1 for every entry c in range.
__global__ __launch_bounds__(256) void check_count_kernel(const int32_t* __restrict__ idx, int n, int k, int32_t* __restrict__ deg,
                                                          int32_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;  // (whole waves leave: no barrier below)
    const int32_t* p = idx + (int64_t)row * k;
    int32_t v[2];
    int f = 0;
    for (int u = 0; u < 2; ++u) {
        const int r = lane + 64 * u;
        v[u] = r < k ? p[r] : -1;
        if (r < k) {
            if (v[u] < 0 || v[u] >= n) f |= FLAG_RANGE;
            else {
                if (v[u] == row) f |= FLAG_SELF;
                atomicAdd(&deg[v[u]], 1);
            }
        }
    }
    for (int i = 0; i < k; ++i) {
        const int32_t w = p[i];
        for (int u = 0; u < 2; ++u) {
            const int r = lane + 64 * u;
            if (r < k && r != i && v[u] == w) f |= FLAG_REPEAT;
        }
    }
    if (f) atomicOr(flags, f);
}

// entry (h, r) of idx goes to the range of the cell it names: (h << 8 | r + 1), ranks 1..k
__global__ __launch_bounds__(256) void fill_kernel(const int32_t* __restrict__ idx, int64_t entries, int k, const int32_t* __restrict__ roff,
                                                   int32_t* __restrict__ cursor, unsigned long long* __restrict__ unordered) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= entries) return;
    const int c = idx[t];
    const int h = (int)(t / k), r = (int)(t % k) + 1;
    const int slot = roff[c] + atomicAdd(&cursor[c], 1);
    unordered[slot] = ((unsigned long long)h << 8) | (unsigned)r;
}

// A wave (workgroup) a cell: its range of `unordered` into `rev` in ascending host order.  Hosts are distinct within a range,
// so an entry's place is the number of smaller entries.
__global__ __launch_bounds__(64) void order_kernel(const int32_t* __restrict__ roff, const unsigned long long* __restrict__ unordered,
                                                   unsigned long long* __restrict__ rev) {
    __shared__ unsigned long long chunk[ORDER_CHUNK];
    const int lane = threadIdx.x;
    const int c = blockIdx.x;
    const int base = roff[c], len = roff[c + 1] - base;
    if (len <= 0) return;
    if (len == 1) {
        if (lane == 0) rev[base] = unordered[base];
        return;
    }
    for (int e0 = 0; e0 < len; e0 += 64) {
        const int e = e0 + lane;
        const unsigned long long mine = e < len ? unordered[base + e] : 0ull;
        int pos = 0;
        for (int f0 = 0; f0 < len; f0 += ORDER_CHUNK) {
            const int m = min(ORDER_CHUNK, len - f0);
            if (f0 > 0 || e0 == 0 || len > ORDER_CHUNK) {  // (a list of one chunk is staged once)
                __syncthreads();
                for (int f = lane; f < m; f += 64) chunk[f] = unordered[base + f0 + f];
                __syncthreads();
            }
            for (int f = 0; f < m; ++f) pos += chunk[f] < mine ? 1 : 0;
        }
        if (e < len) rev[base + pos] = mine;
    }
}

// first position of the ascending list p[0, len) whose host is not below h
__device__ inline int lower_bound_host(const unsigned long long* __restrict__ p, int len, int64_t h) {
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)(p[mid] >> 8) < h) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ inline int wave_sum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ inline int wave_inclusive_scan(int v, int lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// The members of L(j) a lane looks after (lists lane, lane + 64, lane + 128) and where they stand in a window of hosts.
struct LaneLists {
    int member[SNN_PER_LANE];  // the cell s (-1: no such list)
    int base[SNN_PER_LANE], len[SNN_PER_LANE];  // its reverse list rev[base, base + len)
    int lo[SNN_PER_LANE];      // first entry at or beyond the window's start
};

// candidates with hosts in [h0, h1): entries of the reverse lists (from lo on) and the members themselves (rank 0 in their own list)
__device__ inline int window_count(const LaneLists& L, const unsigned long long* __restrict__ rev, int nl, int lane, int64_t h0, int64_t h1) {
    int c = 0;
    for (int u = 0; u < SNN_PER_LANE; ++u) {
        const int t = lane + 64 * u;
        if (t >= nl) continue;
        c += lower_bound_host(rev + L.base[u] + L.lo[u], L.len[u] - L.lo[u], h1);
        if (t > 0 && L.member[u] >= h0 && L.member[u] < h1) ++c;
    }
    return wave_sum(c);
}

// LDS of a cell_kernel workgroup: cap keys, then the lists' tables
template <class Key>
size_t cell_lds_bytes(int cap) {
    return (size_t)cap * sizeof(Key) + (size_t)(4 * (SNN_LISTS + 3)) * sizeof(int);
}

// One wave (one workgroup) a cell.  FILL = false: ecount[j] = its edges, *spilled += cells of more than one window.
// FILL = true: the edges into first / second / weight from eoff[j] on.  cap = the power of two at or above budget.
template <class Key, bool FILL>
__global__ __launch_bounds__(64) void cell_kernel(const int32_t* __restrict__ idx, int n, int k, const int32_t* __restrict__ roff,
                                                  const unsigned long long* __restrict__ rev, int budget, int cap, int type,
                                                  int32_t* __restrict__ ecount, unsigned int* __restrict__ spilled,
                                                  const int64_t* __restrict__ eoff, int32_t* __restrict__ first,
                                                  int32_t* __restrict__ second, double* __restrict__ weight) {
    extern __shared__ __align__(16) unsigned char smem[];
    Key* keys = reinterpret_cast<Key*>(smem);
    int* lpre = reinterpret_cast<int*>(keys + cap);  // [nl + 1] candidates before list t in the window
    int* lbeg = lpre + SNN_LISTS + 3;                // [nl] the list's first entry of the window (position in rev)
    int* lrev = lbeg + SNN_LISTS + 3;                // [nl] how many of the list's candidates are reverse-list entries
    int* lmem = lrev + SNN_LISTS + 3;                // [nl] the member
    const int lane = threadIdx.x;
    const int j = blockIdx.x;
    const int nl = k + 1;
    if (j == 0) {  // no partner below the first cell
        if (!FILL && lane == 0) ecount[0] = 0;
        return;
    }
    LaneLists L;
    for (int u = 0; u < SNN_PER_LANE; ++u) {
        const int t = lane + 64 * u;
        L.member[u] = -1;
        L.base[u] = L.len[u] = L.lo[u] = 0;
        if (t < nl) {
            const int s = t == 0 ? j : idx[(int64_t)j * k + (t - 1)];
            L.member[u] = s;
            L.base[u] = roff[s];
            L.len[u] = roff[s + 1] - L.base[u];
            lmem[t] = s;
        }
    }
    const int total = window_count(L, rev, nl, lane, 0, j);
    if (!FILL && total > budget && lane == 0) atomicAdd(spilled, 1u);
    int64_t epos = FILL ? eoff[j] : 0;
    int nedges = 0;
    int64_t h0 = 0;
    int remaining = total;
    while (h0 < j) {
        // the window's end: all that is left if it fits, else the farthest host whose window still does (one host brings
        // at most k + 1 <= budget candidates)
        int64_t h1 = j;
        if (remaining > budget) {
            int64_t lo = h0 + 1, hi = j;  // window_count(lo) <= budget < window_count(hi)
            while (hi - lo > 1) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                if (window_count(L, rev, nl, lane, h0, mid) <= budget) lo = mid;
                else hi = mid;
            }
            h1 = lo;
        }
        // per list: its entries of the window, whether the member itself is in it; prefix over the lists
        int carry = 0;
        for (int u = 0; u < SNN_PER_LANE; ++u) {
            const int t = lane + 64 * u;
            int c = 0, nrev = 0;
            if (t < nl) {
                nrev = lower_bound_host(rev + L.base[u] + L.lo[u], L.len[u] - L.lo[u], h1);
                c = nrev + ((t > 0 && L.member[u] >= h0 && L.member[u] < h1) ? 1 : 0);
            }
            const int incl = wave_inclusive_scan(c, lane);
            if (t < nl) {
                lpre[t] = carry + incl - c;
                lbeg[t] = L.base[u] + L.lo[u];
                lrev[t] = nrev;
                L.lo[u] += nrev;
            }
            carry += __shfl(incl, 63, 64);
        }
        const int C = carry;  // <= budget <= cap
        if (lane == 0) lpre[nl] = C;
        remaining -= C;
        __syncthreads();
        if (C > 0) {
            int N = 1;
            while (N < C) N <<= 1;
            for (int p = lane; p < N; p += 64) {
                Key key = ~(Key)0;
                if (p < C) {
                    int a = 0, b = nl;  // the last list t with lpre[t] <= p (empty lists share their successor's start)
                    while (b - a > 1) {
                        const int mid = (a + b) >> 1;
                        if (lpre[mid] <= p) a = mid;
                        else b = mid;
                    }
                    const int q = p - lpre[a];
                    if (q < lrev[a]) {
                        const unsigned long long e = rev[lbeg[a] + q];
                        key = ((Key)(e >> 8) << SUM_BITS) | (Key)(a + (int)(e & 255u));
                    } else {
                        key = ((Key)lmem[a] << SUM_BITS) | (Key)a;
                    }
                }
                keys[p] = key;
            }
            __syncthreads();
            for (int size = 2; size <= N; size <<= 1) {
                for (int stride = size >> 1; stride > 0; stride >>= 1) {
                    for (int p = lane; p < (N >> 1); p += 64) {
                        const int i = ((p & ~(stride - 1)) << 1) | (p & (stride - 1));
                        const Key x = keys[i], y = keys[i + stride];
                        if ((x > y) == ((i & size) == 0)) {
                            keys[i] = y;
                            keys[i + stride] = x;
                        }
                    }
                    __syncthreads();
                }
            }
            // every run of one host is an edge
            for (int i0 = 0; i0 < C; i0 += 64) {
                const int i = i0 + lane;
                const Key key = i < C ? keys[i] : (Key)0;
                const Key h = key >> SUM_BITS;
                const bool head = i < C && (i == 0 || (keys[i - 1] >> SUM_BITS) != h);
                const unsigned long long m = __builtin_amdgcn_ballot_w64(head);
                if (FILL && head) {
                    int cnt = 1;
                    while (i + cnt < C && (keys[i + cnt] >> SUM_BITS) == h) ++cnt;
                    const int rsum = (int)(key & (Key)((1 << SUM_BITS) - 1));
                    double w;
                    if (type == 0) w = fmax((double)k - 0.5 * (double)rsum, 1e-6);
                    else if (type == 1) w = fmax((double)cnt, 1e-6);
                    else w = (double)cnt / (double)(2 * (k + 1) - cnt);
                    const int64_t o = epos + nedges + __builtin_popcountll(m & ((1ull << lane) - 1ull));
                    first[o] = j + 1;
                    second[o] = (int32_t)h + 1;
                    weight[o] = w;
                }
                nedges += __builtin_popcountll(m);
            }
        }
        __syncthreads();  // (the tables and the keys are written again in the next window)
        h0 = h1;
    }
    if (!FILL && lane == 0) ecount[j] = nedges;
}

// ---- 64-bit exclusive scan of the cells' edge counts: out [n + 1], out[n] = the number of edges ----
__global__ __launch_bounds__(256) void scan64_sums_kernel(const int32_t* __restrict__ in, int n, int64_t* __restrict__ bsum) {
    __shared__ int64_t red[256];
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * SCAN_ITEMS;
    int64_t s = 0;
    for (int u = 0; u < SCAN_ITEMS; ++u)
        if (i0 + u < n) s += in[i0 + u];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) bsum[blockIdx.x] = red[0];
}
// exclusive scan over 256 values in the LDS (Hillis-Steele); returns the thread's exclusive prefix, *total the sum
__device__ inline int64_t block_exclusive_scan(int64_t v, int64_t* buf, int64_t* total) {
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int64_t add = t >= o ? buf[t - o] : 0;
        __syncthreads();
        buf[t] += add;
        __syncthreads();
    }
    const int64_t incl = buf[t];
    *total = buf[255];
    __syncthreads();
    return incl - v;
}
__global__ __launch_bounds__(256) void scan64_blocks_kernel(int64_t* __restrict__ bsum, int nb) {  // one workgroup, in place
    __shared__ int64_t buf[256];
    int64_t carry = 0;
    for (int b0 = 0; b0 < nb; b0 += 256) {
        const int b = b0 + threadIdx.x;
        const int64_t v = b < nb ? bsum[b] : 0;
        int64_t total;
        const int64_t ex = block_exclusive_scan(v, buf, &total);
        if (b < nb) bsum[b] = carry + ex;
        carry += total;
    }
}
__global__ __launch_bounds__(256) void scan64_write_kernel(const int32_t* __restrict__ in, int n, const int64_t* __restrict__ bsum,
                                                           int64_t* __restrict__ out) {
    __shared__ int64_t buf[256];
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * SCAN_ITEMS;
    int32_t v[SCAN_ITEMS];
    int64_t s = 0;
    for (int u = 0; u < SCAN_ITEMS; ++u) {
        v[u] = i0 + u < n ? in[i0 + u] : 0;
        s += v[u];
    }
    int64_t total;
    int64_t run = bsum[blockIdx.x] + block_exclusive_scan(s, buf, &total);
    for (int u = 0; u < SCAN_ITEMS; ++u) {
        if (i0 + u < n) out[i0 + u] = run;
        run += v[u];
        if (i0 + u == n - 1) out[n] = run;
    }
}

template <class Key>
void launch_cells(hipStream_t stream, bool fill, const int32_t* idx, int n, int k, const int32_t* roff, const unsigned long long* rev,
                  int budget, int cap, int type, int32_t* ecount, unsigned int* spilled, const int64_t* eoff, int32_t* first,
                  int32_t* second, double* weight) {
    const size_t lds = cell_lds_bytes<Key>(cap);
    if (fill)
        hipLaunchKernelGGL((cell_kernel<Key, true>), dim3((unsigned)n), dim3(64), lds, stream, idx, n, k, roff, rev, budget, cap, type,
                           ecount, spilled, eoff, first, second, weight);
    else
        hipLaunchKernelGGL((cell_kernel<Key, false>), dim3((unsigned)n), dim3(64), lds, stream, idx, n, k, roff, rev, budget, cap, type,
                           ecount, spilled, eoff, first, second, weight);
    BMX_LAUNCH_CHECK();
}

struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    EventPair() {
        BMX_HIP(hipEventCreate(&a));
        BMX_HIP(hipEventCreate(&b));
    }
    ~EventPair() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};

}  // namespace

void snn_index_from_r_layout(hipStream_t stream, const int32_t* cm, int n, int k, int32_t* rm) {
    const int64_t entries = (int64_t)n * k;
    if (entries <= 0) return;
    hipLaunchKernelGGL(from_r_layout_kernel, dim3((unsigned)cdiv(entries, 256)), dim3(256), 0, stream, cm, n, k, rm);
    BMX_LAUNCH_CHECK();
}

void snn_stats_read(int64_t out[2]) {
    out[0] = stats().spilled;
    out[1] = stats().graph_us;
}

int64_t snn_graph_device(hipStream_t stream, ScanWorkspace& ws, const int32_t* idx, int n, int k, int type, DevBuf<int32_t>& first,
                         DevBuf<int32_t>& second, DevBuf<double>& weight) {
    stats() = Stats();
    if (n <= 1) return 0;
    const int64_t entries = (int64_t)n * k;
    const int knob = dev_knobs().snn_lds_candidates;
    const int budget = std::min(SNN_MAX_BUDGET, std::max(k + 1, knob > 0 ? knob : SNN_DEFAULT_BUDGET));
    int cap = 64;
    while (cap < budget) cap <<= 1;

    EventPair ev;
    BMX_HIP(hipEventRecord(ev.a, stream));
    // words: [0] the input faults, [1] cells of more than one window; then the in-degrees (afterwards the fill's cursors)
    DevBuf<int32_t> words, deg, roff, ecount;
    DevBuf<unsigned long long> unordered, rev;
    DevBuf<int64_t> eoff, bsum;
    words.reserve(2);
    deg.reserve(n);
    roff.reserve((size_t)n + 1);
    BMX_HIP(hipMemsetAsync(words.p, 0, 2 * sizeof(int32_t), stream));
    BMX_HIP(hipMemsetAsync(deg.p, 0, (size_t)n * sizeof(int32_t), stream));
    hipLaunchKernelGGL(check_count_kernel, dim3((unsigned)cdiv(n, 4)), dim3(256), 0, stream, idx, n, k, deg.p, words.p);
    BMX_LAUNCH_CHECK();
    int32_t flags = 0;
    BMX_HIP(hipMemcpyAsync(&flags, words.p, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    BMX_HIP(hipStreamSynchronize(stream));
    if (flags & FLAG_RANGE) throw Error(BMX_ERR_ARG, "makeSNNGraph: 'index' has an entry outside 1..n");
    if (flags & FLAG_SELF) throw Error(BMX_ERR_ARG, "makeSNNGraph: a row of 'index' lists itself");
    if (flags & FLAG_REPEAT) throw Error(BMX_ERR_ARG, "makeSNNGraph: a row of 'index' lists a row twice");

    exclusive_scan_i32(stream, ws, deg.p, roff.p, n);
    BMX_HIP(hipMemsetAsync(deg.p, 0, (size_t)n * sizeof(int32_t), stream));
    unordered.reserve((size_t)entries);
    rev.reserve((size_t)entries);
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)cdiv(entries, 256)), dim3(256), 0, stream, idx, entries, k, roff.p, deg.p, unordered.p);
    BMX_LAUNCH_CHECK();
    hipLaunchKernelGGL(order_kernel, dim3((unsigned)n), dim3(64), 0, stream, roff.p, unordered.p, rev.p);
    BMX_LAUNCH_CHECK();

    // hosts below 2^23 leave 9 bits of a 32-bit key for the rank sum (and all ones for the padding)
    const bool narrow = n <= (1 << 23);
    ecount.reserve(n);
    unsigned int* spilled = reinterpret_cast<unsigned int*>(words.p + 1);
    if (narrow) launch_cells<uint32_t>(stream, false, idx, n, k, roff.p, rev.p, budget, cap, type, ecount.p, spilled, nullptr, nullptr, nullptr, nullptr);
    else launch_cells<unsigned long long>(stream, false, idx, n, k, roff.p, rev.p, budget, cap, type, ecount.p, spilled, nullptr, nullptr, nullptr, nullptr);
    const int nb = cdiv(n, 256 * SCAN_ITEMS);
    eoff.reserve((size_t)n + 1);
    bsum.reserve(nb);
    hipLaunchKernelGGL(scan64_sums_kernel, dim3(nb), dim3(256), 0, stream, ecount.p, n, bsum.p);
    BMX_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan64_blocks_kernel, dim3(1), dim3(256), 0, stream, bsum.p, nb);
    BMX_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan64_write_kernel, dim3(nb), dim3(256), 0, stream, ecount.p, n, bsum.p, eoff.p);
    BMX_LAUNCH_CHECK();
    int64_t m = 0;
    int32_t nspilled = 0;
    BMX_HIP(hipMemcpyAsync(&m, eoff.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    BMX_HIP(hipMemcpyAsync(&nspilled, words.p + 1, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    BMX_HIP(hipStreamSynchronize(stream));
    first.reserve(std::max<int64_t>(m, 1));
    second.reserve(std::max<int64_t>(m, 1));
    weight.reserve(std::max<int64_t>(m, 1));
    if (m > 0) {
        if (narrow) launch_cells<uint32_t>(stream, true, idx, n, k, roff.p, rev.p, budget, cap, type, ecount.p, spilled, eoff.p, first.p, second.p, weight.p);
        else launch_cells<unsigned long long>(stream, true, idx, n, k, roff.p, rev.p, budget, cap, type, ecount.p, spilled, eoff.p, first.p, second.p, weight.p);
    }
    BMX_HIP(hipEventRecord(ev.b, stream));
    BMX_HIP(hipEventSynchronize(ev.b));
    float ms = 0.f;
    BMX_HIP(hipEventElapsedTime(&ms, ev.a, ev.b));
    stats().spilled = nspilled;
    stats().graph_us = (int64_t)(1000.0 * ms + 0.5);
    return m;
}

}  // namespace bmx
