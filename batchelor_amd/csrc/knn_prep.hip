// Search preparation of the two candidate tiers of the exact kNN: the prepared 16-bit images of references and queries that
// knn_topk_f16 (knn_f16.hip) and knn_topk_bf16 (knn_bf16.hip) multiply -- their head comments have the number formats --,
// the exact norms, and for tier 1 the queries' margins and seed thresholds.
//
// One workgroup prepares one 32-row tile: rows are staged in LDS with coalesced reads, every output element is computed from
// there, and the tile image (fragment-major for references, row-major for queries -- both contiguous per tile) is written out
// in 16-byte pieces, consecutive threads writing consecutive pieces.  The steps of that are written once, below, and
// instantiated per number format; the tiers differ in how an element of a row becomes 16 bits and in their launches:
//   tier 1 (fp16, scaled)  two launches a search: knn_prep_f16_norms, knn_prep_f16_rq           f16_prep_all
//   tier 2 (split bf16)    a launch per side, knn_prep_bf16, and fold_max_slots for references   bf16_prep
#include "knn_internal.hpp"

#include <cmath>

namespace bmx {
namespace {

using namespace sel;

// ---------------------------------------------------------------------------------------------------
// the number formats: 16-bit conversions, the bit patterns of 1.0 and +inf, and element L of a prepared row (of `columns`
// elements before the three norm pieces) from the row's centred f32 coordinates
// ---------------------------------------------------------------------------------------------------
// tier 1: one fp16 value per coordinate, times the power of two `sf`: every product is exact
struct ScaledF16 {
    static constexpr uint16_t ONE = 0x3C00, INF = 0x7C00;
    float sf;
    __device__ __forceinline__ static uint16_t to_bits(float f) {
        const _Float16 h = (_Float16)f;  // v_cvt_f16_f32: round to nearest even, overflow to infinity
        return __builtin_bit_cast(uint16_t, h);
    }
    __device__ __forceinline__ static float from_bits(uint16_t b) { return (float)__builtin_bit_cast(_Float16, b); }
    __device__ __forceinline__ static int columns(int d) { return d; }
    __device__ __forceinline__ uint16_t element(const float* row, int L, int d, int is_query) const {
        (void)d;
        const float f = row[L] * sf;
        return to_bits(is_query ? -2.f * f : f);
    }
};
// tier 2: three blocks of d columns, block L / d: references [rh | rl | rh], queries (of -2 q) [qh | qh | ql]
struct SplitBf16 {
    static constexpr uint16_t ONE = 0x3F80, INF = 0x7F80;
    __device__ __forceinline__ static uint16_t to_bits(float f) {
        uint32_t u = __float_as_uint(f);
        if ((u & 0x7F800000u) == 0x7F800000u) return (uint16_t)(u >> 16);  // inf / nan pass through
        u += 0x7FFFu + ((u >> 16) & 1u);                                   // round to nearest even
        return (uint16_t)(u >> 16);
    }
    __device__ __forceinline__ static float from_bits(uint16_t b) { return __uint_as_float((uint32_t)b << 16); }
    __device__ __forceinline__ static int columns(int d) { return 3 * d; }
    __device__ __forceinline__ uint16_t element(const float* row, int L, int d, int is_query) const {
        const int blk = (L >= d) + (L >= 2 * d), c = L - blk * d;
        const float f = row[c];
        const float g = is_query ? -2.f * f : f;
        const uint16_t hi = to_bits(g);
        const bool want_lo = is_query ? blk == 2 : blk == 1;
        return want_lo ? to_bits(g - from_bits(hi)) : hi;
    }
};

// ---------------------------------------------------------------------------------------------------
// the steps of a tile's preparation (256 threads)
// ---------------------------------------------------------------------------------------------------
// x / m for 0 <= x < 32 * 128 without an integer division: the float quotient is exact up to +-1
struct QuotRem {
    int q, r;
};
__device__ __forceinline__ QuotRem quot_rem(int x, int m, float inv_m) {
    int q = (int)(((float)x + 0.5f) * inv_m);
    int r = x - q * m;
    if (r < 0) {
        --q;
        r += m;
    } else if (r >= m) {
        ++q;
        r -= m;
    }
    return QuotRem{q, r};
}

// rows r0 .. r0 + 31 of (X, rows), centred and rounded to f32, into xs[32][d]; rows from n on are zero
__device__ __forceinline__ void stage_rows(float* xs, int r0, const double* __restrict__ X, const int32_t* __restrict__ rows,
                                           int n, int d, const double* __restrict__ mean) {
    const float inv_d = 1.0f / (float)d;
    for (int e = threadIdx.x; e < 32 * d; e += 256) {
        const QuotRem rc = quot_rem(e, d, inv_d);
        const int r = r0 + rc.q;
        float f = 0.f;
        if (r < n) {
            const int64_t row = rows ? rows[r] : r;
            f = (float)(X[row * d + rc.r] - mean[rc.r]);
        }
        xs[e] = f;
    }
}

// Eight threads per row: thread (rr, sub) sums the columns sub (mod 8) of staged row rr.  Returns |x~|^2 of the f32-rounded
// centred row (exact products, FP64 sum; any order will do) in all eight.
__device__ __forceinline__ double row_norm2(const float* xs, int rr, int sub, int d) {
    double s = 0.0;
    for (int c = sub; c < d; c += 8) {
        const double f = (double)xs[rr * d + c];
        s += f * f;
    }
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 4);
    return s;
}

// The largest norm of the launch: one atomic per wave, spread over 64 words a cache line apart (a single word serialises the
// whole launch in the L2's atomic unit: it was the bulk of the kernel's time); a fold of the 64 slots finishes.
__device__ __forceinline__ void publish_slot_max(double s, bool live, int block, unsigned long long* __restrict__ max_slots) {
    double m = live ? s : 0.0;
    for (int o = 8; o < 64; o <<= 1) m = fmax(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0)
        atomicMax(max_slots + (size_t)(block & 63) * 16, (unsigned long long)__double_as_longlong(m));
}
// Ordered references (knn_order.hpp): the smallest and the largest key of the launch, the same way, in the second 64-bit word
// of the slots -- low half: the largest bit pattern, high half: the largest complement (keys are >= 0: patterns order like
// values, and zero is the neutral start of both)
__device__ __forceinline__ void publish_slot_key_range(float key, bool live, int block, unsigned long long* __restrict__ max_slots) {
    const uint32_t bits = __float_as_uint(key);
    uint32_t mx = live ? bits : 0u, mn = live ? ~bits : 0u;
    for (int o = 8; o < 64; o <<= 1) {
        mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
        mn = max(mn, (uint32_t)__shfl_xor((int)mn, o));
    }
    if ((threadIdx.x & 63) == 0) {
        uint32_t* w = reinterpret_cast<uint32_t*>(max_slots + (size_t)(block & 63) * 16 + 1);
        atomicMax(w, mx);
        atomicMax(w + 1, mn);
    }
}
__device__ __forceinline__ double fold_slots(const unsigned long long* __restrict__ slots) {  // threads 0 .. 63 (one wave)
    double m = __longlong_as_double((long long)slots[(size_t)threadIdx.x * 16]);
    for (int o = 1; o < 64; o <<= 1) m = fmax(m, __shfl_xor(m, o));
    return m;
}

// 16-byte piece p of a tile image -> the row of the tile and the 8-element chunk of that row it holds
struct Piece {
    int row, chunk;
};
__device__ __forceinline__ Piece piece_of(int p, int NS, int is_query, int shape, float inv_pc) {
    if (is_query) {  // row-major
        const QuotRem rc = quot_rem(p, 2 * NS, inv_pc);
        return Piece{rc.q, rc.r};
    }
    if (shape == 0) {  // 32x32 fragments: k-step, lane half, row
        const int ih = p >> 5;  // = 2 * k-step + lane half
        return Piece{p & 31, (ih & 1) * NS + (ih >> 1)};
    }
    // 16x16x32 fragments (even NS): piece p is lane p & 63 of fragment f = 2 * k-step + reference half; the lane holds
    // row 16 * half + (lane & 15), and of the row's four stretches of 4 NS columns the (lane >> 4)-th, as the query's
    // lane does of its (row-major) row
    const int l = p & 63, f = p >> 6;
    return Piece{16 * (f & 1) + (l & 15), (l >> 4) * (NS >> 1) + (f >> 1)};
}

// an f32 as three 16-bit pieces whose sum reproduces it exactly
template <class F>
__device__ __forceinline__ void split_norm3(float nf, uint16_t (&n3)[3]) {
    n3[0] = F::to_bits(nf);
    const float r1 = nf - F::from_bits(n3[0]);
    n3[1] = F::to_bits(r1);
    n3[2] = F::to_bits(r1 - F::from_bits(n3[1]));
}

// element e of a 16-byte piece (eight 16-bit values in four words; the even element of a word comes first and sets it)
__device__ __forceinline__ void pack16(uint32_t (&w)[4], int e, uint16_t v) {
    if (e & 1)
        w[e >> 1] |= (uint32_t)v << 16;
    else
        w[e >> 1] = v;
}

// The tile image of the staged rows xs[32][d] with norms nrm[32], 16 NS elements a row: the format's columns, then three
// columns that carry the norm into the product -- a reference's |r|^2 in three pieces against a query's 1 1 1 (a padded
// reference: +inf, it never passes a threshold; a padded query: all zero) --, then zeros.
template <class F>
__device__ __forceinline__ void write_tile_image(const F& fmt, uint16_t* __restrict__ P, const float* xs, const float* nrm,
                                                 int r0, int n, int d, int NS, int is_query, int shape) {
    uint4* out = reinterpret_cast<uint4*>(P + (int64_t)r0 * (16 * NS));
    const int npieces = 32 * 2 * NS;
    const int ncol = F::columns(d);
    const float inv_pc = 1.0f / (float)(2 * NS);
    for (int p = threadIdx.x; p < npieces; p += 256) {
        const Piece pc = piece_of(p, NS, is_query, shape, inv_pc);
        const bool plive = r0 + pc.row < n;
        uint16_t n3[3];
        split_norm3<F>(nrm[pc.row], n3);
        uint32_t w[4];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int L = 8 * pc.chunk + e;
            uint16_t v = 0;
            if (L < ncol) {
                v = fmt.element(xs + pc.row * d, L, d, is_query);
            } else if (L < ncol + 3) {
                const int piece = L - ncol;
                if (is_query)
                    v = plive ? F::ONE : 0;
                else if (!plive)
                    v = piece == 0 ? F::INF : 0;
                else
                    v = piece == 0 ? n3[0] : (piece == 1 ? n3[1] : n3[2]);
            }
            pack16(w, e, v);
        }
        out[p] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// ---------------------------------------------------------------------------------------------------
// tier 2: one launch per side
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void knn_prep_bf16(const double* __restrict__ X, const int32_t* __restrict__ rows, int n,
                                                     int d, int NS, const double* __restrict__ mean, int is_query,
                                                     uint16_t* __restrict__ P, double* __restrict__ n2,
                                                     unsigned long long* __restrict__ max_slots) {
    extern __shared__ __attribute__((aligned(16))) char smem_pp[];
    float* xs = reinterpret_cast<float*>(smem_pp);  // [32][d] centred, rounded to f32
    float* nrm = xs + 32 * d;                       // [32] f32(|x~|^2): its three bf16 pieces reproduce it exactly
    const int r0 = blockIdx.x * 32;
    stage_rows(xs, r0, X, rows, n, d, mean);
    __syncthreads();
    const int rr = threadIdx.x >> 3, sub = threadIdx.x & 7;
    const bool live = r0 + rr < n;
    const double s = row_norm2(xs, rr, sub, d);
    if (sub == 0) {
        nrm[rr] = (float)s;
        if (live) n2[r0 + rr] = s;
    }
    if (!is_query) publish_slot_max(s, live, blockIdx.x, max_slots);
    __syncthreads();
    write_tile_image(SplitBf16{}, P, xs, nrm, r0, n, d, NS, is_query, 0);
}

__global__ void fold_max_slots(const unsigned long long* __restrict__ slots, unsigned long long* __restrict__ out) {
    const double m = fold_slots(slots);
    if (threadIdx.x == 0) atomicMax(out, (unsigned long long)__double_as_longlong(m));
}

// ---------------------------------------------------------------------------------------------------
// tier 1.  PHASE 0 (references only): centred f32 rows -> exact norms n2[] and their maximum (the scale needs it before
// anything is written).  PHASE 1: the fp16 tile images, scaled.
// ---------------------------------------------------------------------------------------------------
// One tile of 32 rows (tile number `block`).  scale: PHASE 1 only.
template <int PHASE>
__device__ __forceinline__ void prep_rows_f16(char* smem_pp, int block, const double* __restrict__ X,
                                              const int32_t* __restrict__ rows, int n, int d, int NS, int shape,
                                              const double* __restrict__ mean, int is_query, uint16_t* __restrict__ P,
                                              double* __restrict__ n2, unsigned long long* __restrict__ max_slots,
                                              double scale) {
    float* xs = reinterpret_cast<float*>(smem_pp);  // [32][d] centred, rounded to f32
    float* nrm = xs + 32 * d;                       // [32] f32(|x'|^2), scaled: three fp16 pieces reproduce it exactly (33 bits)
    const int r0 = block * 32;
    stage_rows(xs, r0, X, rows, n, d, mean);
    __syncthreads();
    const int rr = threadIdx.x >> 3, sub = threadIdx.x & 7;
    const bool live = r0 + rr < n;
    const double s = row_norm2(xs, rr, sub, d);
    if constexpr (PHASE == 0) {
        if (sub == 0 && live) n2[r0 + rr] = s;
        publish_slot_max(s, live, block, max_slots);
        return;
    }
    const ScaledF16 fmt{(float)scale};
    if (is_query) {
        // a query so far out that -2 q' leaves the fp16 range cannot be handled here: poison its norm, the
        // certificate of knn_refine then fails and the query goes to the next tier
        bool bad = false;
        for (int c = sub; c < d; c += 8) bad |= !(fabsf(-2.f * xs[rr * d + c] * fmt.sf) <= 65504.f);
        bad |= __shfl_xor((int)bad, 1) != 0;
        bad |= __shfl_xor((int)bad, 2) != 0;
        bad |= __shfl_xor((int)bad, 4) != 0;
        if (sub == 0 && live) n2[r0 + rr] = bad ? __builtin_nan("") : s;
    } else if (n2) {
        // references of an ordered search (n2 is null otherwise): the norms follow the image, like everything indexed by image row
        if (sub == 0 && live) n2[r0 + rr] = s;
    }
    if (sub == 0) nrm[rr] = (float)(s * scale * scale);
    __syncthreads();
    write_tile_image(fmt, P, xs, nrm, r0, n, d, NS, is_query, shape);
}

// PHASE 0 over the references: norms + the 64 slot maxima (the slots are zero when the search starts).  With a query centre
// (ordered references, knn_order.hpp) also every row's key |r - qcentre|^2 from the rows already staged, and the keys' range:
// f32 throughout -- the key only decides where a row goes in the image, its precision does not matter, that it is the same
// number every time does (one fixed order of summation).
__global__ __launch_bounds__(256) void knn_prep_f16_norms(const double* __restrict__ X, const int32_t* __restrict__ rows, int n,
                                                          int d, int NS, const double* __restrict__ mean,
                                                          double* __restrict__ n2, unsigned long long* __restrict__ max_slots,
                                                          const double* __restrict__ qcentre, float* __restrict__ key) {
    extern __shared__ __attribute__((aligned(16))) char smem_pp[];
    prep_rows_f16<0>(smem_pp, blockIdx.x, X, rows, n, d, NS, 0, mean, 0, nullptr, n2, max_slots, 1.0);
    if (!key) return;
    const float* xs = reinterpret_cast<const float*>(smem_pp);  // [32][d] as staged
    float* dq = reinterpret_cast<float*>(smem_pp) + 32 * d + 32;  // [d] the query centre, relative to `mean` like the rows
    for (int c = threadIdx.x; c < d; c += 256) dq[c] = (float)(qcentre[c] - mean[c]);
    __syncthreads();
    const int rr = threadIdx.x >> 3, sub = threadIdx.x & 7;
    const bool live = blockIdx.x * 32 + rr < n;
    float kq = 0.f;
    for (int c = sub; c < d; c += 8) {
        const float t = xs[rr * d + c] - dq[c];
        kq += t * t;
    }
    kq += __shfl_xor(kq, 1);
    kq += __shfl_xor(kq, 2);
    kq += __shfl_xor(kq, 4);
    if (sub == 0 && live) key[blockIdx.x * 32 + rr] = kq;
    publish_slot_key_range(kq, live, blockIdx.x, max_slots);
}

// PHASE 1 of references AND queries in one launch (workgroups [0, nrb): reference tiles, the others: query tiles), with
// what used to be four more launches folded in: every workgroup folds the 64 slot maxima itself (workgroup 0 leaves the
// result in *max_n2_bits for the kernels behind and zeroes the search's flagged-query counter); the query workgroups write
// each query's margin (twice the pass's error bound) and, for a seeded search, its seed threshold -- tau_seed, which the
// sample pass folds into the thresholds it publishes, or straight into tau_g when there is no sample pass (tau_init).
__global__ __launch_bounds__(256) void knn_prep_f16_rq(const double* __restrict__ X, const int32_t* __restrict__ rrows, int nr,
                                                       int nrb, const double* __restrict__ Q,
                                                       const int32_t* __restrict__ qrows, int nq, int d, int NS, int shape,
                                                       const double* __restrict__ mean, uint16_t* __restrict__ Pr,
                                                       uint16_t* __restrict__ Pq, double* __restrict__ rn2,
                                                       double* __restrict__ qn2, const unsigned long long* __restrict__ slots,
                                                       unsigned long long* __restrict__ max_n2_bits,
                                                       int32_t* __restrict__ flagged0, float* __restrict__ margin, PassEps pe,
                                                       const float* __restrict__ seed_d2, uint32_t* __restrict__ tau_seed,
                                                       uint32_t* __restrict__ tau_init) {
    extern __shared__ __attribute__((aligned(16))) char smem_pp[];
    __shared__ double sh_max;
    if (threadIdx.x < 64) {
        const double m = fold_slots(slots);
        if (threadIdx.x == 0) {
            sh_max = m;
            if (blockIdx.x == 0) {
                *max_n2_bits = (unsigned long long)__double_as_longlong(m);
                if (flagged0) *flagged0 = 0;
            }
        }
    }
    __syncthreads();
    const double max_rn2 = sh_max;
    const double scale = pass_scale(max_rn2);
    if ((int)blockIdx.x < nrb) {
        prep_rows_f16<1>(smem_pp, blockIdx.x, X, rrows, nr, d, NS, shape, mean, 0, Pr, rn2, nullptr, scale);
        return;
    }
    const int qb = blockIdx.x - nrb;
    prep_rows_f16<1>(smem_pp, qb, Q, qrows, nq, d, NS, shape, mean, 1, Pq, qn2, nullptr, scale);
    const int rr = threadIdx.x >> 3, sub = threadIdx.x & 7;
    if (sub == 0) {
        const int q = qb * 32 + rr;
        const bool live = q < nq;
        // (a query that left the fp16 range has a NaN norm in qn2: its margin and threshold are NaN-safe -- it fails the
        // certificate whatever the pass collects)
        const double nn = live ? qn2[q] : 0.0;
        if (margin) margin[q] = live ? pass_margin(nn, max_rn2, pe) : 0.f;
        uint32_t ts = 0xFF800000u;  // the orderable image of +inf: no seed
        if (seed_d2) ts = live ? pass_seed_tau((double)seed_d2[q], nn, max_rn2, pe) : f32_orderable(-__builtin_inff());
        if (tau_seed) tau_seed[q] = ts;
        if (tau_init) tau_init[q] = ts;
    }
}

}  // namespace

// Tier 1: references (norm pass, then the scaled image) and queries (image, norm, margin, seed threshold) of one search: two
// launches.  `slots` (64 x 16 words) must be zero on entry -- knn_refine leaves them so for the next search.
// ord (nullable): ordered references -- the norm pass also leaves the keys, ref_order_build (knn_order.hip) the two index
// arrays, and the image (Pr) is written in that order; the image launch then rewrites rn2 in image order too.
void f16_prep_all(hipStream_t stream, const double* X, const int32_t* rrows, int nr, int nr_pad, const double* Q,
                  const int32_t* qrows, int nq, int nq_pad, int d, int NS, int shape, const double* mean, uint16_t* Pr, uint16_t* Pq,
                  double* rn2, double* qn2, unsigned long long* maxbits, unsigned long long* slots, int32_t* flagged0,
                  float* margin, const PassEps& pe, const float* seed_d2, uint32_t* tau_seed, uint32_t* tau_init,
                  const RefOrder* ord) {
    const size_t lds = (size_t)32 * d * 4 + 128 + 16;
    hipLaunchKernelGGL(knn_prep_f16_norms, dim3(nr_pad / 32), dim3(256), lds + (ord ? (size_t)d * 4 : 0), stream, X, rrows, nr, d,
                       NS, mean, rn2, slots, ord ? ord->qcentre : nullptr, ord ? ord->key : nullptr);
    BMX_LAUNCH_CHECK();
    if (ord) {  // the image in key order: its tiles gather their rows of X through img_src
        ref_order_build(stream, ord->key, nr, rrows, slots, ord->scratch, ord->img_src, ord->img_pos);
        rrows = ord->img_src;
    }
    hipLaunchKernelGGL(knn_prep_f16_rq, dim3(nr_pad / 32 + nq_pad / 32), dim3(256), lds, stream, X, rrows, nr, nr_pad / 32, Q, qrows,
                       nq, d, NS, shape, mean, Pr, Pq, ord ? rn2 : nullptr, qn2, (const unsigned long long*)slots, maxbits, flagged0, margin, pe, seed_d2,
                       tau_seed, tau_init);
    BMX_LAUNCH_CHECK();
}

// Tier 2: one side of a search (is_query = 0: the references, whose largest norm goes to *maxbits through the slots).
void bf16_prep(hipStream_t stream, const double* X, const int32_t* rows, int n, int n_pad, int d, int NS,
               const double* mean, int is_query, uint16_t* P, double* n2, unsigned long long* maxbits,
               unsigned long long* slots) {
    const size_t lds = (size_t)32 * d * 4 + 128 + 16;
    if (!is_query) BMX_HIP(hipMemsetAsync(slots, 0, 64 * 16 * sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(knn_prep_bf16, dim3(n_pad / 32), dim3(256), lds, stream, X, rows, n, d, NS, mean, is_query, P, n2, slots);
    BMX_LAUNCH_CHECK();
    if (!is_query) {
        hipLaunchKernelGGL(fold_max_slots, dim3(1), dim3(64), 0, stream, slots, maxbits);
        BMX_LAUNCH_CHECK();
    }
}

}  // namespace bmx
