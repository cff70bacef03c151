// Tier 1 of the exact kNN, search preparation: the prepared fp16 images of references and queries that knn_topk_f16
// (knn_f16.hip, whose head comment has the number format) multiplies, the exact norms, the queries' margins and seed
// thresholds.  Two launches a search.
#include "knn_internal.hpp"

#include <cmath>

namespace bmx {
namespace {

using namespace sel;

__device__ __forceinline__ uint16_t f32_to_f16_bits(float f) {
    const _Float16 h = (_Float16)f;  // v_cvt_f16_f32: round to nearest even, overflow to infinity
    return __builtin_bit_cast(uint16_t, h);
}
__device__ __forceinline__ float f16_bits_to_f32(uint16_t b) { return (float)__builtin_bit_cast(_Float16, b); }

// power-of-two scale that puts the largest reference norm into (24, 48]; 1 for degenerate input
__host__ __device__ __forceinline__ double f16_scale(double max_n2) {
    const double rm = sqrt(max_n2);
    if (!(rm > 1e-150) || !(rm < 1e150)) return 1.0;
    int e = 0;
    (void)frexp(48.0 / rm, &e);  // 48 / rm = f * 2^e, f in [0.5, 1)
    return ldexp(1.0, e - 1);
}

// ---------------------------------------------------------------------------------------------------
// prep.  PHASE 0 (references only): centred f32 rows -> exact norms n2[] and their maximum (the scale needs it
// before anything is written).  PHASE 1: the fp16 tile images (fragment-major for references, row-major for
// queries; same addressing as knn_prep_bf16), scaled.
// ---------------------------------------------------------------------------------------------------
// One tile of 32 rows (tile number `block`).  scale: PHASE 1 only.  Returns the row's exact squared norm (the eight threads
// of a row all hold it).
template <int PHASE>
__device__ __forceinline__ double prep_rows(char* smem_pp, int block, const double* __restrict__ X,
                                            const int32_t* __restrict__ rows, int n, int d, int NS, int shape,
                                            const double* __restrict__ mean, int is_query, uint16_t* __restrict__ P,
                                            double* __restrict__ n2, unsigned long long* __restrict__ max_slots,
                                            double scale) {
    const int K = 16 * NS;
    float* xs = reinterpret_cast<float*>(smem_pp);  // [32][d] centred, rounded to f32
    float* nrm = xs + 32 * d;                       // [32] f32(|x'|^2), scaled
    const int tid = threadIdx.x;
    const int r0 = block * 32;
    const float inv_d = 1.0f / (float)d;
    for (int e = tid; e < 32 * d; e += 256) {
        int rr = (int)(((float)e + 0.5f) * inv_d);  // e < 32 * 128: the float quotient is exact up to +-1
        int c = e - rr * d;
        if (c < 0) {
            --rr;
            c += d;
        } else if (c >= d) {
            ++rr;
            c -= d;
        }
        const int r = r0 + rr;
        float f = 0.f;
        if (r < n) {
            const int64_t row = rows ? rows[r] : r;
            f = (float)(X[row * d + c] - mean[c]);
        }
        xs[e] = f;
    }
    __syncthreads();
    const int rr = tid >> 3, sub = tid & 7;  // eight threads per row
    const bool live = r0 + rr < n;
    double s = 0.0;  // |x~|^2 of the f32-rounded centred row (exact products, FP64 sum)
    for (int c = sub; c < d; c += 8) {
        const double f = (double)xs[rr * d + c];
        s += f * f;
    }
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 4);
    if constexpr (PHASE == 0) {
        if (sub == 0 && live) n2[r0 + rr] = s;
        double m = live ? s : 0.0;
        for (int o = 8; o < 64; o <<= 1) m = fmax(m, __shfl_xor(m, o));
        if ((tid & 63) == 0)  // one atomic per wave, spread over 64 words a cache line apart
            atomicMax(max_slots + (size_t)(block & 63) * 16, (unsigned long long)__double_as_longlong(m));
        return s;
    }
    const float sf = (float)scale;  // a power of two: every product below is exact
    if (is_query) {
        // a query so far out that -2 q' leaves the fp16 range cannot be handled here: poison its norm, the
        // certificate of knn_refine then fails and the query goes to the next tier
        bool bad = false;
        for (int c = sub; c < d; c += 8) bad |= !(fabsf(-2.f * xs[rr * d + c] * sf) <= 65504.f);
        bad |= __shfl_xor((int)bad, 1) != 0;
        bad |= __shfl_xor((int)bad, 2) != 0;
        bad |= __shfl_xor((int)bad, 4) != 0;
        if (sub == 0 && live) n2[r0 + rr] = bad ? __builtin_nan("") : s;
    }
    if (sub == 0) nrm[rr] = (float)(s * scale * scale);
    __syncthreads();
    uint4* out = reinterpret_cast<uint4*>(P + (int64_t)r0 * K);
    const int npieces = 32 * 2 * NS;
    const float inv_pc = 1.0f / (float)(2 * NS);
    for (int p = tid; p < npieces; p += 256) {
        int prow, i;  // row of the tile, 8-element chunk of the row
        if (is_query) {
            prow = (int)(((float)p + 0.5f) * inv_pc);
            i = p - prow * 2 * NS;
            if (i < 0) {
                --prow;
                i += 2 * NS;
            } else if (i >= 2 * NS) {
                ++prow;
                i -= 2 * NS;
            }
        } else if (shape == 0) {
            prow = p & 31;
            const int ih = p >> 5;  // = 2 * k-step + lane half
            i = (ih & 1) * NS + (ih >> 1);
        } else {
            // 16x16x32 fragments (even NS): piece p is lane p & 63 of fragment f = 2 * k-step + reference half; the lane holds
            // row 16 * half + (lane & 15), and of the row's four stretches of 4 NS columns the (lane >> 4)-th, as the query's
            // lane does of its (row-major) row
            const int l = p & 63, f = p >> 6;
            prow = 16 * (f & 1) + (l & 15);
            i = (l >> 4) * (NS >> 1) + (f >> 1);
        }
        const bool plive = r0 + prow < n;
        const float nf = nrm[prow];  // three fp16 pieces reproduce the f32 value exactly (33 bits)
        const uint16_t na = f32_to_f16_bits(nf);
        const float nr1 = nf - f16_bits_to_f32(na);
        const uint16_t nb = f32_to_f16_bits(nr1);
        const uint16_t nc = f32_to_f16_bits(nr1 - f16_bits_to_f32(nb));
        uint32_t w[4];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int L = 8 * i + e;
            uint16_t v = 0;
            if (L < d) {
                const float f = xs[prow * d + L] * sf;
                v = f32_to_f16_bits(is_query ? -2.f * f : f);
            } else if (L < d + 3) {
                const int piece = L - d;
                if (is_query)
                    v = plive ? 0x3C00 : 0;  // 1.0 (padded queries stay all-zero)
                else if (!plive)
                    v = piece == 0 ? 0x7C00 : 0;  // +inf: a padded reference never passes a threshold
                else
                    v = piece == 0 ? na : (piece == 1 ? nb : nc);
            }
            if (e & 1)
                w[e >> 1] |= (uint32_t)v << 16;
            else
                w[e >> 1] = v;
        }
        out[p] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    return s;
}

// PHASE 0 over the references: norms + the 64 slot maxima (the slots are zero when the search starts)
__global__ __launch_bounds__(256) void knn_prep_f16_norms(const double* __restrict__ X, const int32_t* __restrict__ rows, int n,
                                                          int d, int NS, const double* __restrict__ mean,
                                                          double* __restrict__ n2, unsigned long long* __restrict__ max_slots) {
    extern __shared__ __attribute__((aligned(16))) char smem_pp[];
    (void)prep_rows<0>(smem_pp, blockIdx.x, X, rows, n, d, NS, 0, mean, 0, nullptr, n2, max_slots, 1.0);
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
        double m = __longlong_as_double((long long)slots[(size_t)threadIdx.x * 16]);
        for (int o = 1; o < 64; o <<= 1) m = fmax(m, __shfl_xor(m, o));
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
    const double scale = f16_scale(max_rn2);
    if ((int)blockIdx.x < nrb) {
        (void)prep_rows<1>(smem_pp, blockIdx.x, X, rrows, nr, d, NS, shape, mean, 0, Pr, rn2, nullptr, scale);
        return;
    }
    const int qb = blockIdx.x - nrb;
    const double s = prep_rows<1>(smem_pp, qb, Q, qrows, nq, d, NS, shape, mean, 1, Pq, qn2, nullptr, scale);
    const int rr = threadIdx.x >> 3, sub = threadIdx.x & 7;
    if (sub == 0) {
        const int q = qb * 32 + rr;
        const bool live = q < nq;
        // (a query that left the fp16 range has a NaN norm in qn2: its margin and threshold are NaN-safe -- it fails the
        // certificate whatever the pass collects)
        const double nn = live ? qn2[q] : 0.0;
        (void)s;
        if (margin) margin[q] = live ? pass_margin(nn, max_rn2, pe) : 0.f;
        uint32_t ts = 0xFF800000u;  // the orderable image of +inf: no seed
        if (seed_d2) ts = live ? pass_seed_tau((double)seed_d2[q], nn, max_rn2, pe) : f32_orderable(-__builtin_inff());
        if (tau_seed) tau_seed[q] = ts;
        if (tau_init) tau_init[q] = ts;
    }
}

}  // namespace

// References (norm pass, then the scaled image) and queries (image, norm, margin, seed threshold) of one search: two
// launches.  `slots` (64 x 16 words) must be zero on entry -- knn_refine leaves them so for the next search.
void f16_prep_all(hipStream_t stream, const double* X, const int32_t* rrows, int nr, int nr_pad, const double* Q,
                  const int32_t* qrows, int nq, int nq_pad, int d, int NS, int shape, const double* mean, uint16_t* Pr, uint16_t* Pq,
                  double* rn2, double* qn2, unsigned long long* maxbits, unsigned long long* slots, int32_t* flagged0,
                  float* margin, const PassEps& pe, const float* seed_d2, uint32_t* tau_seed, uint32_t* tau_init) {
    const size_t lds = (size_t)32 * d * 4 + 128 + 16;
    hipLaunchKernelGGL(knn_prep_f16_norms, dim3(nr_pad / 32), dim3(256), lds, stream, X, rrows, nr, d, NS, mean, rn2, slots);
    BMX_LAUNCH_CHECK();
    hipLaunchKernelGGL(knn_prep_f16_rq, dim3(nr_pad / 32 + nq_pad / 32), dim3(256), lds, stream, X, rrows, nr, nr_pad / 32, Q, qrows,
                       nq, d, NS, shape, mean, Pr, Pq, rn2, qn2, (const unsigned long long*)slots, maxbits, flagged0, margin, pe, seed_d2,
                       tau_seed, tau_init);
    BMX_LAUNCH_CHECK();
}

double f16_scale_host(double max_n2) { return f16_scale(max_n2); }

}  // namespace bmx
