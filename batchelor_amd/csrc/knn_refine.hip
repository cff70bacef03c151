// The FP64 re-rank behind a candidate pass of the exact kNN (knn.hip): knn_refine (a wave per query), knn_refine_half (half a
// wave per query, for queries with one list of at most 32 candidates) and their launch, refine_launch.
#include "knn_fp64.hpp"
#include "knn_internal.hpp"

#include <type_traits>

namespace bmx {
namespace {

using namespace sel;

// ---------------------------------------------------------------------------------------------------
// refine: exact FP64 re-rank of the candidates + certification.  One wave per query.
//   1. the candidates of all reference ranges are gathered into one dense list (ordered references, knn_order.hpp: the
//      pass lists image rows, which become reference positions here, through img_pos -- positions from there on);
//   2. they are ranked by their approximate values: only the KS best go on (the first one cut bounds all the others
//      from below and enters the certificate), and of those only the ones within twice the error bound of the k-th
//      best -- a candidate further out is provably farther than k others, so its exact distance is never needed;
//   3. FP64 distances (the CPU's summation order, bit for bit), exact (distance, index) ranking;
//   4. certificate: every reference the candidate pass rejected had an approximate value >= tau, i.e. an exact
//      squared distance >= tau + |q~|^2 - eps, so the top k is proven when the k-th exact distance is below that.
// Values of a scaled pass (fp16 tier: coordinates times the power of two s) are brought back with 1 / s^2.
// ---------------------------------------------------------------------------------------------------
constexpr int REFINE_MAXM = MAX_CHUNKS * 48;


typedef double d2 __attribute__((ext_vector_type(2)));

// ---- the pieces the two forms share ---------------------------------------------------------------------------------
// error bound of the candidate pass for one query (unscaled units), and the scale its values come back with
struct PassError {
    double s, s2inv, eps;
};
__device__ __forceinline__ PassError pass_error(double qn2q, const unsigned long long* __restrict__ max_rn2_bits, int scaled,
                                                double eps_k, double eps_qr, double eps_split, double eps_den) {
    const double max_rn2 = __longlong_as_double((long long)*max_rn2_bits);
    const double s = scaled ? pass_scale(max_rn2) : 1.0;
    const double s2inv = 1.0 / (s * s);
    const double eps = pass_bound(qn2q, max_rn2, s, scaled, eps_k, eps_qr, eps_split, eps_den);
    return PassError{s, s2inv, eps};
}

// lane p of a quad: its NC 16-byte pieces of a row of np pieces (piece 4 c + p; zero beyond the row)
template <int NC>
__device__ __forceinline__ void quad_load(d2 (&v)[NC], const d2* __restrict__ row2, int p, int np) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        v[c] = d2{0.0, 0.0};
        if (4 * c + p < np) v[c] = row2[4 * c + p];
    }
}

// Four lanes per candidate row: their 16-byte loads are 64 contiguous bytes of the (randomly placed) row, so every cache
// line of it is asked for twice instead of eight times as with a lane per row.  The sum stays the reference's: one running
// value per row, handed from lane to lane of the quad (DPP) every two elements, strictly left to right (compiled with
// -ffp-contract=off: bit for bit the CPU's sum).  x: this lane's pieces of the query (quad_load).  Returns the lane's running
// sum: the row's squared distance on lane (np - 1) & 3 of the quad.  Every lane of the wave calls it (DPP).
template <int NC>
__device__ __forceinline__ double quad_chain_d2(const d2 (&x)[NC], const double* __restrict__ row, int p, int np) {
    d2 y[NC];
    quad_load<NC>(y, reinterpret_cast<const d2*>(row), p, np);
    // the squares: every lane its own two per piece, all at once; only the additions have an order
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const double t0 = x[c][0] - y[c][0], t1 = x[c][1] - y[c][1];
        y[c][0] = t0 * t0;
        y[c][1] = t1 * t1;
    }
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        if (4 * c < np) {  // (wave-uniform)
#pragma unroll
            for (int ph = 0; ph < 4; ++ph) {
                // the running sum as the previous lane of the quad has it (lane 0: lane 3's, from the piece before)
                const unsigned long long bits = (unsigned long long)__double_as_longlong(acc);
                const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)bits, 0x93, 0xF, 0xF, false);
                const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(bits >> 32), 0x93, 0xF, 0xF, false);
                const double prev = __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
                // (0 + x is x exactly: the first element needs no case of its own -- prev is lane 3's untouched 0)
                double run = prev + y[c][0];
                run += y[c][1];
                if (p == ph && 4 * c + ph < np) acc = run;
            }
        }
    }
    return acc;
}

// 4. the certificate, on one lane of the query: every reference the candidate pass rejected had an approximate value >= tmin.
// A query that is not proven is listed with its k-th candidate distance: the true k-th neighbour is no farther.
__device__ __forceinline__ void certify(double kth, double kth_full, float tmin, const PassError& pe, double qn2q, bool full,
                                        int q, int32_t* __restrict__ flagged, double* __restrict__ flag_bound,
                                        double* __restrict__ kth_out) {
    const bool proven = kth < (double)tmin * pe.s2inv + qn2q - pe.eps;
    if (!proven) {
        const int pos = atomicAdd(&flagged[0], 1);
        flagged[1 + pos] = q;
        flag_bound[pos] = kth;
    }
    // the largest distance of a certified FULL row (what the intersection's probe rejects against without reading the
    // row); +inf where the row is short or may still be rewritten: the probe then reads the row
    if (kth_out) kth_out[q] = (proven && full) ? sqrt(kth_full) : __builtin_inf();
}

template <int REFINE_NC>  // pieces of 8 doubles (one 16-byte load per lane of a quad) a row may have; 0: lane-per-row gather
__global__ __launch_bounds__(256) void knn_refine(const double* __restrict__ X, const int32_t* __restrict__ ref_rows,
                                                  const double* __restrict__ Q, const int32_t* __restrict__ q_rows,
                                                  int nq, int d, int k, int KS, int nchunks, double eps_k, double eps_qr,
                                                  double eps_split, double eps_den, int scaled,
                                                  const int32_t* __restrict__ cand, const float* __restrict__ cand_v,
                                                  const float* __restrict__ tau, const double* __restrict__ qn2,
                                                  const unsigned long long* __restrict__ max_rn2_bits,
                                                  const float* __restrict__ seed_d2, int32_t* __restrict__ idx_out,
                                                  double* __restrict__ dist_out, int32_t* __restrict__ flagged,
                                                  double* __restrict__ flag_bound,
                                                  unsigned long long* __restrict__ zero_slots, int q0,
                                                  double* __restrict__ kth_out, int sq = 0,
                                                  const int32_t* __restrict__ img_pos = nullptr) {
    __shared__ __attribute__((aligned(16))) double sd[4][REFINE_MAXM];
    __shared__ int si[4][REFINE_MAXM];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // (the prep kernels' 64 slot maxima have been folded by now: left zeroed for the next search's norm pass)
    if (zero_slots && blockIdx.x == 0 && threadIdx.x < 64) {
        zero_slots[(size_t)threadIdx.x * 16] = 0ull;
        zero_slots[(size_t)threadIdx.x * 16 + 1] = 0ull;  // (the keys' range of an ordered search)
    }
    const int q = q0 + blockIdx.x * 4 + w;  // (queries [q0, nq): the ones in front go through knn_refine_half)
    if (q >= nq) return;
    const int Mall = nchunks * KS;
    const double* qv = Q + (int64_t)(q_rows ? q_rows[q] : q) * d;
    const PassError pe = pass_error(qn2[q], max_rn2_bits, scaled, eps_k, eps_qr, eps_split, eps_den);
    const double s = pe.s, eps = pe.eps;
    // 1. dense list of the valid candidates (ballot prefix)
    int M = 0;
    // this wave's sd row doubles as the list of rank keys until the exact distances go there: (order-preserving image
    // of the approximate value) << 32 | index -- unique, and ordered like (value, index)
    unsigned long long* sk = reinterpret_cast<unsigned long long*>(&sd[w][0]);
    for (int m0 = 0; m0 < Mall; m0 += 64) {
        const int m = m0 + lane;
        int id = m < Mall ? cand[(int64_t)q * Mall + m] : -1;
        if (img_pos && id >= 0) id = img_pos[id];  // ordered references: image row -> reference position, positions from here on
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(id >= 0);
        const int pos = M + __builtin_popcountll(mask & ((1ull << lane) - 1ull));
        if (id >= 0) {
            si[w][pos] = id;
            if (cand_v) sk[pos] = ((unsigned long long)f32_orderable(cand_v[(int64_t)q * Mall + m]) << 32) | (uint32_t)id;
        }
        M += __builtin_popcountll(mask);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // 2. rank by approximate value
    float tmerge = __builtin_inff();
    if (cand_v && M > k) {
        constexpr int NU = (REFINE_MAXM + 63) / 64;
        int rk[NU], ids[NU];
        float vs[NU];
        float vk = __builtin_inff();  // k-th smallest approximate value
#pragma unroll
        for (int uu = 0; uu < NU; ++uu) {
            const int m = lane + 64 * uu;
            rk[uu] = 0x7FFFFFFF;
            ids[uu] = 0;
            vs[uu] = 0.f;
            if (m < M) {
                const unsigned long long km = sk[m];
                const float vm = orderable_f32((uint32_t)(km >> 32));
                int rank = 0;
                int f = 0;
                for (; f + 2 <= M; f += 2) {  // (16-byte reads: the row is 16-byte aligned, f even)
                    typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
                    const u64x2 kf = *reinterpret_cast<const u64x2*>(sk + f);
                    rank += (kf[0] < km ? 1 : 0) + (kf[1] < km ? 1 : 0);
                }
                if (f < M) rank += sk[f] < km ? 1 : 0;
                rk[uu] = rank;
                ids[uu] = (int)(uint32_t)km;
                vs[uu] = vm;
                if (rank == k - 1) vk = vm;
                if (rank == KS) tmerge = vm;  // the first one cut by rank bounds all the others cut from below
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            tmerge = fminf(tmerge, __shfl_xor(tmerge, o));
            vk = fminf(vk, __shfl_xor(vk, o));
        }
        // a candidate whose approximate value exceeds the k-th best by more than twice the bound is farther (exactly)
        // than each of the k best: it cannot be among the k nearest, whatever else happens
        const float cut = (float)((double)vk + 2.0 * eps * (s * s) * 1.0000002 + 1e-30);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        int Mn = 0;
#pragma unroll
        for (int uu = 0; uu < NU; ++uu) {
            if (uu * 64 < M) {
                const bool keep = rk[uu] < KS && vs[uu] <= cut;
                const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
                if (keep) si[w][Mn + __builtin_popcountll(mask & ((1ull << lane) - 1ull))] = ids[uu];
                Mn += __builtin_popcountll(mask);
            }
        }
        M = Mn;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    // 3. exact distances and ranks
    if constexpr (REFINE_NC > 0) {
        // a quad of lanes per candidate row (quad_chain_d2), 16 rows a trip
        const int g = lane >> 2, p = lane & 3;
        const int np = d >> 1;  // 16-byte pieces per row
        d2 x[REFINE_NC];
        quad_load<REFINE_NC>(x, reinterpret_cast<const d2*>(qv), p, np);
        const int p_last = (np - 1) & 3;
        for (int r0 = 0; r0 < M; r0 += 16) {
            const int m = r0 + g;
            const int id = si[w][m < M ? m : 0];
            const double acc = quad_chain_d2<REFINE_NC>(x, X + (int64_t)(ref_rows ? ref_rows[id] : id) * d, p, np);
            if (p == p_last && m < M) sd[w][m] = acc;
        }
    } else {
        for (int m = lane; m < M; m += 64) {
            const int id = si[w][m];
            sd[w][m] = exact_d2(qv, X + (int64_t)(ref_rows ? ref_rows[id] : id) * d, d);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // fewer than k candidates: never certified -- unless the search was seeded, where the row is complete as soon as
    // nothing within the seed distance can have been rejected: the seed then plays the k-th distance's part
    const double seed = seed_d2 ? (double)seed_d2[q] : __builtin_inf();
    double kth = M >= k ? 0.0 : seed;
    // (an unseeded row short of candidates is never certified and is rewritten by the exact sweep -- but an optimistic run
    // reads it before the host has seen the flag: its unused places hold a valid position, not whatever was there)
    for (int m = M + lane; m < k; m += 64) idx_out[(int64_t)q * k + m] = seed_d2 ? -1 : 0;
    for (int m = lane; m < M; m += 64) {
        const double dm = sd[w][m];
        const int im = si[w][m];
        int rank = 0;
        for (int f = 0; f < M; ++f) rank += key_less(sd[w][f], si[w][f], dm, im) ? 1 : 0;
        if (rank < k) {
            idx_out[(int64_t)q * k + rank] = im;
            if (dist_out) dist_out[(int64_t)q * k + rank] = sq ? dm : sqrt(dm);  // (sq: squared, for the partitioned search's merge)
        }
        if (rank == k - 1) kth = dm;
    }
    // 4. certificate
    float tmin = tmerge;
    for (int c = lane; c < nchunks; c += 64) tmin = fminf(tmin, tau[(int64_t)q * nchunks + c]);
    for (int o = 32; o > 0; o >>= 1) {
        tmin = fminf(tmin, __shfl_xor(tmin, o));
        kth = fmax(kth, __shfl_xor(kth, o));
    }
    const double kth_full = kth;  // the row's k-th distance (squared) where it has k entries
    // a seeded row only has to be right up to the seed distance: entries beyond it are of no use to the caller
    kth = fmin(kth, seed);
    if (lane == 0) {
        certify(kth, kth_full, tmin, pe, qn2[q], M >= k, q, flagged, flag_bound, kth_out);  // tmin = +inf when nothing was ever rejected
    }
}

// ---------------------------------------------------------------------------------------------------
// The same for queries with ONE list of at most 32 candidates (the query blocks that swept the whole reference as a single
// range with KS = 32: two thirds to nine tenths of a search's queries): HALF a wave per query.  A query's candidates fill
// at most 32 lanes, so a whole wave spent most of the gather, both ranking loops and the certificate on idle lanes; with
// two queries per wave those parts cost half as much per query (the FP64 distance chain -- a quad of lanes per candidate
// row, 8 rows per half and trip -- costs the same).  Same arithmetic, same order, same outputs as knn_refine.
// Layout: query q's list is cand[q * stride .. + 32) (stride = nchunks * KS: the other ranges' columns of such a query hold
// nothing), its threshold tau[q * nchunks].
// ---------------------------------------------------------------------------------------------------
template <int REFINE_NC>
__global__ __launch_bounds__(256) void knn_refine_half(const double* __restrict__ X, const int32_t* __restrict__ ref_rows,
                                                       const double* __restrict__ Q, const int32_t* __restrict__ q_rows,
                                                       int nq, int d, int k, int nchunks, double eps_k, double eps_qr,
                                                       double eps_split, double eps_den, int scaled,
                                                       const int32_t* __restrict__ cand, const float* __restrict__ cand_v,
                                                       const float* __restrict__ tau, const double* __restrict__ qn2,
                                                       const unsigned long long* __restrict__ max_rn2_bits,
                                                       const float* __restrict__ seed_d2, int32_t* __restrict__ idx_out,
                                                       double* __restrict__ dist_out, int32_t* __restrict__ flagged,
                                                       double* __restrict__ flag_bound,
                                                       unsigned long long* __restrict__ zero_slots,
                                                       double* __restrict__ kth_out, int sq = 0,
                                                       const int32_t* __restrict__ img_pos = nullptr) {
    constexpr int KS = 32;
    __shared__ __attribute__((aligned(16))) double sd[8][KS];
    __shared__ int si[8][KS];
    const int lane = threadIdx.x & 63, hl = lane & 31, half = lane >> 5;
    const int w = (threadIdx.x >> 6) * 2 + half;  // the half-wave's row of the LDS arrays
    if (zero_slots && blockIdx.x == 0 && threadIdx.x < 64) {
        zero_slots[(size_t)threadIdx.x * 16] = 0ull;
        zero_slots[(size_t)threadIdx.x * 16 + 1] = 0ull;
    }
    const int qraw = blockIdx.x * 8 + w;
    const bool live = qraw < nq;
    const int q = live ? qraw : nq - 1;  // (an idle half follows the last query and writes nothing: shuffles stay convergent)
    const int64_t stride = (int64_t)nchunks * KS;
    const double* qv = Q + (int64_t)(q_rows ? q_rows[q] : q) * d;
    const PassError pe = pass_error(qn2[q], max_rn2_bits, scaled, eps_k, eps_qr, eps_split, eps_den);
    const double s = pe.s, eps = pe.eps;
    auto half_ballot = [&](bool p) { return (uint32_t)(__builtin_amdgcn_ballot_w64(p) >> (half << 5)); };
    // 1. dense list of the valid candidates
    unsigned long long* sk = reinterpret_cast<unsigned long long*>(&sd[w][0]);
    int M;
    {
        int id = cand[(int64_t)q * stride + hl];
        if (img_pos && id >= 0) id = img_pos[id];
        const uint32_t mask = half_ballot(id >= 0);
        const int pos = __builtin_popcount(mask & ((1u << hl) - 1u));
        if (id >= 0) {
            si[w][pos] = id;
            if (cand_v) sk[pos] = ((unsigned long long)f32_orderable(cand_v[(int64_t)q * stride + hl]) << 32) | (uint32_t)id;
        }
        M = __builtin_popcount(mask);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // 2. rank by approximate value; only the candidates within twice the error bound of the k-th best go on
    const int Mo = max(M, __shfl_xor(M, 32));  // (loops run to the longer of the wave's two lists)
    if (cand_v) {
        const bool rankit = M > k;
        int rank = 0x7FFFFFFF, id = 0;
        float vm = 0.f, vk = __builtin_inff();
        if (hl < M) {
            const unsigned long long km = sk[hl];
            vm = orderable_f32((uint32_t)(km >> 32));
            id = (int)(uint32_t)km;
            rank = 0;
        }
        for (int f = 0; f + 2 <= Mo; f += 2) {
            typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
            const u64x2 kf = *reinterpret_cast<const u64x2*>(sk + f);
            if (hl < M) {
                const unsigned long long km = ((unsigned long long)f32_orderable(vm) << 32) | (uint32_t)id;
                rank += (f < M && kf[0] < km ? 1 : 0) + (f + 1 < M && kf[1] < km ? 1 : 0);
            }
        }
        if ((Mo & 1) && hl < M && Mo - 1 < M) {
            const unsigned long long km = ((unsigned long long)f32_orderable(vm) << 32) | (uint32_t)id;
            rank += sk[Mo - 1] < km ? 1 : 0;
        }
        if (hl < M && rank == k - 1) vk = vm;
        for (int o = 16; o > 0; o >>= 1) vk = fminf(vk, __shfl_xor(vk, o));
        const float cut = (float)((double)vk + 2.0 * eps * (s * s) * 1.0000002 + 1e-30);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (rankit) {
            const bool keep = hl < M && vm <= cut;
            const uint32_t mask = half_ballot(keep);
            if (keep) si[w][__builtin_popcount(mask & ((1u << hl) - 1u))] = id;
            M = __builtin_popcount(mask);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    // 3. exact distances: a quad of lanes per candidate row, 8 rows per half and trip (see knn_refine)
    const int M3 = max(M, __shfl_xor(M, 32));
    if constexpr (REFINE_NC > 0) {
        const int g = hl >> 2, p = hl & 3;
        const int np = d >> 1;
        d2 x[REFINE_NC];
        quad_load<REFINE_NC>(x, reinterpret_cast<const d2*>(qv), p, np);
        const int p_last = (np - 1) & 3;
        for (int r0 = 0; r0 < M3; r0 += 8) {
            const int m = r0 + g;
            const int id = M > 0 ? si[w][m < M ? m : 0] : 0;  // (the other half's list may be the longer one: a valid row)
            const double acc = quad_chain_d2<REFINE_NC>(x, X + (int64_t)(ref_rows ? ref_rows[id] : id) * d, p, np);
            if (p == p_last && m < M) sd[w][m] = acc;
        }
    } else {
        if (hl < M) {
            const int id = si[w][hl];
            sd[w][hl] = exact_d2(qv, X + (int64_t)(ref_rows ? ref_rows[id] : id) * d, d);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const double seed = seed_d2 ? (double)seed_d2[q] : __builtin_inf();
    double kth = M >= k ? 0.0 : seed;
    if (live)
        for (int m = M + hl; m < k; m += 32) idx_out[(int64_t)q * k + m] = seed_d2 ? -1 : 0;
    {
        const double dm = hl < M ? sd[w][hl] : 0.0;
        const int im = hl < M ? si[w][hl] : 0;
        int rank = 0;
        for (int f = 0; f < M3; ++f) {
            if (f < M) rank += key_less(sd[w][f], si[w][f], dm, im) ? 1 : 0;
        }
        if (hl < M && rank < k && live) {
            idx_out[(int64_t)q * k + rank] = im;
            if (dist_out) dist_out[(int64_t)q * k + rank] = sq ? dm : sqrt(dm);  // (sq: squared, for the partitioned search's merge)
        }
        if (hl < M && rank == k - 1) kth = dm;
    }
    // 4. certificate
    for (int o = 16; o > 0; o >>= 1) kth = fmax(kth, __shfl_xor(kth, o));
    const double kth_full = kth;
    kth = fmin(kth, seed);
    if (hl == 0 && live) {
        certify(kth, kth_full, tau[(int64_t)q * nchunks], pe, qn2[q], M >= k, q, flagged, flag_bound, kth_out);
    }
}

}  // namespace

void refine_launch(hipStream_t stream, KnnWorkspace& ws, const PassPlan& plan, int KS, const PassEps& pe, const PassLists& L,
                   const double* X, const int32_t* ref_rows, const double* Qs, const int32_t* qrs, int nq, int d, int k,
                   const float* seed_d2, int32_t* io, double* dout, int32_t* flagged, double* flag_bound,
                   unsigned long long* zero_slots, double* kth_out) {
    // rows of an even number of doubles are 16-byte aligned: the quad gather, instantiated for the row length.  The queries
    // of the whole-range blocks (one list of <= 32 candidates each) take half a wave each, the others a wave
    const int need = (d & 1) ? 0 : cdiv(d, 8);
    const int nq_half = refine_half_queries(plan, KS, nq, dev_knobs());
    const int nchunks = plan.C;
    const int sq = ws.dist_squared ? 1 : 0;
    auto go = [&](auto nc) {
        constexpr int NC = decltype(nc)::value;
        if (nq_half > 0)
            hipLaunchKernelGGL(knn_refine_half<NC>, dim3(cdiv(nq_half, 8)), dim3(256), 0, stream, X, ref_rows, Qs, qrs, nq_half, d,
                               k, nchunks, pe.eps_k, pe.eps_qr, pe.eps_split, pe.eps_den, pe.scaled, L.cand, L.cand_v, L.tau, L.qn2,
                               L.maxbits, seed_d2, io, dout, flagged, flag_bound, zero_slots, kth_out, sq, L.img_pos);
        if (nq > nq_half)
            hipLaunchKernelGGL(knn_refine<NC>, dim3(cdiv(nq - nq_half, 4)), dim3(256), 0, stream, X, ref_rows, Qs, qrs, nq, d, k,
                               KS, nchunks, pe.eps_k, pe.eps_qr, pe.eps_split, pe.eps_den, pe.scaled, L.cand, L.cand_v, L.tau,
                               L.qn2, L.maxbits, seed_d2, io, dout, flagged, flag_bound, nq_half > 0 ? nullptr : zero_slots,
                               nq_half, kth_out, sq, L.img_pos);
    };
    if (need == 0 || need > 16) go(std::integral_constant<int, 0>{});
    else if (need <= 2) go(std::integral_constant<int, 2>{});
    else if (need <= 4) go(std::integral_constant<int, 4>{});
    else if (need <= 7) go(std::integral_constant<int, 7>{});
    else if (need <= 10) go(std::integral_constant<int, 10>{});
    else if (need <= 13) go(std::integral_constant<int, 13>{});
    else go(std::integral_constant<int, 16>{});
    BMX_LAUNCH_CHECK();
}

}  // namespace bmx
