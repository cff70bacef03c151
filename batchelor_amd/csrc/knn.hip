// Exact k-nearest-neighbour search on MI355X (gfx950) -- the >95 % hot spot of fastMNN / reducedMNN.
//
// Replaces the two BiocNeighbors::queryKNN calls inside findMutualNN (R/MNN_tree.R:129) and the one inside
// .tricube_weighted_correction (R/fastMNN.R:605).  Contract: exact Euclidean kNN, ascending distance; ties broken by
// lowest index (upstream leaves ties unpinned).
//
// A search goes through tiers; each tier only sees the queries the one before could not certify:
//   1. knn_topk_f16 (knn_f16.hip): single fp16 product per coordinate, K = d + 3 columns, KS = 32 (k <= 20) or 48
//      (k <= 36) candidates per query and reference range;
//   2. knn_topk_bf16 (knn_bf16.hip): three bf16 products per coordinate (f32-grade), KS = 24 / 40;
//   3. knn_exact_filter / knn_exact_pick: one FP64 sweep of the references against the handful of queries left, bounded
//      by each query's k-th candidate distance;
//   4. knn_exact_dist / knn_exact_select: full FP64 scan (massive exact ties, k > 36, tiny inputs, d > 127).
// After tiers 1 and 2, knn_refine computes the FP64 distances of the candidates in the reference's summation order
// (left to right over the dimensions, no FMA contraction), ranks them by (distance, index), and checks rigorously
// that no reference the candidate pass rejected can enter the top k given the pass's error bound; a query for which
// that cannot be shown is flagged for the next tier.
// Result: indices are exactly those of an FP64 brute-force search with (distance, index) ordering.
//
// This unit: which tiers take a shape (candidate_tiers), one candidate pass -- plan (knn_plan.hpp), reserve and prepare, launch,
// re-rank (knn_refine.hip) --, the tier cascade (search_tiers), knn_device.  The exact paths are in knn_exact.hip, the
// partitioned search for k > 36 in knn_large_k.hip; knn_internal.hpp declares what they call of one another.
#include "knn_internal.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <thread>

namespace bmx {
namespace {

using namespace sel;

std::atomic<int64_t> g_order_counts[2];  // candidate passes of the process with ordered references, without

// ---------------------------------------------------------------------------------------------------
// column sums over a row list (two deterministic stages)
// ---------------------------------------------------------------------------------------------------
// (row i of the sum is row i * stride of the list: a strided sample when stride > 1)
__global__ void colsum_partial(const double* __restrict__ X, const int32_t* __restrict__ rows, int n, int d,
                               int rows_per_block, int stride, double* __restrict__ partial) {
    __shared__ double sm[4][64];
    const int c0 = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int r0 = blockIdx.x * rows_per_block;
    const int r1 = min(n, r0 + rows_per_block);
    for (int cb = 0; cb < d; cb += 64) {
        const int c = cb + c0;
        double s = 0.0;
        if (c < d)
            for (int r = r0 + rl; r < r1; r += 4) {
                const int64_t rs = (int64_t)r * stride;
                const int64_t row = rows ? rows[rs] : rs;
                s += X[row * d + c];
            }
        sm[rl][c0] = s;
        __syncthreads();
        if (rl == 0 && c < d) partial[(int64_t)blockIdx.x * d + c] = (sm[0][c0] + sm[1][c0]) + (sm[2][c0] + sm[3][c0]);
        __syncthreads();
    }
}

__global__ void colsum_final(const double* __restrict__ partial, int nblocks, int d, double scale,
                             double* __restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= d) return;
    double s = 0.0;
    for (int b = 0; b < nblocks; ++b) s += partial[(int64_t)b * d + c];
    out[c] = s * scale;
}

// seeded search: tau_g = min(what is there, the seed's threshold) -- the form for passes that do not take the fused prep
__global__ void seed_tau_kernel(const float* __restrict__ seed_d2, const double* __restrict__ qn2,
                                const unsigned long long* __restrict__ max_rn2_bits, int nq, int nq_pad, PassEps pe,
                                uint32_t* __restrict__ tau_g) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq_pad) return;
    uint32_t o = f32_orderable(-__builtin_inff());  // padded queries: nothing passes
    if (q < nq) o = pass_seed_tau((double)seed_d2[q], qn2[q], __longlong_as_double((long long)*max_rn2_bits), pe);
    tau_g[q] = q < nq ? min(tau_g[q], o) : o;  // the image is order-preserving: min of images = image of the min
}

__global__ void fill_f64(double* __restrict__ p, int n, double v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

__global__ void fill_u32(uint32_t* __restrict__ p, int n, uint32_t v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}


// rows of the flagged queries in the caller's query list: out[f] = rows ? rows[flagged[1 + f]] : flagged[1 + f]
__global__ void flagged_rows(const int32_t* __restrict__ flagged, int n, const int32_t* __restrict__ rows,
                             int32_t* __restrict__ out) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < n) {
        const int q = flagged[1 + f];
        out[f] = rows ? rows[q] : q;
    }
}

// results of a search over the flagged queries back into their rows: out[flagged[1 + f]][j] = sub[f][j]
__global__ void scatter_flagged(const int32_t* __restrict__ flagged, int n, int k, const int32_t* __restrict__ sub_idx,
                                const double* __restrict__ sub_dist, int32_t* __restrict__ idx_out,
                                double* __restrict__ dist_out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * k) return;
    const int f = e / k, j = e - f * k;
    const int64_t o = (int64_t)flagged[1 + f] * k + j;
    idx_out[o] = sub_idx[e];
    if (dist_out) dist_out[o] = sub_dist[e];
}

// Developer experiment (testing hook "tau_replay", EXPERIMENTS.md round 6): what the full pass would cost if every query
// STARTED from the threshold it ends with.  1: every search of a run records its queries' final thresholds (the smallest over
// its reference ranges: each is at least the k-th best value of ITS range plus the margin, hence of the whole reference);
// 2: the same sequence of searches starts its full passes from the recording.  Any valid threshold leaves the results as they
// are; only the number of survivors changes.
__global__ void tau_record_kernel(const float* __restrict__ tau, int nchunks, int nq, uint32_t* __restrict__ rec) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    float t = __builtin_inff();
    for (int c = 0; c < nchunks; ++c) t = fminf(t, tau[(int64_t)q * nchunks + c]);
    rec[q] = f32_orderable(t);
}
__global__ void tau_apply_kernel(const uint32_t* __restrict__ rec, int nq, uint32_t* __restrict__ tau_g) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nq) tau_g[q] = min(tau_g[q], rec[q]);
}

// out[d] = the mean of a strided sample of at most 16k of the rows (X, rows)[0, n)
void strided_mean(hipStream_t stream, KnnWorkspace& ws, const double* X, const int32_t* rows, int n, int d, double* out) {
    const int cstride = std::max(1, n / 16384);
    const int ncs = cdiv(n, cstride);
    const int rpb = 256;
    const int nb = cdiv(ncs, rpb);
    double* red = ws.red.reserve((size_t)nb * d);
    hipLaunchKernelGGL(colsum_partial, dim3(nb), dim3(256), 0, stream, X, rows, ncs, d, rpb, cstride, red);
    BMX_LAUNCH_CHECK();
    hipLaunchKernelGGL(colsum_final, dim3(cdiv(d, 64)), dim3(64), 0, stream, red, nb, d, 1.0 / ncs, out);
    BMX_LAUNCH_CHECK();
}

// the error constants of a tier's pass (knn_select.hpp: pass_eps)
PassEps tier_pass_eps(const Tier& T, int d) {
    PassEps pe;
    if (T.id == 1) {
        pe.eps_k = 16.0 * T.NS;                                            // f32 accumulation over the K columns
        pe.eps_qr = 2.0;                                                   // one product block, <= 2 |q||r|
        pe.eps_split = 2.0 * (0.0009765625 + 2.384185791015625e-07);       // both operands rounded to fp16: 2^-10 (1 + 2^-12) * 2|q||r|
        pe.eps_den = 6.103515625e-05 * (std::sqrt((double)d) + 3.0);       // 2^-14 per flushed input, scaled units
        pe.scaled = 1;
    } else {
        pe.eps_k = 16.0 * T.NS;                                            // f32 accumulation over the concatenated K
        pe.eps_qr = 6.0;                                                   // three product blocks, each <= 2 |q||r|
        pe.eps_split = 1.5 * 3.03 * 2.0 * 1.52587890625e-05;               // dropped ql.rl, qh.r3, q3.rh: 3.03 * 2^-16 * 2|q||r|
        pe.eps_den = 0.0;
        pe.scaled = 0;                                                     // (where that holds: pass_window, knn_select.hpp)
    }
    return pe;
}

}  // namespace

void knn_order_counts(int64_t out[2]) {
    out[0] = g_order_counts[0].load();
    out[1] = g_order_counts[1].load();
}

int candidate_tiers(int d, int k, int nr, Tier out[2]) {
    const int only = dev_knobs().knn_tier;  // testing hook: 1 / 2 = that tier only, 3 = exact scan only
    int n = 0;
    if (k > 36) return 0;
    const int KS1 = k <= 20 ? BMX_KS1 : 48, KS2 = k <= 20 ? 24 : 40;
    const int ns1 = f16_pick_ns(d, KS1);
    if (ns1 && nr > 2 * KS1 && (only == 0 || only == 1)) out[n++] = Tier{1, ns1, KS1};
    const int ns2 = bf16_pick_ns(d);
    if (ns2 && !(KS2 == 40 && ns2 > 16) && nr > 2 * KS2 && (only == 0 || only == 2)) out[n++] = Tier{2, ns2, KS2};
    return n;
}

namespace {

// One candidate pass + refine over the queries (Qs, qrs)[0, nq): certified rows of io / dout are final; the others
// are listed in `flagged` (count in flagged[0]) with their k-th candidate distance in flag_bound.
void candidate_pass(hipStream_t stream, KnnWorkspace& ws, const Tier& T, const double* X, const int32_t* ref_rows, int nr,
                    const double* Qs, const int32_t* qrs, int nq, int d, int k, int32_t* io, double* dout,
                    int32_t* flagged, double* flag_bound, const float* seed_d2, const double* centre, double* kth_out,
                    const double* qcentre) {
    const int NS = T.NS, KS = T.KS;
    ws.last_variant = T.id == 1 ? 3 : 2;
    // 1. the plan.  Queries per workgroup: 8 consumer waves of 32 in the fp16 kernel; 8 or 4 (long rows, long lists) in the
    // bf16 kernel.  (The fp16 ring hands two or four tiles over at a time; a bf16 range is a multiple of 32 rows.)
    const int unit = T.id == 1 ? 256 : 32 * bf16_ncons(NS, KS), rows_per_slot = T.id == 1 ? f16_rows_per_slot(NS, KS) : 32;
    PassPlan plan = plan_candidate_pass(T.id, NS, KS, unit, rows_per_slot, nq, nr, seed_d2 != nullptr, dev_knobs());
    // Ordered references (knn_order.hpp; testing hook "ref_order": 0 never, 1 wherever it is possible): the fp16 tier, with a
    // centre of the queries, where the search has a threshold sample -- the sample is what the order serves first
    const int ord_knob = dev_knobs().ref_order;
    // (the one statement of the rule.  Without a centre from the caller, knn_device allows the mean of a strided sample of at
    // most 16k of the queries, as for the references' centre: two small launches, made only where the order is used)
    const bool ordered = T.id == 1 && (qcentre || ws.qcentre_auto) && ord_knob != 0 && (ord_knob == 1 || plan.S > 0);
    if (ordered && !qcentre) {
        double* qc = ws.qcentre.reserve(d);
        strided_mean(stream, ws, Qs, qrs, nq, d, qc);
        qcentre = qc;
    }
    if (ordered) plan = plan_candidate_pass(T.id, NS, KS, unit, rows_per_slot, nq, nr, seed_d2 != nullptr, dev_knobs(), true);
    ++g_order_counts[ordered ? 0 : 1];
    const int nq_pad = plan.nq_pad, nqb = plan.nqb, S = plan.S, C = plan.C, chunk_len = plan.chunk_len, nr_pad = plan.nr_pad;
    const int nchunks = C;
    if (debug_prints())
        fprintf(stderr, "[bmx] knn tier %d: nq=%d nr=%d d=%d NS=%d KS=%d S=%d C=%d chunk=%d full-range blocks=%d of %d\n", T.id,
                nq, nr, d, NS, KS, S, C, chunk_len, C > 1 ? plan.n_full : nqb, nqb);

    // 2. reserve and prepare
    const int KPw = 8 * NS;  // prepared row width in 4-byte words
    float* pq = ws.pq.reserve((size_t)nq_pad * KPw);
    float* pr = ws.pr.reserve((size_t)(nr_pad + 256) * KPw);  // + tail padding: the producers' prefetches over-read
    double* qn2 = ws.qn2.reserve(nq_pad);
    double* rn2 = ws.rn2.reserve(nr_pad);
    double* mean = ws.mean.reserve((size_t)d + 2);
    unsigned long long* maxbits = reinterpret_cast<unsigned long long*>(mean + d);
    int32_t* cand = ws.cand.reserve((size_t)nq_pad * nchunks * KS);
    float* cand_v = ws.cand_v.reserve((size_t)nq_pad * nchunks * KS);
    float* tau = ws.tau.reserve((size_t)nq_pad * nchunks);
    uint32_t* tau_g = ws.tau_g.reserve(nq_pad);
    unsigned long long* slots = ws.maxslots.reserve(64 * 16);

    // centre of the reference: any vector is valid (the error bound uses the norms actually obtained), a point
    // near the mean keeps it tight -- the mean of a strided sample of <= 16k rows costs next to nothing
    // (the merge engine already holds the column mean of the reference's node and hands it in: nothing to compute)
    if (!centre) {
        strided_mean(stream, ws, X, ref_rows, nr, d, mean);
        centre = mean;
    }
    const PassEps pe = tier_pass_eps(T, d);
    // 3. launch: the sample pass over rows [0, S), the full pass, the re-rank
    PassLaunch L{reinterpret_cast<const uint16_t*>(pq), reinterpret_cast<const uint16_t*>(pr), nqb, 0, plan.sample_range_len,
                 plan.sample_nranges, S, 0, nchunks, tau_g, 1, cand, cand_v, tau};
    const bool no_margin = dev_knobs().no_margin != 0;  // testing hook: the KS-th-best cut only
    auto go = [&](const PassLaunch& l) {
        return T.id == 1 ? f16_launch(stream, ws, NS, KS, l) : bf16_launch(stream, ws, NS, KS, l);
    };
    bool ok = true;
    unsigned long long* zero_slots = nullptr;
    const int32_t* img_pos = nullptr;  // ordered references: the pass lists image rows, the re-rank turns them into positions
    if (T.id == 1) {
        // fp16 tier: references (norms, then image) and queries (image, norm, margin, seed threshold) in TWO launches; the
        // slot maxima are folded by the second one, which also resets the flagged-query counter (knn_f16.hip)
        if (!ws.slots_clean) BMX_HIP(hipMemsetAsync(slots, 0, 64 * 16 * sizeof(unsigned long long), stream));
        float* margin = no_margin ? nullptr : ws.margin.reserve(nq_pad);
        uint32_t* tau_seed = seed_d2 ? ws.tau_seed.reserve(nq_pad) : nullptr;
        // without a sample pass the thresholds start at the seed (or at +inf): prep writes them
        L.shape = f16_pick_shape(NS, KS);  // (the reference image is laid out for the MFMA shape of the sweep)
        RefOrder ord{};
        if (ordered)
            ord = RefOrder{qcentre, ws.ord_key.reserve(nr), ws.ord_scratch.reserve(ref_order_scratch_words(nr)),
                           ws.img_src.reserve(nr), ws.img_pos.reserve(nr)};
        img_pos = ord.img_pos;
        f16_prep_all(stream, X, ref_rows, nr, nr_pad, Qs, qrs, nq, nq_pad, d, NS, L.shape, centre, reinterpret_cast<uint16_t*>(pr),
                     reinterpret_cast<uint16_t*>(pq), rn2, qn2, maxbits, slots, flagged, margin, pe, seed_d2, tau_seed,
                     S == 0 || plan.CS > 1 ? tau_g : nullptr, ordered ? &ord : nullptr);
        if (margin) {
            L.margin = margin;
            L.k = k;
        }
        L.tau_seed = tau_seed;
        zero_slots = slots;  // knn_refine leaves them zeroed for the next search
        ws.slots_clean = false;
        if (S > 0) {
            float* lists = nullptr;
            if (L.nranges > 1 && margin) {  // a split sample: its ranges leave their lists for f16_sample_merge
                lists = ws.samp_lists.reserve((size_t)nq_pad * L.nranges * KS);
                L.cand_v = lists;  // (a sample pass has no other use for it)
            }
            ok = go(L);
            if (lists) f16_sample_merge(stream, lists, L.nranges, KS, nq, k, margin, tau_g);
            L.cand_v = cand_v;
        }
    } else {
        ws.slots_clean = false;
        BMX_HIP(hipMemsetAsync(maxbits, 0, sizeof(unsigned long long), stream));
        bf16_prep(stream, X, ref_rows, nr, nr_pad, d, NS, centre, 0, reinterpret_cast<uint16_t*>(pr), rn2, maxbits, slots);
        bf16_prep(stream, Qs, qrs, nq, nq_pad, d, NS, centre, 1, reinterpret_cast<uint16_t*>(pq), qn2, maxbits, slots);
        // sample pass: threshold estimation over rows [0, S); full pass: every row, starting from that threshold
        if (S == 0) {  // no sample: +inf everywhere (0xFF800000 is the orderable image of +inf)
            hipLaunchKernelGGL(fill_u32, dim3(cdiv(nq_pad, 256)), dim3(256), 0, stream, tau_g, nq_pad, 0xFF800000u);
            BMX_LAUNCH_CHECK();
        }
        if (S > 0) ok = go(L);
        if (seed_d2) {  // tau_g = min(sampled threshold, seed threshold)
            hipLaunchKernelGGL(seed_tau_kernel, dim3(cdiv(nq_pad, 256)), dim3(256), 0, stream, seed_d2, qn2, maxbits, nq, nq_pad,
                               pe, tau_g);
            BMX_LAUNCH_CHECK();
        }
        BMX_HIP(hipMemsetAsync(flagged, 0, sizeof(int32_t), stream));
    }
    L.first_begin = 0;
    L.range_len = chunk_len;
    L.nranges = C;
    L.n_full = C > 1 ? plan.n_full : 0;
    L.r_limit = nr_pad;
    L.sample = 0;
    const int replay = T.id == 1 ? dev_knobs().tau_replay : 0;
    if (replay == 2 && ws.replay_idx < ws.tau_rec.size() && ws.tau_rec[ws.replay_idx].cap >= (size_t)nq_pad) {
        hipLaunchKernelGGL(tau_apply_kernel, dim3(cdiv(nq_pad, 256)), dim3(256), 0, stream,
                           (const uint32_t*)ws.tau_rec[ws.replay_idx].p, nq_pad, tau_g);
        BMX_LAUNCH_CHECK();
    }
    ok = ok && go(L);
    if (replay == 1) {
        if (ws.tau_rec.size() <= ws.replay_idx) ws.tau_rec.resize(ws.replay_idx + 1);
        hipLaunchKernelGGL(tau_record_kernel, dim3(cdiv(nq_pad, 256)), dim3(256), 0, stream, (const float*)tau, nchunks, nq_pad,
                           ws.tau_rec[ws.replay_idx].reserve((size_t)nq_pad));
        BMX_LAUNCH_CHECK();
    }
    if (replay) ++ws.replay_idx;
    if (!ok) throw Error(BMX_ERR_ARG, "kNN: unsupported padded dimension");
    refine_launch(stream, ws, plan, KS, pe, PassLists{cand, cand_v, tau, qn2, maxbits, img_pos}, X, ref_rows, Qs, qrs, nq, d, k, seed_d2,
                  io, dout, flagged, flag_bound, zero_slots, kth_out);
    if (zero_slots) ws.slots_clean = true;
    if (debug_prints()) {
        std::vector<int32_t> hc((size_t)nq * nchunks * KS);
        BMX_HIP(hipMemcpyAsync(hc.data(), cand, hc.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        ws.sync(stream);
        size_t valid = 0;
        for (int32_t v : hc) valid += v >= 0;
        fprintf(stderr, "[bmx] candidates per query after the top-k pass: %.1f (of %d slots)\n", (double)valid / nq,
                nchunks * KS);
    }
}

// one device word to the host: stored into pinned memory by a one-thread kernel, sequence number last, and the host spins
// on that word (no copy to schedule, signal and poll through the runtime: ~15 us instead of ~100 of idle GPU per read-back)
__global__ void publish_word(const int32_t* __restrict__ dev, int32_t* host, int seq) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int32_t v = *dev;
    __hip_atomic_store(&host[0], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&host[1], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace

int read_count(hipStream_t stream, KnnWorkspace& ws, const int32_t* dev) {
    int32_t* h = reinterpret_cast<int32_t*>(ws.pinned_words());  // word 0 of the workspace's pinned block: [value, sequence]
    if (ws.read_seq == 0) h[1] = 0;  // (a pooled block may hold an earlier owner's numbers)
    const int seq = ++ws.read_seq;
    hipLaunchKernelGGL(publish_word, dim3(1), dim3(64), 0, stream, dev, h, seq);
    BMX_LAUNCH_CHECK();
    const double budget = ws.wd_budget_s;
    const auto t0 = std::chrono::steady_clock::now();
    volatile int32_t* vp = h;
    unsigned spins = 0;
    while (vp[1] != seq) {
        if ((++spins & 0x3FFu) == 0) {
            const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (budget > 0.0 && el > budget)
                throw WatchdogTimeout("watchdog: the GPU work queued on the engine's stream did not finish in time; the engine is "
                                      "dead (restart the process)");
            if (el > 0.5) {
                const hipError_t e = hipStreamQuery(stream);
                (void)hipGetLastError();
                if (e != hipSuccess && e != hipErrorNotReady)
                    throw Error(BMX_ERR_HIP, std::string("the search's stream failed: ") + hipGetErrorString(e));
                std::this_thread::sleep_for(std::chrono::microseconds(200));
            }
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return h[0];
}

void search_tiers(hipStream_t stream, KnnWorkspace& ws, const Tier* tiers, int ntiers, int t, const double* X,
                  const int32_t* ref_rows, int nr, const double* Qs, const int32_t* qrs, int nq, int d, int k, int32_t* io,
                  double* dout, const float* seed_d2, const double* centre, double* kth_out, const double* qcentre) {
    if (t >= ntiers) {
        exact_search(stream, ws, X, ref_rows, nr, Qs, qrs, d, k, io, dout, nullptr, nullptr, nq);
        return;
    }
    int32_t* flagged = ws.flagged_t[t].reserve((size_t)nq + 1);
    double* bound = ws.flag_bound_t[t].reserve((size_t)nq + 1);
    // (what a seeded pass cannot settle goes on unseeded: the full k nearest serve the caller just as well)
    // (kth_out: the first tier's re-rank writes it for the rows it certifies; a row any later tier or the exact sweep rewrites
    // keeps +inf there, which only costs the intersection's probe a row read)
    candidate_pass(stream, ws, tiers[t], X, ref_rows, nr, Qs, qrs, nq, d, k, io, dout, flagged, bound, seed_d2, centre,
                   t == 0 ? kth_out : nullptr, qcentre);
    if (ws.optimistic && t == 0) {
        // Optimistic run (the merge engine): no read-back inside a search.  Practically every query is certified by the
        // first tier (config 3: 1-6 of 3 million per step are not), so the bounded FP64 sweep for the few that are not is
        // launched unconditionally with the count left on the device -- with nothing flagged its workgroups end at once.
        // More than OPT_CAP flagged queries, or a list that overflows (massive exact ties), raises opt_state[0]; the engine
        // looks at it at its next wait and repeats the run with host-checked searches.
        launch_bounded_sweep(stream, ws, X, ref_rows, nr, Qs, qrs, d, k, io, dout, flagged, bound, 0, KnnWorkspace::OPT_CAP,
                             seed_d2 != nullptr, ws.opt_state_ptr(stream));
        return;
    }
    // the number of uncertified queries decides what is launched next, so it is read back (one small synchronisation)
    const int count = read_count(stream, ws, flagged);
    if (count == 0) return;
    ws.last_flagged_tier[t] += count;
    // a few hundred leftovers are cheaper in one bounded FP64 sweep than in another candidate pass (prep of the whole
    // reference + a launch that cannot fill the chip)
    if (t + 1 < ntiers && count >= 256) {
        // the next candidate tier sees only these queries: a row list into the caller's query matrix, results into a
        // scratch block that is scattered back afterwards
        int32_t* rows2 = ws.sub_rows[t].reserve((size_t)count);
        hipLaunchKernelGGL(flagged_rows, dim3(cdiv(count, 256)), dim3(256), 0, stream, flagged, count, qrs, rows2);
        BMX_LAUNCH_CHECK();
        int32_t* sub_idx = ws.sub_idx[t].reserve((size_t)count * k);
        double* sub_dist = dout ? ws.sub_dist[t].reserve((size_t)count * k) : nullptr;
        search_tiers(stream, ws, tiers, ntiers, t + 1, X, ref_rows, nr, Qs, rows2, count, d, k, sub_idx, sub_dist, nullptr, centre);
        hipLaunchKernelGGL(scatter_flagged, dim3(cdiv((int64_t)count * k, 256)), dim3(256), 0, stream, flagged, count, k,
                           sub_idx, sub_dist, io, dout);
        BMX_LAUNCH_CHECK();
    } else {
        exact_search(stream, ws, X, ref_rows, nr, Qs, qrs, d, k, io, dout, flagged, bound, count, seed_d2 != nullptr);
    }
}

void knn_device(hipStream_t stream, KnnWorkspace& ws, const double* X, const int32_t* ref_rows, int nr,
                const double* Q, const int32_t* q_rows, int d, int k, int32_t* idx_out, double* dist_out, int q_begin, int q_end, const float* seed_d2, const double* centre, double* kth_out,
                const double* qcentre) {
    const int nq = q_end - q_begin;
    if (nq <= 0 || k <= 0) return;
    if (k > nr) throw Error(BMX_ERR_ARG, "kNN: k exceeds the number of reference cells");
    // sub-range of the query list
    const double* Qs = Q;
    const int32_t* qrs = q_rows;
    if (q_rows)
        qrs = q_rows + q_begin;
    else
        Qs = Q + (int64_t)q_begin * d;
    int32_t* io = idx_out + (int64_t)q_begin * k;
    double* dout = dist_out ? dist_out + (int64_t)q_begin * k : nullptr;

    Tier tiers[2];
    const int ntiers = ws.force_exact ? 0 : candidate_tiers(d, k, nr, tiers);
    ws.last_exact = 0;
    ws.last_flagged_tier[0] = ws.last_flagged_tier[1] = 0;
    if (kth_out && ntiers == 0) {  // no candidate tier takes the shape: every row read by the probe
        hipLaunchKernelGGL(fill_f64, dim3(cdiv(nq, 256)), dim3(256), 0, stream, kth_out + q_begin, nq, __builtin_inf());
        BMX_LAUNCH_CHECK();
    }
    // (k beyond the tiers' lists: P partitions of the reference at k = 36 each, merged exactly; a seeded search goes unseeded --
    // the full k nearest serve its caller just as well)
    // (also k in (20, 36] where no tier holds lists that long: rows of more than 61 columns, BASELINE config 5's 100 PCs)
    if (ntiers == 0 && !ws.force_exact && k > 20 && dev_knobs().knn_tier != 3 &&
        large_k_search(stream, ws, X, ref_rows, nr, Qs, qrs, nq, d, k, io, dout, centre, kth_out ? kth_out + q_begin : nullptr)) {
        ws.exact_total += ws.last_exact;
        return;
    }
    // (a caller without a centre of the queries: the fp16 pass that wants the order takes the strided-sample mean of its
    // queries itself -- candidate_pass has the one statement of the rule; the partitions of the large-k search above do not)
    struct AutoCentre {
        KnnWorkspace& w;
        explicit AutoCentre(KnnWorkspace& ws_) : w(ws_) { w.qcentre_auto = true; }
        ~AutoCentre() { w.qcentre_auto = false; }
    } auto_centre(ws);
    search_tiers(stream, ws, tiers, ntiers, 0, X, ref_rows, nr, Qs, qrs, nq, d, k, io, dout,
                 seed_d2 ? seed_d2 + q_begin : nullptr, centre, kth_out ? kth_out + q_begin : nullptr, qcentre);
    if (ntiers > 0) ws.exact_total += ws.last_exact;
    if (ntiers > 0) ws.tier2_total += ws.last_flagged_tier[0] * (ntiers > 1 ? 1 : 0);
}

}  // namespace bmx
