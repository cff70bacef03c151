// mnnDeltaVariance() (R/mnnDeltaVariance.R:95-201) on the device: for every merge step the per-gene mean of the paired
// cells and the variance of their deltas, over genes x cells FP64 matrices in R's layout that are uploaded once and kept
// in HBM.  The hot path is a gather: every pair reads two whole gene vectors.
//   norms   cos.norm (:121-126): l2 of every cell over the norm genes, each batch's mean l2 by a fixed-order tree, ml2 the
//           mean of those; scale[c] = 1 / pmax(1e-8, l2[c] / ml2).
//   prep    one thread per pair: the two columns' addresses (a search of the batches' offset table) and scales.
//   pass 1  a workgroup owns DELTA_GENE_TILE genes (lanes along the genes, 16-byte loads where G is even) and one chunk
//           of DELTA_PAIR_CHUNK pairs of one step: the sums of s_l x_left and of s_r x_right in pair order.  Four pairs'
//           loads are in flight; a left cell that repeats stays in registers.  mean_reduce_kernel adds the chunk sums:
//           mean (:197) and the mean delta.
//   pass 2  the same walk: sum of (delta - mean delta)^2 (rowVars' two passes, :196); total_reduce_kernel adds the chunks
//           and divides by P - 1 (NaN below two pairs).
// The chunk edges are fixed positions of a step's pair list; the orders of the sums are those of ordered_sums.hpp.  All
// FP64 vector arithmetic, contraction off.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "bmx_ops.hpp"
#include "host_xfer.hpp"
#include "ordered_sums.hpp"
#include "resident_batches.hpp"

namespace bmx {
namespace {

constexpr int GT = DELTA_GENE_TILE;
constexpr int PC = DELTA_PAIR_CHUNK;
constexpr int TPB = GT / 2;  // threads of a pair-pass workgroup: two genes each

struct PairRef {
    const double* l;  // the left cell's column
    const double* r;
    double sl, sr;    // their scales (1 without cos.norm)
};
struct ChunkRef {
    int64_t begin;  // first pair, counted over the steps' concatenated lists
    int32_t len, step;
};

// bmean[b] = mean of l2 over batch b's cells: 256 strided sums, then a tree in a fixed order
__global__ __launch_bounds__(256) void l2_mean_kernel(const double* __restrict__ l2, const int64_t* __restrict__ off,
                                                      double* __restrict__ bmean) {
    __shared__ double sh[256];
    const int b = blockIdx.x;
    const int64_t c0 = off[b], n = off[b + 1] - c0;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += l2[c0 + i];
    const double sum = block_tree_sum<256>(s, sh);
    if (threadIdx.x == 0) bmean[b] = sum / (double)n;
}

// scale[c] = 1 / pmax(1e-8, l2[c] / ml2), ml2 = mean over the batches of bmean (:123-125, R/cosineNorm.R:80)
__global__ __launch_bounds__(256) void scale_kernel(const double* __restrict__ l2, int64_t N,
                                                    const double* __restrict__ bmean, int B, double* __restrict__ scale) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= N) return;
    double m = 0.0;
    for (int b = 0; b < B; ++b) m += bmean[b];
    m /= (double)B;
    scale[c] = 1.0 / cos_clamp(l2[c] / m);
}

// left / right: 1-based columns of the batches side by side; off [B + 1] the batches' first columns, base [B] their
// matrices.  The batch of a column is looked up here, once per pair.
__global__ __launch_bounds__(256) void pair_prep_kernel(const int32_t* __restrict__ left, const int32_t* __restrict__ right,
                                                        int64_t P, const int64_t* __restrict__ off, int B,
                                                        const double* const* __restrict__ base, int G,
                                                        const double* __restrict__ scale, PairRef* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    auto column = [&](int64_t c) {
        int lo = 0, hi = B - 1;  // the last batch that starts at or before c
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (off[mid] <= c) lo = mid; else hi = mid - 1;
        }
        return base[lo] + (c - off[lo]) * G;
    };
    const int64_t cl = (int64_t)left[p] - 1, cr = (int64_t)right[p] - 1;
    PairRef q;
    q.l = column(cl);
    q.r = column(cr);
    q.sl = scale ? scale[cl] : 1.0;
    q.sr = scale ? scale[cr] : 1.0;
    out[p] = q;
}

// this thread's two genes of a column: VEC 2 adjacent ones in one 16-byte load, VEC 1 the genes g0 and g1
template <int VEC>
__device__ __forceinline__ void load2(const double* __restrict__ col, int g0, int g1, double& a, double& b) {
    // (the column's address came out of memory: say that it is global memory, or the loads are flat ones)
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    typedef const __attribute__((address_space(1))) double* gptr;
    typedef const __attribute__((address_space(1))) f64x2* gptr2;
    if (VEC == 2) {
        const f64x2 v = *(gptr2)(col + g0);
        a = v.x;
        b = v.y;
    } else {
        a = *(gptr)(col + g0);
        b = *(gptr)(col + g1);
    }
}

// PASS 1: acc = {sum s_l x_left, sum s_r x_right} for both genes; PASS 2: acc = {sum (delta - mean delta)^2}
template <int PASS>
__device__ __forceinline__ void add_pair(const PairRef& q, double l0, double l1, double r0, double r1, double m0, double m1,
                                         double (&acc)[4]) {
    const double vl0 = q.sl * l0, vl1 = q.sl * l1, vr0 = q.sr * r0, vr1 = q.sr * r1;
    if (PASS == 1) {
        acc[0] += vl0;
        acc[1] += vl1;
        acc[2] += vr0;
        acc[3] += vr1;
    } else {
        const double d0 = (vl0 - vr0) - m0, d1 = (vl1 - vr1) - m1;
        acc[0] += d0 * d0;
        acc[1] += d1 * d1;
    }
}

// grid: chunks x gene tiles.  PASS 1: out_a[ch][g], out_b[ch][g] the chunk's two sums; PASS 2: out_a[ch][g] its sum of
// centred squares, mdelta [steps][G] the steps' mean deltas.  The pair records are read through uniform addresses.
template <int VEC, int PASS>
__global__ __launch_bounds__(TPB) void pair_pass_kernel(const PairRef* __restrict__ pairs, const ChunkRef* __restrict__ chunks,
                                                        int G, const double* __restrict__ mdelta,
                                                        double* __restrict__ out_a, double* __restrict__ out_b) {
    const int ch = blockIdx.x;
    const int t0 = blockIdx.y * GT;
    const int g0 = VEC == 2 ? t0 + 2 * (int)threadIdx.x : t0 + (int)threadIdx.x;
    if (g0 >= G) return;  // (VEC 2: G is even, so g0 + 1 is a gene too)
    const int g1 = VEC == 2 ? g0 + 1 : g0 + TPB;
    const bool has1 = g1 < G;
    const int g1c = has1 ? g1 : G - 1;  // a lane without a second gene reads the last one and drops it
    const ChunkRef c = chunks[ch];
    const PairRef* __restrict__ q = pairs + c.begin;
    double m0 = 0.0, m1 = 0.0;
    if (PASS == 2) {
        m0 = mdelta[(int64_t)c.step * G + g0];
        m1 = mdelta[(int64_t)c.step * G + g1c];
    }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const double* kept = nullptr;  // the column k0 / k1 hold
    double k0 = 0.0, k1 = 0.0;
    int i = 0;
    for (; i + 4 <= c.len; i += 4) {
        const PairRef p0 = q[i], p1 = q[i + 1], p2 = q[i + 2], p3 = q[i + 3];
        double r00, r01, r10, r11, r20, r21, r30, r31;
        // (each branch issues all its loads in one go: a load ahead of the branch would be waited for at the branch)
        if (p0.l == p1.l && p1.l == p2.l && p2.l == p3.l) {  // (uniform) one left cell: read once, or not at all
            if (p0.l != kept) {
                load2<VEC>(p0.l, g0, g1c, k0, k1);
                kept = p0.l;
            }
            load2<VEC>(p0.r, g0, g1c, r00, r01);
            load2<VEC>(p1.r, g0, g1c, r10, r11);
            load2<VEC>(p2.r, g0, g1c, r20, r21);
            load2<VEC>(p3.r, g0, g1c, r30, r31);
            add_pair<PASS>(p0, k0, k1, r00, r01, m0, m1, acc);
            add_pair<PASS>(p1, k0, k1, r10, r11, m0, m1, acc);
            add_pair<PASS>(p2, k0, k1, r20, r21, m0, m1, acc);
            add_pair<PASS>(p3, k0, k1, r30, r31, m0, m1, acc);
        } else {
            double l00, l01, l10, l11, l20, l21;
            load2<VEC>(p0.r, g0, g1c, r00, r01);
            load2<VEC>(p1.r, g0, g1c, r10, r11);
            load2<VEC>(p2.r, g0, g1c, r20, r21);
            load2<VEC>(p3.r, g0, g1c, r30, r31);
            load2<VEC>(p0.l, g0, g1c, l00, l01);
            load2<VEC>(p1.l, g0, g1c, l10, l11);
            load2<VEC>(p2.l, g0, g1c, l20, l21);
            load2<VEC>(p3.l, g0, g1c, k0, k1);
            kept = p3.l;
            add_pair<PASS>(p0, l00, l01, r00, r01, m0, m1, acc);
            add_pair<PASS>(p1, l10, l11, r10, r11, m0, m1, acc);
            add_pair<PASS>(p2, l20, l21, r20, r21, m0, m1, acc);
            add_pair<PASS>(p3, k0, k1, r30, r31, m0, m1, acc);
        }
    }
    for (; i < c.len; ++i) {
        const PairRef p = q[i];
        double r0, r1;
        load2<VEC>(p.r, g0, g1c, r0, r1);
        if (p.l != kept) {
            load2<VEC>(p.l, g0, g1c, k0, k1);
            kept = p.l;
        }
        add_pair<PASS>(p, k0, k1, r0, r1, m0, m1, acc);
    }
    const int64_t row = (int64_t)ch * G;
    if (PASS == 1) {
        out_a[row + g0] = acc[0];
        out_b[row + g0] = acc[2];
        if (has1) {
            out_a[row + g1] = acc[1];
            out_b[row + g1] = acc[3];
        }
    } else {
        out_a[row + g0] = acc[0];
        if (has1) out_a[row + g1] = acc[1];
    }
}

// step s, gene g: the chunk sums of the step in ascending order; mean = (mean left + mean right) / 2 (:197), mdelta = mean
// left - mean right.  chunk0 [steps + 1], npairs [steps].
__global__ __launch_bounds__(256) void mean_reduce_kernel(const double* __restrict__ part_l, const double* __restrict__ part_r,
                                                          int G, const int32_t* __restrict__ chunk0,
                                                          const int64_t* __restrict__ npairs, double* __restrict__ mean,
                                                          double* __restrict__ mdelta) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int s = blockIdx.y;
    if (g >= G) return;
    const double2 lr = fold_ascending<8>(make_double2(0.0, 0.0), chunk0[s], chunk0[s + 1], [&](int ch) {
        return make_double2(part_l[(int64_t)ch * G + g], part_r[(int64_t)ch * G + g]);
    });
    const double P = (double)npairs[s];
    const double ml = lr.x / P, mr = lr.y / P;  // (no pairs: NaN, as rowMeans of no columns)
    mean[(int64_t)s * G + g] = (ml + mr) / 2.0;
    mdelta[(int64_t)s * G + g] = ml - mr;
}

// total = (sum of the chunks' centred squares, ascending) / (P - 1); NaN below two pairs
__global__ __launch_bounds__(256) void total_reduce_kernel(const double* __restrict__ part, int G,
                                                           const int32_t* __restrict__ chunk0,
                                                           const int64_t* __restrict__ npairs, double* __restrict__ total) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int s = blockIdx.y;
    if (g >= G) return;
    const double v = fold_ascending<8>(0.0, chunk0[s], chunk0[s + 1], [&](int ch) { return part[(int64_t)ch * G + g]; });
    const int64_t P = npairs[s];
    total[(int64_t)s * G + g] = P >= 2 ? v / (double)(P - 1) : __longlong_as_double(0x7ff8000000000000ll);
}

}  // namespace

// what Delta::run takes
struct DeltaRun {
    int cos_norm = 0;
    const int32_t* norm_genes0 = nullptr;  // 0-based genes the cosine norms are taken over (null: all genes)
    int n_norm_genes = 0;
    int nsteps = 0;
    const int32_t* const* left = nullptr;   // per step: 1-based columns of the batches in upload order
    const int32_t* const* right = nullptr;
    const int64_t* npairs = nullptr;
    double* mean = nullptr;   // [G x nsteps] column-major
    double* total = nullptr;  // [G x nsteps] column-major
};

// argument checks of Delta::begin_batch / run without a device (throw Error): G genes, N cells uploaded so far
void delta_check_batch(int64_t n, int64_t cells_before) {
    check_cell_count(n);
    if (cells_before + n > 0x7fffffffll) throw Error(BMX_ERR_ARG, "the batches hold at most 2^31 - 1 cells together");
}

void delta_check_run(int G, int64_t N, const DeltaRun& a) {
    if (a.nsteps < 1) throw Error(BMX_ERR_ARG, "'pairs' must hold at least one merge step");
    if (!a.left || !a.right || !a.npairs) throw Error(BMX_ERR_ARG, "the pair lists are missing");
    if (!a.mean || !a.total) throw Error(BMX_ERR_ARG, "an output matrix is missing");
    if (a.n_norm_genes < 0 || (a.norm_genes0 && a.n_norm_genes < 1) || (!a.norm_genes0 && a.n_norm_genes > 0))
        throw Error(BMX_ERR_ARG, "invalid gene list for the cosine norms");
    for (int i = 0; i < a.n_norm_genes; ++i)
        if (a.norm_genes0[i] < 0 || a.norm_genes0[i] >= G) throw Error(BMX_ERR_SUBSET, "subset indices out of range");
    int64_t chunks = 0;
    for (int s = 0; s < a.nsteps; ++s) {
        const int64_t P = a.npairs[s];
        if (P < 0) throw Error(BMX_ERR_ARG, "a merge step has a negative number of pairs");
        if (P > 0 && (!a.left[s] || !a.right[s])) throw Error(BMX_ERR_ARG, "a merge step's pair list is missing");
        for (int64_t p = 0; p < P; ++p)
            if (a.left[s][p] < 1 || a.left[s][p] > N || a.right[s][p] < 1 || a.right[s][p] > N)
                throw Error(BMX_ERR_ARG, "'pairs' indices out of range");
        chunks += (P + PC - 1) / PC;
    }
    if (chunks > 0x7fffffffll) throw Error(BMX_ERR_ARG, "too many pairs");
}

struct DeltaBatch : ResidentBatch {};

// The batches stay resident; the per-gene mean and variance of the MNN-pair deltas of every merge step come out of one run.
class Delta : ResidentBatches<DeltaBatch> {
  public:
    Delta(int device, int G) : ResidentBatches(device, G, "bmx_delta_begin_batch") {}
    ~Delta() { retire(); }

    void begin_batch(int64_t n) {
        delta_check_batch(n, cells());
        check_begin(batches_.empty() ? nullptr : batches_.back().get());
        BMX_HIP(hipSetDevice(device_));
        const size_t elems = (size_t)n * G_;
        const size_t need = (elems + elems / 8 + 64) * sizeof(double);  // what DevBuf::reserve asks for
        size_t free_b = 0, total_b = 0;
        BMX_HIP(hipMemGetInfo(&free_b, &total_b));
        if (need > free_b) {  // parked blocks of earlier handles count as free memory
            DevBlockCache::release_global();
            BMX_HIP(hipMemGetInfo(&free_b, &total_b));
        }
        if (need > free_b) throw Error(BMX_ERR_HIP, no_room(need, free_b));
        try {
            begin(n, [](DeltaBatch&) {});
        } catch (const Error& e) {
            if (std::string(e.what()).find("hipMalloc failed") == std::string::npos) throw;
            throw Error(BMX_ERR_HIP, no_room(need, free_b));
        }
    }

    void add_block(const double* x_block, int64_t m) {
        const double t0 = now_ms();
        add(x_block, m, [&](DeltaBatch& b, double*) {
            if (b.complete()) BMX_HIP(hipStreamSynchronize(stream_));
        });
        ms_[0] += now_ms() - t0;
    }

    void run(const DeltaRun& a) {
        if (batches_.empty()) throw Error(BMX_ERR_ARG, "no batch has been added");
        for (auto& b : batches_)
            if (!b->complete()) throw Error(BMX_ERR_ARG, "a batch has not received all its cells");
        const int64_t N = cells();
        delta_check_run(G_, N, a);
        const double t0 = now_ms();
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        const int G = G_, B = (int)batches_.size(), S = a.nsteps;

        // the steps' lists side by side, cut into chunks at fixed positions of each list
        std::vector<int64_t> npairs(a.npairs, a.npairs + S), off((size_t)B + 1, 0);
        std::vector<int32_t> chunk0((size_t)S + 1, 0);
        std::vector<ChunkRef> chunks;
        int64_t Ptot = 0;
        for (int s = 0; s < S; ++s) {
            for (int64_t b = 0; b < npairs[(size_t)s]; b += PC)
                chunks.push_back({Ptot + b, (int32_t)std::min<int64_t>(PC, npairs[(size_t)s] - b), s});
            Ptot += npairs[(size_t)s];
            chunk0[(size_t)s + 1] = (int32_t)chunks.size();
        }
        const int nch = (int)chunks.size();
        std::vector<const double*> base((size_t)B);
        for (int b = 0; b < B; ++b) {
            base[(size_t)b] = batches_[(size_t)b]->x.p;
            off[(size_t)b + 1] = off[(size_t)b] + batches_[(size_t)b]->n;
        }

        int32_t* d_left = left_.reserve((size_t)std::max<int64_t>(Ptot, 1));
        int32_t* d_right = right_.reserve((size_t)std::max<int64_t>(Ptot, 1));
        PairRef* d_pairs = reinterpret_cast<PairRef*>(pairs_.reserve((size_t)std::max<int64_t>(Ptot, 1) * (sizeof(PairRef) / 8)));
        ChunkRef* d_chunks = reinterpret_cast<ChunkRef*>(chunks_.reserve((size_t)std::max(nch, 1) * (sizeof(ChunkRef) / 8)));
        int64_t* d_off = off_.reserve((size_t)B + 1 + (size_t)S);  // off [B + 1], npairs [S]
        int64_t* d_np = d_off + B + 1;
        int32_t* d_chunk0 = chunk0_.reserve((size_t)S + 1);
        const double** d_base = reinterpret_cast<const double**>(base_.reserve((size_t)B));
        double* part = part_.reserve((size_t)std::max(nch, 1) * G * 2);  // [2][chunks][G]
        double* part_r = part + (size_t)std::max(nch, 1) * G;
        double* stats = stats_.reserve((size_t)S * G * 3);  // mean [S][G], total [S][G], mean delta [S][G]
        double* d_mean = stats;
        double* d_total = stats + (size_t)S * G;
        double* d_mdelta = d_total + (size_t)S * G;

        int64_t at = 0;
        for (int s = 0; s < S; ++s) {
            const size_t bytes = (size_t)npairs[(size_t)s] * sizeof(int32_t);
            if (bytes) {
                upload_small(d_left + at, a.left[s], bytes);
                upload_small(d_right + at, a.right[s], bytes);
            }
            at += npairs[(size_t)s];
        }
        if (nch) upload_small(d_chunks, chunks.data(), (size_t)nch * sizeof(ChunkRef));
        upload_small(d_off, off.data(), ((size_t)B + 1) * sizeof(int64_t));
        upload_small(d_np, npairs.data(), (size_t)S * sizeof(int64_t));
        upload_small(d_chunk0, chunk0.data(), ((size_t)S + 1) * sizeof(int32_t));
        upload_small(d_base, base.data(), (size_t)B * sizeof(double*));
        const int32_t* d_genes = nullptr;
        if (a.cos_norm && a.norm_genes0) {
            int32_t* gp = genes_.reserve((size_t)a.n_norm_genes);
            upload_small(gp, a.norm_genes0, (size_t)a.n_norm_genes * sizeof(int32_t));
            d_genes = gp;
        }
        BMX_HIP(hipStreamSynchronize(stream_));  // (the host vectors may go; the caller's lists have been read)

        const double* d_scale = nullptr;
        if (a.cos_norm) {
            double* l2 = l2_.reserve((size_t)N * 2 + (size_t)B);  // l2 [N], scale [N], bmean [B]
            double* scale = l2 + N;
            double* bmean = scale + N;
            const int e0 = timer_.mark(stream_);
            for (int b = 0; b < B; ++b) {
                const DeltaBatch& bt = *batches_[(size_t)b];
                cell_l2_device(stream_, bt.x.p, G, bt.n, d_genes, a.n_norm_genes, false, l2 + off[(size_t)b]);
            }
            hipLaunchKernelGGL(l2_mean_kernel, dim3((unsigned)B), dim3(256), 0, stream_, (const double*)l2,
                               (const int64_t*)d_off, bmean);
            BMX_LAUNCH_CHECK();
            hipLaunchKernelGGL(scale_kernel, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, stream_, (const double*)l2, N,
                               (const double*)bmean, B, scale);
            BMX_LAUNCH_CHECK();
            timer_.span(1, e0, timer_.mark(stream_));
            d_scale = scale;
        }

        const dim3 rgrid((unsigned)cdiv(G, 256), (unsigned)S);
        const dim3 pgrid((unsigned)std::max(nch, 1), (unsigned)cdiv(G, GT));
        const bool vec2 = G % 2 == 0;
        const int e1 = timer_.mark(stream_);
        if (Ptot > 0) {
            hipLaunchKernelGGL(pair_prep_kernel, dim3((unsigned)cdiv(Ptot, 256)), dim3(256), 0, stream_,
                               (const int32_t*)d_left, (const int32_t*)d_right, Ptot, (const int64_t*)d_off, B,
                               (const double* const*)d_base, G, d_scale, d_pairs);
            BMX_LAUNCH_CHECK();
        }
        const int e2 = timer_.mark(stream_);
        timer_.span(3, e1, e2);
        if (nch > 0) {
            if (vec2)
                hipLaunchKernelGGL((pair_pass_kernel<2, 1>), pgrid, dim3(TPB), 0, stream_, (const PairRef*)d_pairs,
                                   (const ChunkRef*)d_chunks, G, (const double*)nullptr, part, part_r);
            else
                hipLaunchKernelGGL((pair_pass_kernel<1, 1>), pgrid, dim3(TPB), 0, stream_, (const PairRef*)d_pairs,
                                   (const ChunkRef*)d_chunks, G, (const double*)nullptr, part, part_r);
            BMX_LAUNCH_CHECK();
        }
        const int e3 = timer_.mark(stream_);
        timer_.span(2, e2, e3);
        hipLaunchKernelGGL(mean_reduce_kernel, rgrid, dim3(256), 0, stream_, (const double*)part, (const double*)part_r, G,
                           (const int32_t*)d_chunk0, (const int64_t*)d_np, d_mean, d_mdelta);
        BMX_LAUNCH_CHECK();
        const int e4 = timer_.mark(stream_);
        timer_.span(3, e3, e4);
        if (nch > 0) {
            if (vec2)
                hipLaunchKernelGGL((pair_pass_kernel<2, 2>), pgrid, dim3(TPB), 0, stream_, (const PairRef*)d_pairs,
                                   (const ChunkRef*)d_chunks, G, (const double*)d_mdelta, part, (double*)nullptr);
            else
                hipLaunchKernelGGL((pair_pass_kernel<1, 2>), pgrid, dim3(TPB), 0, stream_, (const PairRef*)d_pairs,
                                   (const ChunkRef*)d_chunks, G, (const double*)d_mdelta, part, (double*)nullptr);
            BMX_LAUNCH_CHECK();
        }
        const int e5 = timer_.mark(stream_);
        timer_.span(2, e4, e5);
        hipLaunchKernelGGL(total_reduce_kernel, rgrid, dim3(256), 0, stream_, (const double*)part, G,
                           (const int32_t*)d_chunk0, (const int64_t*)d_np, d_total);
        BMX_LAUNCH_CHECK();
        timer_.span(3, e5, timer_.mark(stream_));

        // the statistics of all steps in one download
        host_.resize((size_t)S * G * 2);
        BMX_HIP(hipMemcpyAsync(host_.data(), stats, host_.size() * sizeof(double), hipMemcpyDeviceToHost, stream_));
        BMX_HIP(hipStreamSynchronize(stream_));
        std::memcpy(a.mean, host_.data(), (size_t)S * G * sizeof(double));
        std::memcpy(a.total, host_.data() + (size_t)S * G, (size_t)S * G * sizeof(double));
        timer_.collect(ms_);
        ms_[4] += now_ms() - t0;
    }

    // milliseconds since the handle was made: upload (host wall time), HIP-event time of the cell norms, of the two pair
    // passes, of the pair preparation and the reductions over chunks, and the host wall time of the runs
    using ResidentBatches::stage_ms;

  private:
    int64_t cells() const {
        int64_t N = 0;
        for (auto& b : batches_) N += b->n;
        return N;
    }
    static std::string no_room(size_t need, size_t free_b) {
        return "the batches do not fit in free HBM (this batch needs " + std::to_string(need >> 20) + " MiB, " +
               std::to_string(free_b >> 20) + " MiB are free): use 'subset_row' to restrict the genes";
    }
    void upload_small(void* dev, const void* host, size_t bytes) {
        if (bytes >= ((size_t)1 << 20))
            upload_pageable(dev, host, bytes, stream_);
        else
            BMX_HIP(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, stream_));
    }

    DevBuf<int32_t> left_, right_, chunk0_, genes_;
    DevBuf<int64_t> off_;
    DevBuf<double> pairs_, chunks_, base_, part_, stats_, l2_;  // (pairs_, chunks_, base_: records of 8-byte words)
    std::vector<double> host_;
};

}  // namespace bmx

/* ---------------------------------------------------------------- bmx_delta_* ----------------------------------- */
struct bmx_delta final : bmx::Delta {
    using Delta::Delta;
};

extern "C" {

int32_t bmx_delta_create(int32_t device, int32_t G, bmx_delta_t** out) {
    return bmx::guarded([&] {
        if (!out) throw bmx::Error(BMX_ERR_ARG, "null output pointer");
        if (G < 1) throw bmx::Error(BMX_ERR_ARG, "mnnDeltaVariance needs at least one gene");
        *out = new bmx_delta(device, G);
    });
}

void bmx_delta_destroy(bmx_delta_t* h) { delete h; }

int32_t bmx_delta_begin_batch(bmx_delta_t* h, int64_t n) {
    return bmx::guarded([&] { bmx::live(h).begin_batch(n); });
}

int32_t bmx_delta_add_block(bmx_delta_t* h, const double* x_block, int64_t n_block) {
    return bmx::guarded([&] { bmx::live(h).add_block(x_block, n_block); });
}

int32_t bmx_delta_run(bmx_delta_t* h, int32_t cos_norm, const int32_t* norm_genes0, int32_t n_norm_genes, int32_t nsteps,
                      const int32_t* const* left, const int32_t* const* right, const int64_t* npairs, double* mean,
                      double* total) {
    return bmx::guarded([&] {
        bmx::DeltaRun a;
        a.cos_norm = cos_norm;
        a.norm_genes0 = norm_genes0;
        a.n_norm_genes = n_norm_genes;
        a.nsteps = nsteps;
        a.left = left;
        a.right = right;
        a.npairs = npairs;
        a.mean = mean;
        a.total = total;
        bmx::live(h).run(a);  // (delta_check_run comes before any device work)
    });
}

int32_t bmx_delta_stage_ms(const bmx_delta_t* h, double* out5) {
    return bmx::guarded([&] {
        if (!h || !out5) throw bmx::Error(BMX_ERR_ARG, "null argument");
        h->stage_ms(out5);
    });
}

}  // extern "C"
