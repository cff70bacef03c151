// Per-batch, per-gene mean and variance (what scran::modelGeneVar takes from its input before any trend) on the device:
// genes x cells FP64 values in R's layout, dense (GeneVar, bmx_genevar_*) or canonical CSC (GeneVarSparse,
// bmx_genevar_sparse_*).  A batch streams through TWO block buffers: a block is reduced into a running per-gene state
// behind the copy of the next block, so neither the matrix nor one partial per chunk stays in HBM.
//   per block, on the kernel stream, once the block has landed:
//     gv_dense_kernel      lanes along the genes (16-byte loads, two genes a lane, where G is even), the block's cells cut
//                          into chunks of NCH at fixed positions within the batch.  Per chunk and gene, two sweeps over the
//                          chunk while it sits in the block buffer: the sum gives the chunk mean, then the sum of
//                          (x - chunk mean)^2, both in the cell order of ordered_sums.hpp.  Also the flag for a value
//                          that is not finite.
//     gv_csc_check_kernel  one wave a cell over its stored entries: the flags for a value that is not finite, a row
//                          outside [0, G) and rows that do not ascend strictly within a column
//     gv_csc_kernel        one workgroup per (chunk, tile of GT genes), sum / count / squares of the tile in the LDS:
//                          the chunk's columns in ascending order (csc_tile_walk: every column's tile range by binary
//                          search, a barrier between columns), twice.  The stored entries contribute (v - m)^2, the
//                          (cells - stored) implicit zeros of the chunk (cells - stored) * m * m.
//     gv_merge_kernel      one thread a gene: the block's chunks, ascending, folded into the gene's running
//                          (mean, M2) by genevar_merge (gene_var_host.hpp); the count is the same for every gene
//   per batch: gv_final_kernel, total = M2 / (n - 1)
// Never the one-pass E[x^2] - E[x]^2.  Contraction off; the chunk edges do not depend on the blocks (a block holds whole
// chunks), and the sums keep the orders of ordered_sums.hpp, so every block width and every run give the same bits.
// A block's entry positions come from an indptr the host has checked (check_csc_block); a row index is compared with its
// bounds before it addresses anything, and an entry that fails is skipped.
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "bmx_ops.hpp"
#include "csc_device.hpp"
#include "gene_var_host.hpp"
#include "host_xfer.hpp"
#include "ordered_sums.hpp"
#include "resident_batches.hpp"

namespace bmx {
namespace {

constexpr int NCH = GENEVAR_CHUNK;
constexpr int GT = GENEVAR_GENE_TILE;  // genes per tile of the CSC kernel: 2 x 16 KiB of doubles + 8 KiB of counts in the LDS
constexpr double DBL_LARGEST = 1.7976931348623157e308;
// flags (device): a value that is not finite, then the pattern pair (CSC_F_ROW, CSC_F_ORDER)
enum { F_VALUE = 0, F_PATTERN = 1, F_WORDS = F_PATTERN + CSC_F_WORDS };

__device__ __forceinline__ int not_finite(double v) { return !(fabs(v) <= DBL_LARGEST); }

// The chunks of a block of m cells at x ([m][G]): chunk blockIdx.x holds the cells [ch * NCH, min(m, (ch + 1) * NCH)).
// pmean / pm2 [chunks][G]: the chunk's mean and its sum of squared deviations from that mean, both sums in cell order.
// V2: two genes a thread, 16-byte loads (G even).
template <bool V2>
__global__ __launch_bounds__(256) void gv_dense_kernel(const double* __restrict__ x, int G, int64_t m,
                                                       double* __restrict__ pmean, double* __restrict__ pm2,
                                                       int32_t* __restrict__ flags) {
    const int t = blockIdx.y * 256 + threadIdx.x;
    if (t >= (V2 ? G / 2 : G)) return;
    const int64_t ch = blockIdx.x;
    const int64_t b = ch * NCH;
    const int64_t e = b + NCH < m ? b + NCH : m;
    const double cnt = (double)(e - b);
    int bad = 0;
    if (V2) {
        const double2* x2 = reinterpret_cast<const double2*>(x);
        const int64_t G2 = G / 2;
        const auto at = [&](int64_t i) { return x2[i * G2 + t]; };
        double s0 = 0.0, s1 = 0.0;
        ordered_walk4(
            b, e,
            [&](int64_t i) {
                const double2 v = at(i);
                bad |= not_finite(v.x) | not_finite(v.y);
                return v;
            },
            [&](double2 v) {
                s0 += v.x;
                s1 += v.y;
            });
        const double m0 = s0 / cnt, m1 = s1 / cnt;
        double q0 = 0.0, q1 = 0.0;
        ordered_walk4(b, e, at, [&](double2 v) {
            q0 += (v.x - m0) * (v.x - m0);
            q1 += (v.y - m1) * (v.y - m1);
        });
        reinterpret_cast<double2*>(pmean)[ch * G2 + t] = make_double2(m0, m1);
        reinterpret_cast<double2*>(pm2)[ch * G2 + t] = make_double2(q0, q1);
    } else {
        const auto at = [&](int64_t i) { return x[i * G + t]; };
        double s = 0.0;
        ordered_walk4(
            b, e,
            [&](int64_t i) {
                const double v = at(i);
                bad |= not_finite(v);
                return v;
            },
            [&](double v) { s += v; });
        const double m0 = s / cnt;
        double q = 0.0;
        ordered_walk4(b, e, at, [&](double v) { q += (v - m0) * (v - m0); });
        pmean[ch * G + t] = m0;
        pm2[ch * G + t] = q;
    }
    if (bad) flags[F_VALUE] = 1;
}

// ---- a block kept as CSC: indptr [m + 1] positions into idx / val, relative to the block.  indptr has been checked on
// the host (starts at 0, non-decreasing, ends at the block's number of entries), idx and val have not.

// The entries of the cells [0, m), one wave a cell: the value and pattern flags (csc_entry_flags).
__global__ __launch_bounds__(256) void gv_csc_check_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                           const double* __restrict__ val, int G, int64_t m,
                                                           int32_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= m) return;  // (a whole wave leaves)
    const int64_t kb = indptr[c], ke = indptr[c + 1];
    int bad = 0, bad_row = 0, bad_order = 0;
    for (int64_t k = kb + lane; k < ke; k += 64) {
        bad |= not_finite(val[k]);
        (void)csc_entry_flags(idx, k, kb, idx[k], G, bad_row, bad_order);
    }
    if (bad) flags[F_VALUE] = 1;
    if (bad_row) flags[F_PATTERN + CSC_F_ROW] = 1;
    if (bad_order) flags[F_PATTERN + CSC_F_ORDER] = 1;
}

// gv_dense_kernel for the genes of tile blockIdx.y and the chunk ch0 + blockIdx.x of a CSC block of m cells: no two
// threads meet at an accumulator (on a column that is not canonical they may, CSC_F_ORDER has been raised for it, and the
// addresses stay inside the tile).  The sum of the stored entries in cell order is the dense sum in cell order with terms
// of +0 left out, which changes no bit of it but the sign of a zero.
__global__ __launch_bounds__(256) void gv_csc_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                     const double* __restrict__ val, int G, int64_t m, int ch0,
                                                     double* __restrict__ pmean, double* __restrict__ pm2) {
    __shared__ double acc[GT], sq[GT];
    __shared__ int32_t stored[GT];
    __shared__ int64_t lo[NCH], hi[NCH];
    const int64_t ch = (int64_t)ch0 + blockIdx.x;
    const int g0 = blockIdx.y * GT, g1 = min(G, g0 + GT);
    const int64_t b = ch * NCH;
    const int cells = (int)((b + NCH < m ? b + NCH : m) - b);
    for (int i = threadIdx.x; i < g1 - g0; i += 256) {
        acc[i] = 0.0;
        sq[i] = 0.0;
        stored[i] = 0;
    }
    // (csc_tile_walk's first barrier stands between the clearing and the first addition)
    csc_tile_walk<NCH>(indptr, idx, m, ch, g0, g1, lo, hi, [&](int64_t, int64_t k, int r) {
        acc[r - g0] += val[k];
        stored[r - g0] += 1;
    });
    const double cnt = (double)cells;
    for (int i = threadIdx.x; i < g1 - g0; i += 256) acc[i] = acc[i] / cnt;  // the chunk means
    __syncthreads();
    csc_tile_walk<NCH>(indptr, idx, m, ch, g0, g1, lo, hi, [&](int64_t, int64_t k, int r) {
        const double d = val[k] - acc[r - g0];
        sq[r - g0] += d * d;
    });
    for (int i = threadIdx.x; i < g1 - g0; i += 256) {
        const double mu = acc[i];
        const double zeros = (double)(cells - stored[i]);
        pmean[ch * G + g0 + i] = mu;
        pm2[ch * G + g0 + i] = sq[i] + (zeros * mu) * mu;
    }
}

// The chunks [0, nch) of a block (pmean / pm2 [nch][G]) of a batch that held n_before cells before it, m cells in the
// block: folded in ascending order into state[g] (the mean), state[G + g] (M2).
__global__ __launch_bounds__(256) void gv_merge_kernel(const double* __restrict__ pmean, const double* __restrict__ pm2, int G,
                                                       int nch, int64_t n_before, int64_t m, double* __restrict__ state) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    GeneVarState s{(double)n_before, 0.0, 0.0};
    if (n_before > 0) {
        s.mean = state[g];
        s.m2 = state[G + g];
    }
    for (int ch = 0; ch < nch; ++ch) {
        const int64_t b = (int64_t)ch * NCH;
        const int64_t e = b + NCH < m ? b + NCH : m;
        s = genevar_merge(s, GeneVarState{(double)(e - b), pmean[(int64_t)ch * G + g], pm2[(int64_t)ch * G + g]});
    }
    state[g] = s.mean;
    state[G + g] = s.m2;
}

// state[G + g]: M2 -> the sample variance of the batch's n cells
__global__ __launch_bounds__(256) void gv_final_kernel(int G, int64_t n, double* __restrict__ state) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    state[G + g] = genevar_total(GeneVarState{(double)n, state[g], state[G + g]});
}

struct GeneVarResults {
    DevBuf<double> state;  // [2][G]: mean, then M2 (the batch complete: the variance)
};
struct GeneVarBatch : BlockLedger, GeneVarResults {
    static constexpr bool dense_x = false;  // (the store reserves no matrix: the cells pass through the block buffers)
};
struct GeneVarCscBatch : CscLedger, GeneVarResults {
    static constexpr bool dense_x = false;
};

}  // namespace

// What both handles share: the two streams, the block buffers' hand-over, the partials of a block, the merge and the
// results.  Slot: what a block buffer holds.
template <class Batch, class Slot>
class GeneVarBase : protected ResidentBatches<Batch> {
  protected:
    using Store = ResidentBatches<Batch>;
    using Store::batches_;
    using Store::cache_;
    using Store::device_;
    using Store::G_;
    using Store::ms_;
    using Store::stream_;
    using Store::timer_;

    GeneVarBase(int device, int G, const char* begin_entry) : Store(device, G, begin_entry) {
        CacheScope scope(&cache_);
        BMX_HIP(hipStreamCreateWithFlags(&kstream_, hipStreamNonBlocking));
        BMX_HIP(hipEventCreateWithFlags(&landed_, hipEventDisableTiming));
        for (hipEvent_t& e : done_) BMX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        BMX_HIP(hipMemsetAsync(flags_.reserve(F_WORDS), 0, F_WORDS * sizeof(int32_t), stream_));
        BMX_HIP(hipStreamSynchronize(stream_));
    }
    ~GeneVarBase() {
        this->retire({kstream_});
        if (landed_) (void)hipEventDestroy(landed_);
        for (hipEvent_t e : done_)
            if (e) (void)hipEventDestroy(e);
    }

    void begin_state(Batch& b) { b.state.reserve(2 * (size_t)G_); }

    // The block buffer the next block goes into.  Before the copy may overwrite it, the kernels of the block it held last
    // have finished (the copy stream waits for their event); before it is made larger, both streams are idle.
    template <class Grow>
    Slot& next_slot(bool must_grow, Grow&& grow) {
        const int i = nblocks_ & 1;
        if (must_grow) {
            BMX_HIP(hipStreamSynchronize(kstream_));
            BMX_HIP(hipStreamSynchronize(stream_));
            grow(slots_[i]);
        } else if (used_[i]) {
            BMX_HIP(hipStreamWaitEvent(stream_, done_[i], 0));
        }
        return slots_[i];
    }

    // Behind the copy of a block of m cells that has just been queued: reduce(pmean, pm2, chunks) queues the kernels that
    // write the block's partials, then the merge, the batch's last block also the variance.  b.filled counts the block.
    template <class F>
    void reduce_block(Batch& b, int64_t m, F&& reduce) {
        const int i = nblocks_ & 1;
        BMX_HIP(hipEventRecord(landed_, stream_));
        BMX_HIP(hipStreamWaitEvent(kstream_, landed_, 0));
        const int64_t nch = cdiv(m, NCH);
        if (nch > 0x7fffffffll) throw Error(BMX_ERR_ARG, "a block holds at most 2^31 - 1 chunks");
        double* part = part_.reserve(2 * (size_t)nch * G_);  // (grown only while kstream_ is idle: see below)
        const int ea = timer_.mark(kstream_);
        reduce(part, part + (size_t)nch * G_, (int)nch);
        BMX_LAUNCH_CHECK();
        const dim3 ggrid((unsigned)cdiv(G_, 256));
        hipLaunchKernelGGL(gv_merge_kernel, ggrid, dim3(256), 0, kstream_, (const double*)part,
                           (const double*)(part + (size_t)nch * G_), G_, (int)nch, b.filled - m, m, b.state.p);
        BMX_LAUNCH_CHECK();
        if (b.complete()) {
            hipLaunchKernelGGL(gv_final_kernel, ggrid, dim3(256), 0, kstream_, G_, b.n, b.state.p);
            BMX_LAUNCH_CHECK();
        }
        timer_.span(1, ea, timer_.mark(kstream_));
        BMX_HIP(hipEventRecord(done_[i], kstream_));
        used_[i] = true;
        ++nblocks_;
        if (b.complete()) {
            BMX_HIP(hipStreamSynchronize(stream_));
            BMX_HIP(hipStreamSynchronize(kstream_));
            timer_.collect(ms_);
        }
    }
    // part_ is read by kernels in flight: it grows only when a block needs more chunks than any before, after a drain
    void ensure_part(int64_t m) {
        const size_t want = 2 * (size_t)cdiv(m, NCH) * G_;
        if (want > part_.cap) {
            BMX_HIP(hipStreamSynchronize(kstream_));
            part_.reserve(want);
        }
    }

  public:
    // mean_out / total_out: [G x batches] column-major host memory
    void run(double* mean_out, double* total_out) {
        const double t0 = now_ms();
        if (batches_.empty()) throw Error(BMX_ERR_ARG, "no batch has been added");
        if (!mean_out || !total_out) throw Error(BMX_ERR_ARG, "an output matrix is missing");
        for (auto& b : batches_)
            if (!b->complete()) throw Error(BMX_ERR_ARG, "a batch has not received all its cells");
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        const size_t G = (size_t)G_;
        for (size_t i = 0; i < batches_.size(); ++i) {
            const double* s = batches_[i]->state.p;
            BMX_HIP(hipMemcpyAsync(mean_out + i * G, s, G * sizeof(double), hipMemcpyDeviceToHost, kstream_));
            BMX_HIP(hipMemcpyAsync(total_out + i * G, s + G, G * sizeof(double), hipMemcpyDeviceToHost, kstream_));
        }
        int32_t flags[F_WORDS] = {0, 0, 0};
        BMX_HIP(hipMemcpyAsync(flags, flags_.p, sizeof(flags), hipMemcpyDeviceToHost, kstream_));
        BMX_HIP(hipStreamSynchronize(kstream_));
        ms_[2] += now_ms() - t0;
        throw_if_bad_pattern(flags + F_PATTERN);
        if (flags[F_VALUE]) throw Error(BMX_ERR_ARG, "values should be finite");
    }

    // milliseconds since the handle was made: upload (host wall time of the staged copies, with the waits for a free
    // block buffer), HIP-event time of the kernels, host wall time of run
    void stage_ms(double* out3) const { std::memcpy(out3, ms_, 3 * sizeof(double)); }

  protected:
    hipStream_t kstream_ = nullptr;  // kernels (the store's stream_ takes the copies)
    hipEvent_t landed_ = nullptr, done_[2] = {nullptr, nullptr};
    bool used_[2] = {false, false};
    int64_t nblocks_ = 0;
    Slot slots_[2];
    DevBuf<double> part_;
    DevBuf<int32_t> flags_;
};

namespace {
struct DenseSlot {
    DevBuf<double> x;  // [m][G]
};
struct CscSlot {
    DevBuf<int64_t> indptr;   // [m + 1] relative to the block
    DevBuf<int32_t> indices;  // [nnz of the block] 0-based rows
    DevBuf<double> data;
};
}  // namespace

class GeneVar : public GeneVarBase<GeneVarBatch, DenseSlot> {
  public:
    GeneVar(int device, int G) : GeneVarBase(device, G, "bmx_genevar_begin_batch") {}

    void begin_batch(int64_t n) {
        check_cell_count(n);
        begin(n, [&](GeneVarBatch& b) { begin_state(b); });
    }

    // the next m cells of the batch begun last: x_block is G x m column-major host memory (pageable)
    void add_block(const double* x_block, int64_t m) {
        const double t0 = now_ms();
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        GeneVarBatch* bp = batches_.empty() ? nullptr : batches_.back().get();
        check_block(bp, x_block, m, begin_entry_);
        GeneVarBatch& b = *bp;
        genevar_check_block(b.n, b.filled, m);
        const size_t count = (size_t)m * G_;
        ensure_part(m);
        DenseSlot& slot = next_slot(count > slots_[nblocks_ & 1].x.cap, [&](DenseSlot& s) { s.x.reserve(count); });
        upload_pageable(slot.x.p, x_block, count * sizeof(double), stream_);
        b.filled += m;
        const int G = G_;
        const double* x = slot.x.p;
        reduce_block(b, m, [&](double* pmean, double* pm2, int nch) {
            if (G % 2 == 0)
                hipLaunchKernelGGL(gv_dense_kernel<true>, dim3((unsigned)nch, (unsigned)cdiv(G / 2, 256)), dim3(256), 0,
                                   kstream_, x, G, m, pmean, pm2, flags_.p);
            else
                hipLaunchKernelGGL(gv_dense_kernel<false>, dim3((unsigned)nch, (unsigned)cdiv(G, 256)), dim3(256), 0, kstream_,
                                   x, G, m, pmean, pm2, flags_.p);
        });
        ms_[0] += now_ms() - t0;
    }
};

class GeneVarSparse : public GeneVarBase<GeneVarCscBatch, CscSlot> {
  public:
    GeneVarSparse(int device, int G) : GeneVarBase(device, G, "bmx_genevar_sparse_begin_batch") {}

    // a batch of n cells with nnz stored entries in all
    void begin_batch(int64_t n, int64_t nnz) {
        check_cell_count(n);
        check_csc_begin(nnz);
        begin(n, [&](GeneVarCscBatch& b) {
            b.nnz = nnz;
            begin_state(b);
        });
    }

    // the next m cells of the batch begun last: indptr [m + 1] relative to the block, its nnz entries (pageable)
    void add_block(int64_t m, const int64_t* indptr, const int32_t* indices, const double* data, int64_t nnz) {
        const double t0 = now_ms();
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        GeneVarCscBatch* bp = batches_.empty() ? nullptr : batches_.back().get();
        check_block(bp, indptr, m, begin_entry_);
        GeneVarCscBatch& b = *bp;
        genevar_check_sparse_block(b.n, b.filled, m, indptr, indices, data, nnz);
        check_csc_entries(b, m, nnz);
        const size_t ne = (size_t)std::max<int64_t>(nnz, 1);
        ensure_part(m);
        const CscSlot& cur = slots_[nblocks_ & 1];
        CscSlot& slot = next_slot((size_t)m + 1 > cur.indptr.cap || ne > cur.indices.cap || ne > cur.data.cap, [&](CscSlot& s) {
            s.indptr.reserve((size_t)m + 1);
            s.indices.reserve(ne);
            s.data.reserve(ne);
        });
        upload_pageable(slot.indptr.p, indptr, (size_t)(m + 1) * sizeof(int64_t), stream_);
        upload_pageable(slot.indices.p, indices, (size_t)nnz * sizeof(int32_t), stream_);
        upload_pageable(slot.data.p, data, (size_t)nnz * sizeof(double), stream_);
        b.filled += m;
        b.nnz_filled += nnz;
        const int G = G_;
        const int64_t* ip = slot.indptr.p;
        const int32_t* idx = slot.indices.p;
        const double* val = slot.data.p;
        reduce_block(b, m, [&](double* pmean, double* pm2, int nch) {
            hipLaunchKernelGGL(gv_csc_check_kernel, dim3((unsigned)cdiv(m, 4)), dim3(256), 0, kstream_, ip, idx, val, G, m,
                               flags_.p);
            BMX_LAUNCH_CHECK();
            for (int ch = 0; ch < nch; ch += 65535) {  // (gene tiles on the first grid dimension would cap G instead)
                const unsigned k = (unsigned)std::min(65535, nch - ch);
                hipLaunchKernelGGL(gv_csc_kernel, dim3(k, (unsigned)cdiv(G, GT)), dim3(256), 0, kstream_, ip, idx, val, G, m, ch,
                                   pmean, pm2);
                BMX_LAUNCH_CHECK();
            }
        });
        ms_[0] += now_ms() - t0;
    }
};

}  // namespace bmx

/* ---------------------------------------------------------------- bmx_genevar_*, bmx_genevar_sparse_* ----------- */
struct bmx_genevar final : bmx::GeneVar {
    using GeneVar::GeneVar;
};
struct bmx_genevar_sparse final : bmx::GeneVarSparse {
    using GeneVarSparse::GeneVarSparse;
};

extern "C" {

int32_t bmx_genevar_create(int32_t device, int32_t G, bmx_genevar_t** out) {
    return bmx::guarded([&] {
        if (!out) throw bmx::Error(BMX_ERR_ARG, "null output pointer");
        bmx::genevar_check_create(G);
        *out = new bmx_genevar(device, G);
    });
}

void bmx_genevar_destroy(bmx_genevar_t* h) { delete h; }

int32_t bmx_genevar_check_create(int32_t G) {
    return bmx::guarded([&] { bmx::genevar_check_create(G); });
}

int32_t bmx_genevar_check_block(int64_t n, int64_t filled, int64_t n_block) {
    return bmx::guarded([&] { bmx::genevar_check_block(n, filled, n_block); });
}

int32_t bmx_genevar_check_sparse_block(int64_t n, int64_t filled, int64_t n_block, const int64_t* indptr,
                                       const int32_t* indices, const double* data, int64_t nnz) {
    return bmx::guarded([&] { bmx::genevar_check_sparse_block(n, filled, n_block, indptr, indices, data, nnz); });
}

int32_t bmx_genevar_begin_batch(bmx_genevar_t* h, int64_t n) {
    return bmx::guarded([&] { bmx::live(h).begin_batch(n); });
}

int32_t bmx_genevar_add_block(bmx_genevar_t* h, const double* x_block, int64_t n_block) {
    return bmx::guarded([&] { bmx::live(h).add_block(x_block, n_block); });
}

int32_t bmx_genevar_run(bmx_genevar_t* h, double* mean_out, double* total_out) {
    return bmx::guarded([&] { bmx::live(h).run(mean_out, total_out); });
}

int32_t bmx_genevar_stage_ms(const bmx_genevar_t* h, double* out3) {
    return bmx::guarded([&] {
        if (!h || !out3) throw bmx::Error(BMX_ERR_ARG, "null argument");
        h->stage_ms(out3);
    });
}

int32_t bmx_genevar_sparse_create(int32_t device, int32_t G, bmx_genevar_sparse_t** out) {
    return bmx::guarded([&] {
        if (!out) throw bmx::Error(BMX_ERR_ARG, "null output pointer");
        bmx::genevar_check_create(G);
        *out = new bmx_genevar_sparse(device, G);
    });
}

void bmx_genevar_sparse_destroy(bmx_genevar_sparse_t* h) { delete h; }

int32_t bmx_genevar_sparse_begin_batch(bmx_genevar_sparse_t* h, int64_t n, int64_t nnz) {
    return bmx::guarded([&] { bmx::live(h).begin_batch(n, nnz); });
}

int32_t bmx_genevar_sparse_add_block(bmx_genevar_sparse_t* h, int64_t n_block, const int64_t* indptr, const int32_t* indices,
                                     const double* data, int64_t nnz) {
    return bmx::guarded([&] { bmx::live(h).add_block(n_block, indptr, indices, data, nnz); });
}

int32_t bmx_genevar_sparse_run(bmx_genevar_sparse_t* h, double* mean_out, double* total_out) {
    return bmx::guarded([&] { bmx::live(h).run(mean_out, total_out); });
}

int32_t bmx_genevar_sparse_stage_ms(const bmx_genevar_sparse_t* h, double* out3) {
    return bmx::guarded([&] {
        if (!h || !out3) throw bmx::Error(BMX_ERR_ARG, "null argument");
        h->stage_ms(out3);
    });
}

}  // extern "C"
