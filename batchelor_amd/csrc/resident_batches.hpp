// What the handles that keep genes x cells batches in HBM (Pca, PcaSparse, Cluster, ClusterSparse, Linear, Norm,
// NormSparse, Delta, DeltaSparse) have
// in common: the guard their C entry points go through, the argument checks of a batch, the bookkeeping of a batch that
// arrives in column blocks -- dense, or CSC (NormSparse, PcaSparse, DeltaSparse, ClusterSparse) --, the event-pair stage timer, the store that owns
// the cache, the copy stream, the batches and the stage times, and the blocked pass that writes every cell (or every
// stored entry).  The checks, the bookkeeping and the cutting of output blocks make no HIP call.  GeneVar / GeneVarSparse
// (gene_var.hip) use the store for everything but the batches' cells, which only pass through two block buffers.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <memory>
#include <string>
#include <vector>

#include "bmx_common.hpp"
#include "host_xfer.hpp"

namespace bmx {

inline double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ---- the extern "C" boundary (abi.hip).  Nothing throws across it: fn runs, an exception becomes its status code and
// the thread's bmx_last_error() text.
int guarded(const std::function<void()>& fn);
// the handle an entry point was given
template <class H>
H& live(H* h) {
    if (!h) throw Error(BMX_ERR_ARG, "null handle");
    return *h;
}

// ---- argument checks, without a device (throw Error(BMX_ERR_ARG))
// int32_cells: the handle indexes a batch's cells with 32-bit integers
inline void check_cell_count(int64_t n, bool int32_cells = true) {
    if (n < 1) throw Error(BMX_ERR_ARG, "every batch needs at least one cell");
    if (int32_cells && n > 0x7fffffffll) throw Error(BMX_ERR_ARG, "a batch holds at most 2^31 - 1 cells");
}
// a batch's restriction: 1-based cells of its n, in any order; a null list or n_restrict < 0 means all cells
inline bool is_restricted(const int32_t* restrict_idx, int64_t n_restrict) { return restrict_idx && n_restrict >= 0; }
inline void check_restriction(int64_t n, const int32_t* restrict_idx, int64_t n_restrict) {
    if (!is_restricted(restrict_idx, n_restrict)) return;
    if (n_restrict == 0) throw Error(BMX_ERR_ARG, "no cells remaining in a batch after restriction");
    if (n_restrict > 0x7fffffffll) throw Error(BMX_ERR_ARG, "'restrict' names at most 2^31 - 1 cells");
    for (int64_t i = 0; i < n_restrict; ++i)
        if (restrict_idx[i] < 1 || restrict_idx[i] > n) throw Error(BMX_ERR_ARG, "'restrict' indices out of range");
}

// ---- a batch announced with n cells whose columns arrive in blocks, in order
struct BlockLedger {
    int64_t n = 0;       // cells announced
    int64_t filled = 0;  // cells received so far
    bool complete() const { return filled == n; }
};
// `last`: the batch begun before, if any
inline void check_begin(const BlockLedger* last) {
    if (last && !last->complete()) throw Error(BMX_ERR_ARG, "the previous batch has not received all its cells");
}
// `open`: the batch begun last, if any; `begin_entry`: the entry point that begins one ("bmx_pca_begin_batch")
inline void check_block(const BlockLedger* open, const void* x_block, int64_t m, const char* begin_entry) {
    if (!open) throw Error(BMX_ERR_ARG, std::string(begin_entry) + " has not been called");
    if (m < 1 || open->filled + m > open->n) throw Error(BMX_ERR_ARG, "the block does not fit into the batch announced");
    if (!x_block) throw Error(BMX_ERR_ARG, "the block is missing");
}

// ---- the same for a batch kept as CSC: n cells with nnz stored entries in all
struct CscLedger : BlockLedger {
    int64_t nnz = 0, nnz_filled = 0;  // entries announced, received so far
};
// a block of m cells for a batch of n cells that holds `filled` so far: indptr [m + 1] relative to the block (starts at
// 0, never decreases, ends at nnz); indices / data [nnz]
inline void check_csc_block(int64_t n, int64_t filled, int64_t m, const int64_t* indptr, const int32_t* indices,
                            const double* data, int64_t nnz) {
    if (!indptr) throw Error(BMX_ERR_ARG, "the block's 'indptr' is missing");
    if (nnz < 0) throw Error(BMX_ERR_ARG, "the block's number of stored entries is negative");
    if (nnz > 0 && (!indices || !data)) throw Error(BMX_ERR_ARG, "the block's 'indices' or 'data' is missing");
    if (n < 1 || filled < 0 || m < 1 || m > n || filled > n - m)
        throw Error(BMX_ERR_ARG, "the block does not fit into the batch announced");
    if (indptr[0] != 0) throw Error(BMX_ERR_ARG, "the block's 'indptr' does not start at 0");
    for (int64_t i = 0; i < m; ++i)
        if (indptr[i + 1] < indptr[i]) throw Error(BMX_ERR_ARG, "the block's 'indptr' decreases");
    if (indptr[m] != nnz) throw Error(BMX_ERR_ARG, "the block's 'indptr' does not end at its number of stored entries");
}
inline void check_csc_begin(int64_t nnz) {
    if (nnz < 0) throw Error(BMX_ERR_ARG, "the batch's number of stored entries is negative");
}
// the next m cells of `open` bring nnz entries (the block has passed check_block and check_csc_block)
inline void check_csc_entries(const CscLedger& open, int64_t m, int64_t nnz) {
    if (nnz > open.nnz - open.nnz_filled) throw Error(BMX_ERR_ARG, "the block holds more entries than the batch announced");
    if (open.filled + m == open.n && open.nnz_filled + nnz != open.nnz)
        throw Error(BMX_ERR_ARG, "the batch has received fewer entries than it announced");
}
// what the kernels that read every stored entry report (csc_device.hpp: csc_entry_flags), a pair of adjacent device words:
// a row index outside [0, G), rows of a column that do not ascend strictly
enum { CSC_F_ROW = 0, CSC_F_ORDER = 1, CSC_F_WORDS = 2 };
inline void throw_if_bad_pattern(const int32_t* pair) {
    if (pair[CSC_F_ROW]) throw Error(BMX_ERR_ARG, "sparse counts: a row index is outside [0, number of genes)");
    if (pair[CSC_F_ORDER])
        throw Error(BMX_ERR_ARG, "sparse counts: the row indices of a column should be strictly ascending");
}

// ---- the per-gene sums of a batch whose cells are cut into chunks of `width` at fixed positions: a chunk is summed by
// the first block after which all its cells are resident, so the chunk edges never depend on the blocks
struct ChunkProgress {
    int nchunks = 0;   // chunks of the whole batch
    int sum_done = 0;  // chunks summed so far
    // the chunks that are complete with `have` of the batch's `total` cells resident: the whole ones, and with the last
    // cell the short one at the end
    int chunks_complete(int64_t have, int64_t total, int width) const {
        return have == total ? nchunks : (int)(have / width);
    }
};

// ---- a block of a pass that writes every cell or stored entry: the cells [c0, c0 + mb) of batch bi, `count` elements
// that go to outs[bi] + at
struct OutBlock {
    int bi;
    int64_t c0;
    int mb;
    int64_t at, count;
};
// The blocks of a CSC batch of n cells, hindptr [n + 1] its absolute indptr: runs of whole cells in order, each up to the
// last cell boundary within cap_elements stored entries and max_cells cells, one cell at the least; a run without entries
// has nothing to write and is left out.  (bi is 0: the caller names the batch.)
inline std::vector<OutBlock> plan_csc_output_blocks(const int64_t* hindptr, int64_t n, int64_t cap_elements,
                                                    int64_t max_cells = (int64_t)1 << 30) {
    std::vector<OutBlock> blocks;
    for (int64_t c0 = 0; c0 < n;) {
        const int64_t end = std::min(n, c0 + max_cells);
        int64_t c1 = std::upper_bound(hindptr + c0, hindptr + end + 1, hindptr[c0] + cap_elements) - hindptr - 1;
        c1 = std::max(c1, c0 + 1);
        if (hindptr[c1] > hindptr[c0]) blocks.push_back({0, c0, (int)(c1 - c0), hindptr[c0], hindptr[c1] - hindptr[c0]});
        c0 = c1;
    }
    return blocks;
}

// ---- device time by stage, from pairs of events
class SpanTimer {
  public:
    ~SpanTimer() {
        for (hipEvent_t e : events_) (void)hipEventDestroy(e);
    }
    // a timing event recorded on `stream` now
    int mark(hipStream_t stream) {
        if (next_ == (int)events_.size()) {
            hipEvent_t e = nullptr;
            BMX_HIP(hipEventCreate(&e));
            events_.push_back(e);
        }
        BMX_HIP(hipEventRecord(events_[(size_t)next_], stream));
        return next_++;
    }
    hipEvent_t event(int i) const { return events_[(size_t)i]; }
    void span(int stage, int a, int b) { spans_.push_back({stage, a, b}); }
    // the spans since the last call go into ms[stage] and the events are free again (the streams marked are idle)
    void collect(double* ms) {
        for (const Span& s : spans_) {
            float t = 0.0f;
            if (hipEventElapsedTime(&t, events_[(size_t)s.a], events_[(size_t)s.b]) == hipSuccess) ms[s.stage] += (double)t;
            (void)hipGetLastError();
        }
        spans_.clear();
        next_ = 0;
    }

  private:
    struct Span {
        int stage, a, b;
    };
    std::vector<hipEvent_t> events_;
    int next_ = 0;
    std::vector<Span> spans_;
};

// ---- the store.  Batch: a struct derived from ResidentBatch with the handle's own per-batch buffers -- or, for a handle
// that keeps its cells as CSC, from CscBatch: begin_csc() / add_csc() are then what begin() / add() are for the others.
struct ResidentBatch : BlockLedger {
    static constexpr bool dense_x = true;
    DevBuf<double> x;  // [n][G] (= genes x cells column-major)
};
struct CscBatch : CscLedger {
    static constexpr bool dense_x = false;
    DevBuf<int64_t> indptr;        // [n + 1] absolute positions
    DevBuf<int32_t> indices;       // [nnz] 0-based rows
    DevBuf<double> data;           // [nnz]
    std::vector<int64_t> hindptr;  // indptr on the host: a pass over the stored entries cuts its blocks by it
};

template <class Batch>
class ResidentBatches {
  public:
    ResidentBatches(int device, int G, const char* begin_entry) : device_(device), G_(G), begin_entry_(begin_entry) {
        BMX_HIP(hipSetDevice(device_));
        BMX_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    }
    ResidentBatches(const ResidentBatches&) = delete;
    ResidentBatches& operator=(const ResidentBatches&) = delete;
    // milliseconds by stage since the handle was made (the handle says which five)
    void stage_ms(double* out5) const { std::memcpy(out5, ms_, sizeof(ms_)); }

  protected:
    // Destruction.  A DevBuf hands its block to the cache DevBlockCache::current() names at that moment, so two things
    // must hold for every DevBuf of the store, of its batches and of the derived handle: (1) current() names cache_
    // before the first of them is released, and (2) cache_ is destroyed after the last.  (2): cache_ is the first member
    // of this base, and a base's members go after everything the derived class declares.  (1): the derived class's
    // destructor BODY -- which runs before any member is released -- calls retire(); this destructor alone would be
    // too late for the derived members.  retire() also drains and destroys the copy stream, then `more` in order.
    void retire(std::initializer_list<hipStream_t> more = {}) {
        (void)hipSetDevice(device_);
        if (stream_) {
            (void)hipStreamSynchronize(stream_);
            (void)hipStreamDestroy(stream_);
            stream_ = nullptr;
        }
        for (hipStream_t s : more)
            if (s) {
                (void)hipStreamSynchronize(s);
                (void)hipStreamDestroy(s);
            }
        DevBlockCache::current() = &cache_;  // the blocks go back to this handle's cache, which frees them
    }
    ~ResidentBatches() = default;

    // A new batch of n cells (the caller has checked n: check_cell_count): x is reserved (a dense batch), then fill(batch)
    // reserves and uploads what else the handle keeps for it; the batch joins the list when fill returns.
    template <class F>
    void begin(int64_t n, F&& fill) {
        check_begin(batches_.empty() ? nullptr : batches_.back().get());
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        auto nb = std::make_unique<Batch>();
        nb->n = n;
        if constexpr (Batch::dense_x) nb->x.reserve((size_t)n * G_);
        fill(*nb);
        batches_.push_back(std::move(nb));
    }
    // The next m cells (columns) of the batch begun last: x_block is G x m column-major host memory (pageable is fine: it
    // goes through the pinned staging ring, which has taken the block by the time the copy is queued).  The copy is
    // queued on the copy stream, then queued(batch, p) does the handle's work behind it: p is where the block lands,
    // batch.filled already counts it.
    template <class F>
    void add(const double* x_block, int64_t m, F&& queued) {
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        Batch* b = batches_.empty() ? nullptr : batches_.back().get();
        check_block(b, x_block, m, begin_entry_);
        double* p = b->x.p + b->filled * G_;
        upload_pageable(p, x_block, (size_t)m * G_ * sizeof(double), stream_);
        b->filled += m;
        queued(*b, p);
    }
    // begin() for a CSC batch with nnz stored entries in all: the three arrays are reserved before fill(batch) runs
    template <class F>
    void begin_csc(int64_t n, int64_t nnz, F&& fill) {
        check_csc_begin(nnz);
        begin(n, [&](Batch& b) {
            b.nnz = nnz;
            b.indptr.reserve((size_t)n + 1);
            b.indices.reserve((size_t)std::max<int64_t>(nnz, 1));
            b.data.reserve((size_t)std::max<int64_t>(nnz, 1));
            b.hindptr.assign((size_t)n + 1, 0);
            fill(b);
        });
    }
    // add() for a CSC batch: indptr [m + 1] relative to the block, its nnz entries (pageable).  indptr goes up rebased
    // to absolute positions; queued(batch, first cell of the block) runs with filled / nnz_filled already advanced.
    template <class F>
    void add_csc(int64_t m, const int64_t* indptr, const int32_t* indices, const double* data, int64_t nnz, F&& queued) {
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        Batch* bp = batches_.empty() ? nullptr : batches_.back().get();
        check_block(bp, indptr, m, begin_entry_);
        Batch& b = *bp;
        check_csc_block(b.n, b.filled, m, indptr, indices, data, nnz);
        check_csc_entries(b, m, nnz);
        int64_t* habs = b.hindptr.data() + b.filled;
        for (int64_t i = 0; i <= m; ++i) habs[i] = b.nnz_filled + indptr[i];
        upload_pageable(b.indptr.p + b.filled, habs, (size_t)(m + 1) * sizeof(int64_t), stream_);
        upload_pageable(b.indices.p + b.nnz_filled, indices, (size_t)nnz * sizeof(int32_t), stream_);
        upload_pageable(b.data.p + b.nnz_filled, data, (size_t)nnz * sizeof(double), stream_);
        b.filled += m;
        b.nnz_filled += nnz;
        queued(b, b.filled - m);
    }

    DevBlockCache cache_;  // first: see retire()
    int device_, G_;
    const char* begin_entry_;
    hipStream_t stream_ = nullptr;  // copies (and, in Pca and Cluster, the kernels)
    std::vector<std::unique_ptr<Batch>> batches_;
    SpanTimer timer_;                 // the stages' event pairs, collected into ms_
    double ms_[5] = {0, 0, 0, 0, 0};  // what stage_ms reports (Pca reports none and leaves both alone)
};

// ---- a pass that writes the blocks of a list (none: nothing happens) through the two device buffers of `buf`, sized
// by the largest block: launch(block, device out) queues the kernel of a block on `kstream`; the block then goes to
// outs[bi] + at through the download ring on `copy` while the next block's kernel runs into the other buffer.  The
// kernels' event time goes to the timer's `stage`.  Both streams are idle when this returns.
template <class F>
void run_output_blocks(const std::vector<OutBlock>& blocks, hipStream_t kstream, hipStream_t copy, SpanTimer& timer,
                       int stage, DevBuf<double> (&buf)[2], double* const* outs, F&& launch) {
    if (blocks.empty()) return;
    int64_t largest = 1;
    for (const OutBlock& k : blocks) largest = std::max(largest, k.count);
    double* dev[2] = {buf[0].reserve((size_t)largest), buf[1].reserve((size_t)largest)};
    std::vector<int> done(blocks.size(), -1);
    auto queue = [&](size_t i) {
        const int ea = timer.mark(kstream);
        launch(blocks[i], dev[i & 1]);
        BMX_LAUNCH_CHECK();
        done[i] = timer.mark(kstream);
        timer.span(stage, ea, done[i]);
    };
    queue(0);
    for (size_t i = 0; i < blocks.size(); ++i) {
        if (i + 1 < blocks.size()) queue(i + 1);  // (its buffer was emptied by the download of block i - 1)
        const OutBlock& k = blocks[i];
        BMX_HIP(hipStreamWaitEvent(copy, timer.event(done[i]), 0));
        download_pageable(outs[k.bi] + k.at, dev[i & 1], (size_t)k.count * sizeof(double), copy);
    }
    BMX_HIP(hipStreamSynchronize(kstream));
    BMX_HIP(hipStreamSynchronize(copy));
}

// every cell of every dense batch (Linear, Norm), in blocks of at most `per` cells: launch(bi, batch, first cell, cells,
// device out)
template <class Batch, class F>
void blocked_output(const std::vector<std::unique_ptr<Batch>>& batches, int G, int64_t per, hipStream_t kstream,
                    hipStream_t copy, SpanTimer& timer, int stage, DevBuf<double> (&buf)[2], double* const* outs,
                    F&& launch) {
    std::vector<OutBlock> blocks;
    for (size_t bi = 0; bi < batches.size(); ++bi)
        for (int64_t c0 = 0; c0 < batches[bi]->n; c0 += per) {
            const int64_t mb = std::min(per, batches[bi]->n - c0);
            blocks.push_back({(int)bi, c0, (int)mb, c0 * G, mb * G});
        }
    run_output_blocks(blocks, kstream, copy, timer, stage, buf, outs, [&](const OutBlock& k, double* out) {
        launch(k.bi, *batches[(size_t)k.bi], k.c0, k.mb, out);
    });
}

}  // namespace bmx
