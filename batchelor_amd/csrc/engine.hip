// Merge engine (host orchestration of the HIP kernels): R/fastMNN.R:398-562, R/MNN_tree.R:61-77,113-226.  This unit: the
// engine's lifetime and watchdog, the upload, the searches and the run; one merge is engine_merge.hip, the ranks'
// exchange engine_exchange.hip, what a finished run hands out engine_results.hip.
#include "engine_internal.hpp"
#include "host_xfer.hpp"
#include "merge_plan.hpp"
#include "rccl_dyn.hpp"

#include <atomic>
#include <chrono>
#include <cstring>
#include <limits>
#include <thread>

namespace bmx {
namespace {

// testing hook of the watchdog: spins on the 100 MHz real-time counter, then ends
__global__ void stall_kernel(unsigned long long ticks) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
}

// The run's device words go to the host by a STORE into pinned (host-coherent) memory, the sequence number last: the host
// spins on that word instead of waiting for a copy to be scheduled, signalled and polled through the runtime (measured:
// 100-170 us of idle GPU per wait that way, 14 waits per config-3 step).
__global__ void publish_state(const int32_t* __restrict__ st, int32_t* host, int seq) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int32_t v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = st[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) __hip_atomic_store(&host[i], v[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&host[8], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Several ranks, optimistic searches: a rank's "this search could not be completed on the device" flag (opt_state[0]) is
// all-gathered with the search's lists and OR-ed into every rank's own flag, so that the next wait of EVERY rank sees it and
// all of them start the run over at the same point (a rank that restarted alone would leave the others in a collective).
__global__ void stage_opt_flag(const int32_t* __restrict__ st, int32_t* __restrict__ slot) {
    if (threadIdx.x == 0 && blockIdx.x == 0) slot[0] = st[0];
}
__global__ void merge_opt_flags(const int32_t* __restrict__ flags, int world, int32_t* __restrict__ st) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int any = 0;
    for (int r = 0; r < world; ++r) any |= flags[4 * r];
    if (any) st[0] = 1;
}

// right cells named more than once: the pairs of all positions of a cell belong to the cell (rowsum groups by cell,
// R/fastMNN.R:571-579): fold[r] = the cell's pairs at its first position, 0 at the others
__global__ void fold_dup_counts(const int32_t* __restrict__ cnt, const int32_t* __restrict__ next, const int32_t* __restrict__ head,
                                int n, int32_t* __restrict__ fold) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    int t = 0;
    if (head[r])
        for (int p = r; p >= 0; p = next[p]) t += cnt[p];
    fold[r] = t;
}

}  // namespace

Engine::Engine(int device) : device_(device) {
    CacheScope cache_scope(&cache_);
    BMX_HIP(hipSetDevice(device_));
    stream_ = StreamPool::take();
    scal_.reserve(4096);
}

void Engine::check_alive() const {
    if (dead_)
        throw Error(BMX_ERR_HIP, "the engine is dead after a watchdog timeout (GPU work that never finished); restart the "
                                 "process to get the GPU back");
}

void Engine::mark_dead() {
    dead_ = true;
    cache_.leak = true;  // hipFree would wait for the device
    knn_ws_.abandon = true;
}

void Engine::wait(double work_s) {
    // the deadline covers everything queued since the last wait that came back (queued_work_s_), e.g. the
    // adjust_shift_variance of the previous merge in front of this merge's first search
    try {
        guarded_stream_sync(stream_, wd_base_s_ > 0.0 ? wd_base_s_ + queued_work_s_ + work_s : 0.0);
    } catch (const WatchdogTimeout&) {
        mark_dead();
        throw;
    }
    queued_work_s_ = 0.0;
}

void Engine::debug_stall(int ms) {
    check_alive();
    BMX_HIP(hipSetDevice(device_));
    hipLaunchKernelGGL(stall_kernel, dim3(1), dim3(64), 0, stream_, (unsigned long long)std::max(0, ms) * 100000ull);
    BMX_LAUNCH_CHECK();
}

Engine::~Engine() {
    (void)hipSetDevice(device_);
    if (dead_) {
        // nothing on this stream can be waited for: the stream, the communicator and the device blocks are abandoned
        DevBlockCache::current() = &cache_;
        return;
    }
    if (scal_pin_ && scal_pin_bytes_ > KnnWorkspace::kPinnedSmall) (void)hipHostFree(scal_pin_);
    else KnnWorkspace::pinned_small_give(scal_pin_);
    if (stream_) (void)hipStreamSynchronize(stream_);  // (a pair-list copy may still be on its way into the pinned block)
    if (copy_stream_) (void)hipStreamSynchronize(copy_stream_);
    if (pairs_ev_) (void)hipEventDestroy(pairs_ev_);
    if (pairs_ready_ev_) (void)hipEventDestroy(pairs_ready_ev_);
    PinnedBlocks::give(PinnedBlocks::Blk{pairs_pin_, pairs_pin_bytes_});
    if (comm_ && rccl::api().CommDestroy) {
        if (stream_) (void)hipStreamSynchronize(stream_);
        (void)rccl::api().CommDestroy(comm_);
    }
    for (hipEvent_t ev : up_ev_)
        if (ev) (void)hipEventDestroy(ev);
    // (a stream that reports an error is destroyed, an idle one parked for the next engine on this device)
    for (hipStream_t s : {copy_stream_, stream_}) {
        if (!s) continue;
        if (hipStreamSynchronize(s) == hipSuccess) StreamPool::give(s);
        else (void)hipStreamDestroy(s);
    }
    // the members' DevBufs are released after this body: into this engine's cache, which its own destructor frees
    DevBlockCache::current() = &cache_;
}

void Engine::ensure_uploaded(int b) {
    if (uploaded_[b]) return;
    const size_t bytes = (size_t)nrows_[b] * d_ * sizeof(double);
    if (!copy_stream_) copy_stream_ = StreamPool::take();
    if ((int)up_ev_.size() < B_) {
        const size_t old = up_ev_.size();
        up_ev_.resize(B_, nullptr);
        for (size_t i = old; i < up_ev_.size(); ++i) BMX_HIP(hipEventCreateWithFlags(&up_ev_[i], hipEventDisableTiming));
    }
    upload_pageable(inputs_cm_[b].p, host_data_[b], bytes, copy_stream_);
    BMX_HIP(hipEventRecord(up_ev_[b], copy_stream_));
    uploaded_[b] = 1;
}

void Engine::prefetch_one() {
    if (!lazy_) return;
    while (need_pos_ < need_order_.size() && uploaded_[need_order_[need_pos_]]) ++need_pos_;
    if (need_pos_ < need_order_.size()) ensure_uploaded(need_order_[need_pos_++]);
}

void Engine::upload(int nbatches, int d, const double* const* data, const int32_t* nrows,
                    const int32_t* const* restrict_idx, const int32_t* n_restrict, bool lazy) {
    check_alive();
    CacheScope cache_scope(&cache_);
    BMX_HIP(hipSetDevice(device_));
    root_.reset();  // results of an earlier run describe other inputs
    merges_.clear();
    if (emu_mode_ != 0) {  // a recording describes the exchanges of the inputs it was made on
        emu_rec_.clear();
        emu_mode_ = 0;
        rank_ = 0;
        world_ = 1;
    }
    if (nbatches < 2) throw Error(BMX_ERR_ARG, "at least two batches must be specified");  // R/fastMNN.R:345
    if (d < 1 || d > 256) throw Error(BMX_ERR_ARG, "number of dimensions must be in [1, 256]");
    B_ = nbatches;
    d_ = d;
    N_ = 0;
    nrows_.assign(nrows, nrows + nbatches);
    inputs_cm_.clear();
    inputs_cm_.resize(nbatches);
    inputs_restrict_.clear();
    inputs_restrict_.resize(nbatches);
    inputs_dup_.clear();
    inputs_dup_.resize(nbatches);
    has_dups_.assign(nbatches, 0);
    n_restrict_.assign(nbatches, -1);
    lazy_ = lazy;
    host_data_.assign(data, data + nbatches);
    uploaded_.assign(nbatches, 0);
    need_order_.clear();
    need_pos_ = 0;
    for (int b = 0; b < nbatches; ++b) {
        if (nrows[b] < 1) throw Error(BMX_ERR_ARG, "every batch needs at least one cell");
        N_ += nrows[b];
        double* p = inputs_cm_[b].reserve((size_t)nrows[b] * d);
        // the caller's matrices are pageable (R-owned): through the pinned staging ring at link speed (host_xfer.hpp)
        if (!lazy) {
            upload_pageable(p, data[b], (size_t)nrows[b] * d * sizeof(double), stream_);
            uploaded_[b] = 1;
        }
        const bool has = restrict_idx && restrict_idx[b] && n_restrict && n_restrict[b] >= 0;
        if (has) {
            const int m = n_restrict[b];
            if (m == 0) throw Error(BMX_ERR_ARG, "no cells remaining in a batch after restriction");  // R/checkInputs.R:116
            // an R subsetting vector in the caller's order (R/checkInputs.R:96-120 keeps it as given); a cell may be named
            // more than once (see Node::restrict_dups)
            const RestrictChains rc = restrict_chains(restrict_idx[b], m, nrows[b], 1);
            int32_t* rp = inputs_restrict_[b].reserve(m);
            BMX_HIP(hipMemcpyAsync(rp, rc.rows.data(), (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
            if (rc.dups) {
                int32_t* dp = inputs_dup_[b].reserve((size_t)2 * m);
                BMX_HIP(hipMemcpyAsync(dp, rc.chain.data(), (size_t)2 * m * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
            }
            has_dups_[b] = rc.dups ? 1 : 0;
            BMX_HIP(hipStreamSynchronize(stream_));  // rc goes out of scope
            n_restrict_[b] = m;
        }
    }
    if (N_ > std::numeric_limits<int32_t>::max() / 2) throw Error(BMX_ERR_ARG, "too many cells for int32 indices");
    BMX_HIP(hipStreamSynchronize(stream_));
    if (!lazy) host_data_.clear();  // the caller's matrices are free again
}

void Engine::knn(const double* X, const int32_t* ref_rows, int nr, const double* Q, const int32_t* q_rows, int nq,
                 int k, int32_t* idx, double* dist, const float* seed_d2, const double* centre, double* kth, bool gather,
                 const double* qcentre) {
    // query rows are split over ranks; the padded per-rank slices are contiguous, so the all-gather is in place
    int64_t b = 0, e = nq;
    bmx_shard_range_impl(nq, rank_, world_, &b, &e);
    // watchdog budget of this search's waits: ~1e4 times what the candidate pass takes per pair evaluation (1.5e-13 s),
    // and enough for a search that falls through to the FP64 scan (1e-10 s per pair and dimension)
    queued_work_s_ += 2e-10 * (double)nq * (double)nr * (double)d_ / 50.0;
    knn_ws_.wd_budget_s = wd_base_s_ > 0.0 ? wd_base_s_ + queued_work_s_ : 0.0;
    try {
        knn_device(stream_, knn_ws_, X, ref_rows, nr, Q, q_rows, d_, k, idx, dist, (int)b, (int)e, seed_d2, centre, kth, qcentre);
    } catch (const WatchdogTimeout&) {  // (the search's own waits go through knn_ws_.sync, not through wait())
        mark_dead();
        throw;
    }
    {
        const int64_t per = bmx_shard_rows_per_rank(nq, world_);
        // indices and distances of one search: grouped, RCCL sends them as one launch
        const bool flags = world_ > 1 && knn_ws_.optimistic;  // (see stage_opt_flag)
        int32_t* xf = nullptr;
        if (flags) {
            xf = xflags_.reserve((size_t)4 * world_);
            hipLaunchKernelGGL(stage_opt_flag, dim3(1), dim3(64), 0, stream_, (const int32_t*)knn_ws_.opt_state_ptr(stream_),
                               xf + 4 * rank_);
            BMX_LAUNCH_CHECK();
        }
        const bool group = (dist || kth || flags) && comm_ && world_ > 1 && rccl::api().GroupStart && rccl::api().GroupEnd;
        if (group) (void)rccl::api().GroupStart();
        try {
            // (gather = false: the caller goes on with its own slice of the lists and exchanges what it makes of them)
            if (gather) exchange(idx, per * k * (int64_t)sizeof(int32_t));
            if (gather && dist) exchange(dist, per * k * (int64_t)sizeof(double));
            if (gather && kth) exchange(kth, per * (int64_t)sizeof(double));
            if (flags) exchange(xf, 4 * (int64_t)sizeof(int32_t), /* flags_only */ true);
        } catch (...) {
            if (group) (void)rccl::api().GroupEnd();  // never leave the group open behind an error
            throw;
        }
        if (group && rccl::api().GroupEnd() != 0) throw Error(BMX_ERR_EXCHANGE, "ncclGroupEnd failed");
        if (flags) {
            hipLaunchKernelGGL(merge_opt_flags, dim3(1), dim3(64), 0, stream_, (const int32_t*)xf, world_,
                               knn_ws_.opt_state_ptr(stream_));
            BMX_LAUNCH_CHECK();
        }
    }
}

// The run's small device words (KnnWorkspace::opt_state: [0] optimistic search failed, [1] queries through the bounded exact
// sweep, [2] listed left cells, [3] pairs, [4] MNN-involved right cells) come back in ONE 32-byte copy per wait.
const int32_t* Engine::read_state() {
    int32_t* st = knn_ws_.opt_state_ptr(stream_);
    int32_t* pin = reinterpret_cast<int32_t*>(knn_ws_.pinned_words() + 8);  // [0..7] the words, [8] the sequence number
    if (state_seq_ == 0) pin[8] = 0;  // (a pooled block may hold an earlier engine's numbers)
    const int seq = ++state_seq_;
    hipLaunchKernelGGL(publish_state, dim3(1), dim3(64), 0, stream_, (const int32_t*)st, pin, seq);
    BMX_LAUNCH_CHECK();
    prefetch_one();  // (lazy upload: the host has nothing to do until the GPU is through -- move the next batch)
    // the wait: spin on the sequence word (host memory: no runtime call in the loop), with the watchdog's deadline
    const double budget = wd_base_s_ > 0.0 ? wd_base_s_ + queued_work_s_ : 0.0;
    const auto t0 = std::chrono::steady_clock::now();
    volatile int32_t* vp = pin;
    unsigned spins = 0;
    while (vp[8] != seq) {
        if ((++spins & 0x3FFu) == 0) {
            const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (budget > 0.0 && el > budget) {
                mark_dead();
                throw WatchdogTimeout("watchdog: the GPU work queued on the engine's stream did not finish in time; the engine is "
                                      "dead (restart the process)");
            }
            if (el > 0.5) {  // a long wait (adjust_shift_variance at scale): stop burning the core, and look for errors
                const hipError_t e = hipStreamQuery(stream_);
                (void)hipGetLastError();
                if (e != hipSuccess && e != hipErrorNotReady)
                    throw Error(BMX_ERR_HIP, std::string("the engine's stream failed: ") + hipGetErrorString(e));
                std::this_thread::sleep_for(std::chrono::microseconds(200));
            }
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    queued_work_s_ = 0.0;
    if (pin[0] != 0) {
        // a search of this rank alone (auto-merge's counts, dealt over the ranks) must not restart this rank alone: note it,
        // lower the device flag, go on; gather_counts tells everybody
        if (!solo_) throw OptimisticRetry();
        solo_flag_ = true;
        BMX_HIP(hipMemsetAsync(st, 0, sizeof(int32_t), stream_));
    }
    return pin;
}

Engine::MnnOut Engine::find_mnn(const Node& left, const Node& right, int k, double prop_k, const double* mu_left,
                                const double* mu_right) {
    // .restricted_mnn (R/MNN_tree.R:113-133): search among the restricted rows only
    const int nL = left.has_restrict ? left.n_restrict : left.n;
    const int nR = right.has_restrict ? right.n_restrict : right.n;
    const int32_t* lrows = left.has_restrict ? left.restrict_rows.p : nullptr;
    const int32_t* rrows = right.has_restrict ? right.restrict_rows.p : nullptr;
    MnnOut o;
    o.k1 = std::min(choose_k(k, prop_k, nL), nL);  // neighbours sought in LEFT for each right cell
    o.k2 = std::min(choose_k(k, prop_k, nR), nR);  // neighbours sought in RIGHT for each left cell
    if (o.k1 < 1 || o.k2 < 1) throw Error(BMX_ERR_ARG, "'k' must be positive");
    int32_t* st = knn_ws_.opt_state_ptr(stream_);
    const int64_t perR = bmx_shard_rows_per_rank(nR, world_) * (int64_t)world_;
    int32_t* idxRL = idxRL_.reserve((size_t)perR * o.k1);
    // 1. every right cell's neighbours in LEFT, with their distances
    double* distRL = distRL_.reserve((size_t)perR * o.k1);
    // (the other node's mean as the centre of the queries: the fp16 tier sweeps the references nearest to it first)
    knn(left.data.p, lrows, nL, right.data.p, rrows, nR, o.k1, idxRL, distRL, nullptr, mu_left, nullptr, true, mu_right);
    // 2. a pair needs its left cell in some right cell's list, so only those left cells are searched in RIGHT (with a
    //    growing merged reference most left cells are in nobody's list).  The result is the same set of pairs.
    const size_t stamp_cap = stampL_.cap;
    int32_t* stamp = stampL_.reserve(nL);
    if (stampL_.cap != stamp_cap) {  // a fresh block: stamps start at zero, the searches' numbers at one
        BMX_HIP(hipMemsetAsync(stamp, 0, stampL_.cap * sizeof(int32_t), stream_));
        if (stamp_gen_ > 0x7FFFFF00) stamp_gen_ = 0;
    }
    if (stamp_gen_ > 0x7FFFFF00) {
        BMX_HIP(hipMemsetAsync(stamp, 0, stampL_.cap * sizeof(int32_t), stream_));
        stamp_gen_ = 0;
    }
    const int gen = ++stamp_gen_;
    int32_t* offSel = offSel_.reserve((size_t)nL + 1);
    int32_t* lsel = lsel_.reserve(nL);
    // (an upper bound sizes what the selected cells accumulate into: their seeds and pair masks are zeroed as they are selected)
    const int64_t perLmax = bmx_shard_rows_per_rank(nL, world_) * (int64_t)world_;
    float* seed = seedL_.reserve((size_t)std::max<int64_t>(1, perLmax));
    unsigned long long* maskL = maskL_.reserve(std::max(1, nL));
    select_listed_rows(stream_, scan_ws_, idxRL, (int64_t)nR * o.k1, nL, stamp, gen, offSel, lsel, st + 2, seed, maskL);
    // A right cell r can only pair with a left cell l if it lists l, at a distance search 1 has just measured: the
    // largest such distance bounds how far search 2 has to look for l -- a tight starting threshold for free.  Rows may
    // come back short, padded with -1.  (The seeds only need the selected cells' positions, not their number.)
    seed_thresholds(stream_, idxRL, distRL, (int64_t)nR * o.k1, offSel, nL, seed, st + 2, rank_, world_);
    const int32_t nsel = read_state()[2];
    o.nsel = nsel;
    if (debug_prints()) fprintf(stderr, "[bmx] find_mnn: %d of %d left cells are in some right cell's list\n", nsel, nL);
    const int32_t* qsel = lsel;  // rows of left.data to query with
    if (lrows) {
        int32_t* q = qsel_.reserve(nsel);
        compose_row_list(stream_, lsel, nsel, lrows, q);
        qsel = q;
    }
    const int64_t perL = bmx_shard_rows_per_rank(nsel, world_) * (int64_t)world_;
    int32_t* idxLR = idxLR_.reserve((size_t)std::max<int64_t>(1, perL) * o.k2);
    double* kthL = kthL_.reserve((size_t)std::max<int64_t>(1, perL));
    // (the mean of the whole left node stands for the selected cells: the order is a heuristic, it only has to be cheap)
    knn(right.data.p, rrows, nR, left.data.p, qsel, nsel, o.k2, idxLR, nullptr, seed, mu_right, kthL, true, mu_left);
    int32_t* cntL = o.k2 > 64 ? cntL_.reserve(std::max(1, nsel)) : nullptr;
    int32_t* offL = offL_.reserve((size_t)nsel + 1);
    int32_t* partR = partR_.reserve((size_t)nR * o.k1);
    int32_t* cntR = cntR_.reserve(nR);
    int32_t* offR = offR_.reserve((size_t)nR + 1);
    int32_t* second_u = second_u_.reserve(nR);
    mutual_counts(stream_, idxLR, nsel, o.k2, idxRL, nR, o.k1, cntL, partR, cntR, lsel, offSel, maskL, /* mask_is_clear */ true,
                  distRL, kthL, &sorted_);
    const int32_t* cntR_cells = cntR;
    if (right.restrict_dups) {
        int32_t* fold = cntFold_.reserve(nR);
        hipLaunchKernelGGL(fold_dup_counts, dim3(cdiv(nR, 256)), dim3(256), 0, stream_, (const int32_t*)cntR,
                           (const int32_t*)right.dup_next.p, (const int32_t*)right.dup_head.p, nR, fold);
        BMX_LAUNCH_CHECK();
        cntR_cells = fold;
    }
    pair_scans(stream_, scan_ws_, maskL, cntL, nsel, o.k2, offL, st + 3, cntR_cells, nR, offR, second_u, st + 4);
    const int32_t* pin = read_state();
    o.P = pin[3];
    o.U = pin[4];
    return o;
}

void Engine::run(const bmx_params_t& p, const int32_t* tree, int tree_len) {
    CacheScope cache_scope(&cache_);
    BMX_HIP(hipSetDevice(device_));
    check_alive();
    // Optimistic first: the searches leave the count of their uncertified queries on the device and sweep them without a
    // host round trip (knn.hip: search_tiers).  A search that cannot be completed that way (hundreds of uncertified queries,
    // lists overflowing with exact ties) raises a device flag the waits of the merge loop look at; the run then starts over
    // from the resident inputs with host-checked searches.  Nothing of a merge is visible outside before the run returns.
    // With several ranks the flag is agreed on: it travels with every search's lists (Engine::knn) and with the counts of the
    // searches a rank runs alone (gather_counts), so all ranks see it at the same wait and start over together.
    knn_ws_.optimistic = !knn_ws_.force_exact;
    solo_ = solo_flag_ = false;
    try {
        run_once(p, tree, tree_len);
    } catch (const OptimisticRetry&) {
        if (debug_prints()) fprintf(stderr, "[bmx] optimistic run gave up; repeating with host-checked searches\n");
        ++optimistic_retries_;
        knn_ws_.optimistic = false;
        run_once(p, tree, tree_len);
    }
    knn_ws_.optimistic = false;
}

void Engine::run_once(const bmx_params_t& p, const int32_t* tree, int tree_len) {
    if (B_ < 2) throw Error(BMX_ERR_ARG, "at least two batches must be specified");
    if (p.k < 1) throw Error(BMX_ERR_ARG, "'k' must be positive");
    reset_run();
    if (!p.auto_merge)
        run_tree(p, tree, tree_len);
    else
        run_auto(p);
    finish_run();
}

void Engine::reset_run() {
    queued_work_s_ = 0.0;
    root_.reset();  // a run that fails half-way leaves nothing to download
    pairs_pinned_ = false;
    merges_.clear();
    merges_.resize(B_ - 1);
    n_extras_ = 0;
    xchg_calls_ = xchg_bytes_ = 0;
    emu_next_ = 0;
    knn_ws_.events_used = 0;
    knn_ws_.replay_idx = 0;
    asv_pairs_ = 0.0;
    vecs_.reserve((size_t)(2 * B_ + 8) * d_);
    // statistics slots (column means [d] + total variance) and batch.size scalars: a merge takes at most one per
    // segment before and after its centring, plus one
    slot_cap_ = (2 * B_ + 2) * B_ + 8;
    n_slots_ = 0;
    scal_.reserve(slot_cap_);
    means_pool_.reserve((size_t)slot_cap_ * d_);
    BMX_HIP(hipMemsetAsync(scal_.p, 0, (size_t)slot_cap_ * sizeof(double), stream_));
    BMX_HIP(hipMemsetAsync(knn_ws_.opt_state_ptr(stream_), 0, 8 * sizeof(int32_t), stream_));
    scal_host_.assign(slot_cap_, 0.0);
    knn_ws_.exact_total = knn_ws_.tier2_total = 0;
}

// a leaf: the row-major working copy of resident input b
std::unique_ptr<Node> Engine::make_leaf(int b, double* arena_rows) {
    auto n = std::make_unique<Node>();
    n->index = {b + 1};
    n->n = nrows_[b];
    n->origin = {Segment{b + 1, nrows_[b]}};
    double* dp;
    if (arena_rows) {
        n->data.alias(arena_rows, (size_t)n->n * d_);
        dp = n->data.p;
    } else {
        dp = n->data.reserve((size_t)n->n * d_);
    }
    if (lazy_) {  // the batch may still be on its way: the transpose queues behind its copy
        if ((size_t)b >= host_data_.size() && !uploaded_[b])
            throw Error(BMX_ERR_ARG, "internal: a lazily uploaded batch has lost its host matrix");
        ensure_uploaded(b);
        BMX_HIP(hipStreamWaitEvent(stream_, up_ev_[b], 0));
    }
    transpose_cm_to_rm(stream_, inputs_cm_[b].p, n->n, d_, dp);
    if (n_restrict_[b] >= 0) {
        const int m = n_restrict_[b];
        const int32_t* chain = has_dups_[b] ? inputs_dup_[b].p : nullptr;  // [2 m]: next, then head
        copy_restrict(*n, m, inputs_restrict_[b].p, chain, chain ? chain + m : nullptr);
    }
    return n;
}

// Predefined tree: the leaves go into ONE arena in the order the post-order code names them (= left to right in the
// tree), so the two children of every merge are adjacent row ranges and the merged node is their union in place.
void Engine::run_tree(const bmx_params_t& p, const int32_t* tree, int tree_len) {
    double* arena = arena_.reserve((size_t)N_ * d_);
    const MergePlan plan = plan_merges(tree, tree_len, B_, nrows_.data());
    if (lazy_) {  // the order in which the merges will ask for the batches: what to prefetch next
        need_order_ = plan.need_order;
        need_pos_ = 0;
    }
    // finished nodes: a leaf is materialised when its merge comes up (a lazily uploaded batch arrives in the meantime)
    std::vector<std::unique_ptr<Node>> nodes(plan.nodes.size());
    const auto t_run = std::chrono::steady_clock::now();
    for (int mdx = 0; mdx < B_ - 1; ++mdx) {
        const int cur = plan.merges[mdx];
        const PlanNode& s = plan.nodes[cur];
        for (int child : {s.left, s.right})
            if (!nodes[child]) nodes[child] = make_leaf(plan.nodes[child].batch, arena + (size_t)plan.nodes[child].row0 * d_);
        std::unique_ptr<Node> merged;
        if (debug_timings())  // (host clock: when the host got to queue this merge)
            fprintf(stderr, "[bmx]   merge %d queued from %.2f ms\n", mdx + 1,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_run).count());
        merge_step(mdx, *nodes[s.left], *nodes[s.right], p, merged);
        nodes[s.left].reset();
        nodes[s.right].reset();
        nodes[cur] = std::move(merged);  // .update_tree (R/MNN_tree.R:71-77)
    }
    root_ = std::move(nodes.back());
}

// auto-merge (R/MNN_tree.R:154-226) picks pairs as it goes: its leaves own their buffers and a merge copies
void Engine::run_auto(const bmx_params_t& p) {
    std::vector<std::unique_ptr<Node>> rem;
    for (int b = 0; b < B_; ++b) rem.push_back(make_leaf(b, nullptr));
    CountMatrix stats(B_, std::vector<int64_t>(B_, 0));
    {
        // .initialize_auto_search (R/MNN_tree.R:160-164): B (B - 1) / 2 independent counts.  With several ranks they are
        // dealt round robin -- each a whole, unsharded search on its rank: no gathers inside, all ranks busy -- and the
        // numbers all-gathered at the end, instead of every rank walking every count with row-split searches
        std::vector<std::pair<int, int>> todo;
        for (int i = 0; i < B_; ++i)
            for (int j = 0; j < i; ++j) todo.emplace_back(i, j);
        std::vector<int32_t> counts = solo_counts((int)todo.size(), [&](int t) {
            return count_mnn_pairs(*rem[todo[t].first], *rem[todo[t].second], p);
        });
        for (size_t t = 0; t < todo.size(); ++t) stats[todo[t].first][todo[t].second] = counts[t];
    }
    for (int mdx = 0; mdx < B_ - 1; ++mdx) {
        const BestMerge best = pick_best_merge(stats);
        if (best.count <= 0) throw Error(BMX_ERR_NO_PAIRS, "no mutual nearest neighbours found between batches");
        std::unique_ptr<Node> merged;
        merge_step(mdx, *rem[best.left], *rem[best.right], p, merged);
        // .update_remainders: drop both, recount the new node against every remaining one
        std::vector<int> keep;
        CountMatrix ns = drop_merged(stats, best.left, best.right, keep);
        std::vector<std::unique_ptr<Node>> nrem;
        for (int i : keep) nrem.push_back(std::move(rem[i]));
        if (!keep.empty()) {
            const std::vector<int32_t> all = recount_merged(*merged, nrem, p);
            for (size_t c = 0; c < keep.size(); ++c) ns[keep.size()][c] = all[c];
        }
        nrem.push_back(std::move(merged));
        rem = std::move(nrem);
        stats = std::move(ns);
    }
    root_ = std::move(rem[0]);
}

// .update_remainders (R/MNN_tree.R:205-226): the pairs of the new node with every remaining one
std::vector<int32_t> Engine::recount_merged(const Node& merged, const std::vector<std::unique_ptr<Node>>& rem,
                                            const bmx_params_t& p) {
    // upstream keeps orthogonalising the SAME left copy across j (R/MNN_tree.R:185-186)
    // (.update_remainders, R/MNN_tree.R:205-226: the K counts are dealt over the ranks like the initial ones; the
    // orthogonalisations of the shared left copy are cheap row passes every rank applies in order)
    const int K = (int)rem.size();
    std::unique_ptr<Node> lcopy = clone_node(merged);
    std::vector<int32_t> mine((size_t)K, 0);
    for (int c = 0; c < K; ++c) {
        orthogonalize(*lcopy, rem[c]->extras);
        if (c % world_ != rank_) continue;
        const Node* r = rem[c].get();
        std::unique_ptr<Node> rc;
        if (!merged.extras.empty()) {
            rc = clone_node(*rem[c]);
            orthogonalize(*rc, merged.extras);
            r = rc.get();
        }
        SoloRank solo(this);  // an unsharded search on this rank alone
        mine[c] = (int32_t)find_mnn(*lcopy, *r, p.k, p.prop_k).P;
    }
    return gather_counts(mine);
}

// what the host reads back when the merges are queued: the run's scalars, the last search's state, the pair lists
void Engine::finish_run() {
    const size_t scal_bytes = scal_host_.size() * sizeof(double);
    if (scal_bytes > scal_pin_bytes_) {  // (more than ~60 batches: a block of its own instead of a pooled 64 KiB one)
        if (scal_pin_ && scal_pin_bytes_ > KnnWorkspace::kPinnedSmall) (void)hipHostFree(scal_pin_);
        else KnnWorkspace::pinned_small_give(scal_pin_);
        scal_pin_ = nullptr;
        if (scal_bytes <= KnnWorkspace::kPinnedSmall) {
            scal_pin_ = static_cast<double*>(KnnWorkspace::pinned_small_take());
            scal_pin_bytes_ = KnnWorkspace::kPinnedSmall;
        } else {
            BMX_HIP(hipHostMalloc((void**)&scal_pin_, scal_bytes, hipHostMallocDefault));
            scal_pin_bytes_ = scal_bytes;
        }
    }
    BMX_HIP(hipMemcpyAsync(scal_pin_, scal_.p, scal_host_.size() * sizeof(double), hipMemcpyDeviceToHost, stream_));
    // (with var_adj the last merge's adjust_shift_variance is still running: its budget is n2 (nr1 + nr2) pair visits)
    const int32_t* fin = read_state();  // (the last tricube search's flag is looked at here)
    knn_ws_.exact_total += fin[1];
    std::memcpy(scal_host_.data(), scal_pin_, scal_host_.size() * sizeof(double));
    if (lazy_) {  // every batch is resident now: later runs need nothing from the caller
        for (int b = 0; b < B_; ++b) ensure_uploaded(b);
        BMX_HIP(hipStreamSynchronize(copy_stream_));
        host_data_.clear();
        lazy_ = false;
    }
    fallbacks_ = knn_ws_.exact_total;
    stage_pairs();
}

}  // namespace bmx
