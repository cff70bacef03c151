// Merge engine, what a finished run hands out: the corrected rows and merge records, the pair lists (staged in pinned
// memory when the run ends), the diagnostics' snapshots and tallies, and the profiles.
#include "engine_internal.hpp"
#include "host_xfer.hpp"

#include <cstdlib>
#include <cstring>
#include <limits>

namespace bmx {

void Engine::download(double* corrected, int32_t* batch, int32_t* merge_left, int32_t* merge_right,
                      double* batch_size, int32_t* skipped, double* lost_var) {
    check_alive();
    CacheScope cache_scope(&cache_);
    BMX_HIP(hipSetDevice(device_));
    if (!root_) throw Error(BMX_ERR_ARG, "no finished run to download");
    const int nmerges = B_ - 1;
    if (corrected) {
        // rows back in input batch order (R/fastMNN.R:541-547): batch b starts at the sum of earlier batch sizes
        std::vector<int64_t> start(B_ + 1, 0);
        for (int b = 0; b < B_; ++b) start[b + 1] = start[b] + nrows_[b];
        DevBuf<double> out_cm;
        double* oc = out_cm.reserve((size_t)N_ * d_);
        int r0 = 0;
        for (const Segment& s : root_->origin) {
            transpose_rm_to_cm(stream_, root_->data.p + (size_t)r0 * d_, s.n, d_, oc, (int)N_, (int)start[s.batch - 1]);
            r0 += s.n;
        }
        download_pageable(corrected, oc, (size_t)N_ * d_ * sizeof(double), stream_);
    }
    if (batch) {
        int64_t o = 0;
        for (int b = 0; b < B_; ++b)
            for (int i = 0; i < nrows_[b]; ++i) batch[o++] = b + 1;
    }
    for (int m = 0; m < nmerges; ++m) {
        const MergeRecord& rec = merges_[m];
        if (merge_left)
            for (int j = 0; j < B_; ++j) merge_left[(size_t)m * B_ + j] = j < (int)rec.left_set.size() ? rec.left_set[j] : 0;
        if (merge_right)
            for (int j = 0; j < B_; ++j)
                merge_right[(size_t)m * B_ + j] = j < (int)rec.right_set.size() ? rec.right_set[j] : 0;
        if (batch_size)
            batch_size[m] = rec.batch_size_na || rec.bs_slot < 0 ? std::numeric_limits<double>::quiet_NaN()
                                                                  : scal_host_[rec.bs_slot];
        if (skipped) skipped[m] = rec.skipped ? 1 : 0;
        if (lost_var) {
            for (int b = 0; b < B_; ++b) lost_var[(size_t)b * nmerges + m] = 0.0;  // 1 - var.kept, var.kept starts at 1
            for (size_t s = 0; s < rec.var_batches.size(); ++s) {
                const double oldv = scal_host_[rec.old_slot[s]], newv = scal_host_[rec.new_slot[s]];
                lost_var[(size_t)(rec.var_batches[s] - 1) * nmerges + m] = 1.0 - newv / oldv;
            }
        }
    }
}

namespace {
// node position (1-based) -> output row (1-based), R/fastMNN.R:533-547: a node is a run of whole batches; tab[i] = first
// position of its i-th batch inside the node (tab[ns] = its size), tab[ns + 1 + i] = that batch's first row in the input
// batch order
__global__ void remap_pairs_tab(const int32_t* __restrict__ in, int64_t n, const int32_t* __restrict__ tab, int ns,
                                int32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int pos = in[i] - 1;
    int sgi = 0;
    for (int t = 1; t < ns; ++t) sgi += pos >= tab[t] ? 1 : 0;
    out[i] = tab[ns + 1 + sgi] + (pos - tab[sgi]) + 1;
}
}  // namespace

int64_t Engine::pairs_count(int merge) const {
    check_alive();
    if (!root_) throw Error(BMX_ERR_ARG, "no finished run to download");
    if (merge < 0 || merge >= (int)merges_.size()) throw Error(BMX_ERR_ARG, "merge index out of range");
    return merges_[merge].npairs;
}

void Engine::stage_pairs() {
    // shift every merge's pairs to their nodes' places in the final merged order, then to the input batch order
    // (R/fastMNN.R:533-547): a short table per side, applied on the device; all merges into one block
    pairs_pinned_ = false;
    const int nmerges = (int)merges_.size();
    pairs_off_.assign(nmerges + 1, 0);
    for (int m = 0; m < nmerges; ++m) pairs_off_[m + 1] = pairs_off_[m] + 2 * merges_[m].npairs;
    const int64_t total = pairs_off_[nmerges];
    if (total == 0) return;
    std::vector<int64_t> in_start(B_ + 1, 0);
    for (int b = 0; b < B_; ++b) in_start[b + 1] = in_start[b] + nrows_[b];
    std::vector<size_t> tab_off(nmerges, 0);
    pairs_tab_host_.clear();
    auto fill = [&](const std::vector<int>& set) {
        const int ns = (int)set.size();
        const size_t base = pairs_tab_host_.size();
        pairs_tab_host_.resize(base + 2 * ns + 1);
        int32_t* t = pairs_tab_host_.data() + base;
        int64_t o = 0;
        for (int i = 0; i < ns; ++i) {
            t[i] = (int32_t)o;
            t[ns + 1 + i] = (int32_t)in_start[set[i] - 1];
            o += nrows_[set[i] - 1];
        }
        t[ns] = (int32_t)o;
    };
    for (int m = 0; m < nmerges; ++m) {
        tab_off[m] = pairs_tab_host_.size();
        fill(merges_[m].left_set);
        fill(merges_[m].right_set);
    }
    // (the previous run's lists may still be on their way out of pairs_all_)
    if (pairs_copy_pending_ && pairs_ev_) BMX_HIP(hipStreamWaitEvent(stream_, pairs_ev_, 0));
    pairs_copy_pending_ = false;
    int32_t* dt = pairs_tab_.reserve(pairs_tab_host_.size());
    BMX_HIP(hipMemcpyAsync(dt, pairs_tab_host_.data(), pairs_tab_host_.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
    int32_t* all = pairs_all_.reserve((size_t)total);
    for (int m = 0; m < nmerges; ++m) {
        const MergeRecord& rec = merges_[m];
        const int64_t P = rec.npairs;
        if (P == 0) continue;
        const int nl = (int)rec.left_set.size(), nr = (int)rec.right_set.size();
        hipLaunchKernelGGL(remap_pairs_tab, dim3((unsigned)cdiv(P, 256)), dim3(256), 0, stream_, (const int32_t*)rec.first.p, P,
                           (const int32_t*)(dt + tab_off[m]), nl, all + pairs_off_[m]);
        hipLaunchKernelGGL(remap_pairs_tab, dim3((unsigned)cdiv(P, 256)), dim3(256), 0, stream_, (const int32_t*)rec.second.p, P,
                           (const int32_t*)(dt + tab_off[m] + 2 * nl + 1), nr, all + pairs_off_[m] + P);
    }
    BMX_LAUNCH_CHECK();
    const size_t bytes = (size_t)total * sizeof(int32_t);
    if (bytes <= ((size_t)64 << 20)) {  // (beyond that the lists stay on the device and go out through the staging ring)
        if (bytes > pairs_pin_bytes_) {
            if (pairs_ev_ && pairs_pin_) guarded_event_sync(pairs_ev_);  // (an earlier run's copy into the block that goes away)
            PinnedBlocks::give(PinnedBlocks::Blk{pairs_pin_, pairs_pin_bytes_});
            const PinnedBlocks::Blk b = PinnedBlocks::take(bytes);
            pairs_pin_ = b.p;
            pairs_pin_bytes_ = b.bytes;
        }
        // on the copy stream (a DMA engine), behind the remap kernels: the engine's stream is free for the next run
        if (!pairs_ev_) BMX_HIP(hipEventCreateWithFlags(&pairs_ev_, hipEventDisableTiming));
        if (!pairs_ready_ev_) BMX_HIP(hipEventCreateWithFlags(&pairs_ready_ev_, hipEventDisableTiming));
        if (!copy_stream_) copy_stream_ = StreamPool::take();
        BMX_HIP(hipEventRecord(pairs_ready_ev_, stream_));
        BMX_HIP(hipStreamWaitEvent(copy_stream_, pairs_ready_ev_, 0));
        BMX_HIP(hipMemcpyAsync(pairs_pin_, all, bytes, hipMemcpyDeviceToHost, copy_stream_));
        BMX_HIP(hipEventRecord(pairs_ev_, copy_stream_));
        pairs_pinned_ = true;
        pairs_copy_pending_ = true;
    }
}

void Engine::pairs_into(int merge, int32_t* left, int32_t* right) {
    CacheScope cache_scope(&cache_);
    BMX_HIP(hipSetDevice(device_));
    const int64_t P = pairs_count(merge);
    if (P == 0) return;
    if (pairs_pinned_) {  // the whole run's lists were sent to pinned memory when the run ended: a host copy
        guarded_event_sync(pairs_ev_);
        const int32_t* src = static_cast<const int32_t*>(pairs_pin_) + pairs_off_[merge];
        host_parallel_memcpy(left, src, (size_t)P * sizeof(int32_t));
        host_parallel_memcpy(right, src + P, (size_t)P * sizeof(int32_t));
        return;
    }
    download_pageable(left, pairs_all_.p + pairs_off_[merge], (size_t)P * sizeof(int32_t), stream_);
    download_pageable(right, pairs_all_.p + pairs_off_[merge] + P, (size_t)P * sizeof(int32_t), stream_);
}

void Engine::pairs_all_into(int nmerges, int32_t* const* left, int32_t* const* right, const int64_t* capacity) {
    check_alive();
    if (!root_) throw Error(BMX_ERR_ARG, "no finished run to download");
    if (nmerges != (int)merges_.size()) throw Error(BMX_ERR_ARG, "bmx_engine_pairs_all_into: the last run had another number of merges");
    for (int m = 0; m < nmerges; ++m) {
        if (capacity[m] < merges_[m].npairs) throw Error(BMX_ERR_ARG, "bmx_engine_pairs_all_into: an array is too short");
        if (merges_[m].npairs > 0 && (!left[m] || !right[m])) throw Error(BMX_ERR_ARG, "bmx_engine_pairs_all_into: null array");
    }
    if (!pairs_pinned_) {  // (lists beyond the pinned block's bound: through the staging ring, one by one)
        for (int m = 0; m < nmerges; ++m) pairs_into(m, left[m], right[m]);
        return;
    }
    CacheScope cache_scope(&cache_);
    BMX_HIP(hipSetDevice(device_));
    guarded_event_sync(pairs_ev_);
    // the whole run's lists sit in pinned memory: ONE job of the host threads over all of them, in pieces of 64 KB (the
    // first touch of the caller's fresh pages spreads over the threads like the bytes do)
    struct Piece {
        char* dst;
        const char* src;
        size_t bytes;
    };
    constexpr size_t kPiece = (size_t)64 << 10;
    // pieces in round-robin order over the 2 x nmerges arrays: threads that take consecutive pieces then fault pages of
    // DIFFERENT arrays (consecutive pieces of one ~2 MB array share a page-table page and its lock: measured slower than
    // the one-array-at-a-time calls this replaces)
    std::vector<Piece> pieces;
    size_t longest = 0;
    for (int m = 0; m < nmerges; ++m) longest = std::max(longest, (size_t)merges_[m].npairs * sizeof(int32_t));
    for (size_t o = 0; o < longest; o += kPiece)
        for (int m = 0; m < nmerges; ++m) {
            const size_t bytes = (size_t)merges_[m].npairs * sizeof(int32_t);
            if (o >= bytes) continue;
            const char* src = reinterpret_cast<const char*>(static_cast<const int32_t*>(pairs_pin_) + pairs_off_[m]);
            for (int side = 0; side < 2; ++side) {
                char* dst = reinterpret_cast<char*>(side == 0 ? left[m] : right[m]);
                pieces.push_back({dst + o, src + side * bytes + o, std::min(kPiece, bytes - o)});
            }
        }
    HostPool::get().parallel_for(pieces.size(), [&](size_t i) { std::memcpy(pieces[i].dst, pieces[i].src, pieces[i].bytes); });
}

void Engine::pairs(int merge, int32_t** left, int32_t** right, int64_t* npairs) {
    const int64_t P = pairs_count(merge);
    int32_t* L = (int32_t*)std::malloc(std::max<size_t>(1, (size_t)P) * sizeof(int32_t));
    int32_t* R = (int32_t*)std::malloc(std::max<size_t>(1, (size_t)P) * sizeof(int32_t));
    if (!L || !R) {
        std::free(L);
        std::free(R);
        throw std::bad_alloc();
    }
    try {
        pairs_into(merge, L, R);
    } catch (...) {
        std::free(L);
        std::free(R);
        throw;
    }
    *left = L;
    *right = R;
    *npairs = P;
}

void Engine::snapshot(double* left_rm, double* right_rm, int64_t* nl, int64_t* nr) {
    CacheScope cache_scope(&cache_);
    BMX_HIP(hipSetDevice(device_));
    if (snap_merge_ < 0 || !root_ || !snap_l_.p) throw Error(BMX_ERR_ARG, "no snapshot was taken");
    if (nl) *nl = snap_nl_;
    if (nr) *nr = snap_nr_;
    if (left_rm)
        BMX_HIP(hipMemcpyAsync(left_rm, snap_l_.p, (size_t)snap_nl_ * d_ * sizeof(double), hipMemcpyDeviceToHost, stream_));
    if (right_rm)
        BMX_HIP(hipMemcpyAsync(right_rm, snap_r_.p, (size_t)snap_nr_ * d_ * sizeof(double), hipMemcpyDeviceToHost, stream_));
    BMX_HIP(hipStreamSynchronize(stream_));
}

void Engine::snapshot_var_adj(double* left_rm, double* right_rm, double* corr_rm, double* scaling, int32_t* r1,
                              int32_t* r2, int64_t* sizes4) {
    CacheScope cache_scope(&cache_);
    BMX_HIP(hipSetDevice(device_));
    if (snap_merge_ < 0 || !root_ || !snap_as_.p) throw Error(BMX_ERR_ARG, "no snapshot of a variance adjustment was taken");
    if (sizes4) {
        sizes4[0] = snap_anl_;
        sizes4[1] = snap_anr_;
        sizes4[2] = snap_ar1_;
        sizes4[3] = snap_ar2_;
    }
    auto out = [&](void* dst, const void* src, size_t bytes) {
        if (dst && bytes) BMX_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream_));
    };
    out(left_rm, snap_al_.p, (size_t)snap_anl_ * d_ * sizeof(double));
    out(right_rm, snap_ar_.p, (size_t)snap_anr_ * d_ * sizeof(double));
    out(corr_rm, snap_ac_.p, (size_t)snap_anr_ * d_ * sizeof(double));
    out(scaling, snap_as_.p, (size_t)snap_anr_ * sizeof(double));
    out(r1, snap_ai1_.p, (size_t)snap_ar1_ * sizeof(int32_t));
    out(r2, snap_ai2_.p, (size_t)snap_ar2_ * sizeof(int32_t));
    BMX_HIP(hipStreamSynchronize(stream_));
}

void Engine::var_adj_tally(int merge, int64_t* out3) const {
    if (merge < 0 || merge >= (int)merges_.size()) throw Error(BMX_ERR_ARG, "merge index out of range");
    for (int i = 0; i < 3; ++i) out3[i] = merges_[merge].asv_tally[i];
}

void Engine::var_adj_strict_cells(int merge, int64_t* cells) const {
    if (merge < 0 || merge >= (int)merges_.size()) throw Error(BMX_ERR_ARG, "merge index out of range");
    *cells = merges_[merge].asv_strict;
}

void Engine::snapshot_var_adj_modes(unsigned char* dst, int64_t n) const {
    for (int64_t i = 0; i < n; ++i) dst[i] = (size_t)i < snap_modes_.size() ? snap_modes_[(size_t)i] : 255;
}

void Engine::merge_stats(int merge, int64_t* out6) const {
    if (merge < 0 || merge >= (int)merges_.size()) throw Error(BMX_ERR_ARG, "merge index out of range");
    for (int i = 0; i < 6; ++i) out6[i] = merges_[merge].stats[i];
}

Engine::Section::Section(Engine* eng) : e(eng) {
    if (e->knn_ws_.profile) {
        ev = e->knn_ws_.next_events(3);
        (void)hipEventRecord(ev.first, e->stream_);
    }
}
Engine::Section::~Section() {
    if (ev.second) (void)hipEventRecord(ev.second, e->stream_);
}

void Engine::profile_detail(double* out10) {
    for (int i = 0; i < 10; ++i) out10[i] = 0.0;
    for (size_t i = 0; i < knn_ws_.events_used; ++i) {
        float t = 0.f;
        BMX_HIP(hipEventElapsedTime(&t, knn_ws_.events[i].first, knn_ws_.events[i].second));
        switch (knn_ws_.event_tag[i]) {
            case 1: out10[0] += t; out10[1] += 1; break;
            case 2: out10[2] += t; out10[3] += 1; break;
            case 0: out10[4] += t; out10[5] += 1; break;
            case 4: break;  // (adjust_shift_variance: profile_var_adj)
            default: out10[6] += t; break;
        }
    }
    out10[7] = (double)fallbacks_;
    out10[8] = (double)knn_ws_.tier2_total;
    out10[9] = (double)optimistic_retries_;
}

void Engine::profile_var_adj(double* out3) {
    out3[0] = out3[1] = 0.0;
    for (size_t i = 0; i < knn_ws_.events_used; ++i) {
        if (knn_ws_.event_tag[i] != 4) continue;
        float t = 0.f;
        BMX_HIP(hipEventElapsedTime(&t, knn_ws_.events[i].first, knn_ws_.events[i].second));
        out3[0] += t;
        out3[1] += 1;
    }
    out3[2] = asv_pairs_;
}

void Engine::profile(double* topk_ms, int64_t* launches, int64_t* fallbacks) {
    double ms = 0.0;
    int64_t n = 0;
    for (size_t i = 0; i < knn_ws_.events_used; ++i) {
        if (knn_ws_.event_tag[i] >= 3) continue;  // a streaming section / a variance adjustment, not a candidate-pass launch
        float t = 0.f;
        BMX_HIP(hipEventElapsedTime(&t, knn_ws_.events[i].first, knn_ws_.events[i].second));
        ms += t;
        ++n;
    }
    if (topk_ms) *topk_ms = ms;
    if (launches) *launches = n;
    if (fallbacks) *fallbacks = fallbacks_;
}

}  // namespace bmx
