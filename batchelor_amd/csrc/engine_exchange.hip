// Merge engine, the ranks and what they exchange: the shard layout, the transports (callback, RCCL, the one-GPU emulation),
// the all-gather itself and auto-merge's dealt counts.
#include "engine_internal.hpp"
#include "rccl_dyn.hpp"

#include <cstring>

namespace bmx {

// The one place the sharded search's layout is decided (the engine and the host-side tests both go through it): n query
// rows are cut into `world` padded slices of rows_per_rank rows; rank r owns rows [r * rows_per_rank, ...) clipped to n,
// and the list buffers hold world * rows_per_rank rows so that the all-gather is in place with equal counts.
int64_t bmx_shard_rows_per_rank(int64_t n, int world) { return world > 0 ? (n + world - 1) / world : n; }

void bmx_shard_range_impl(int64_t n, int rank, int world, int64_t* begin, int64_t* end) {
    const int64_t per = bmx_shard_rows_per_rank(n, world);
    const int64_t b = std::min<int64_t>(n, per * rank);
    *begin = b;
    *end = std::min<int64_t>(n, b + per);
}

void Engine::set_shard(int rank, int world, bmx_allgather_fn fn, void* ctx) {
    if (emu_mode_ != 0) throw Error(BMX_ERR_ARG, "the engine is emulating a rank (bmx_engine_emulate): switch that off first");
    if (world < 1 || rank < 0 || rank >= world) throw Error(BMX_ERR_ARG, "invalid rank / world size");
    if (world > 1 && !fn) throw Error(BMX_ERR_ARG, "a multi-rank engine needs an all-gather callback");
    if (comm_ && rccl::api().CommDestroy) {  // a callback replaces an RCCL communicator
        if (stream_) (void)hipStreamSynchronize(stream_);
        (void)rccl::api().CommDestroy(comm_);
        comm_ = nullptr;
    }
    rank_ = rank;
    world_ = world;
    gather_fn_ = fn;
    gather_ctx_ = ctx;
}

void Engine::init_rccl(int rank, int world, const void* unique_id) {
    CacheScope cache_scope(&cache_);
    BMX_HIP(hipSetDevice(device_));
    if (emu_mode_ != 0) throw Error(BMX_ERR_ARG, "the engine is emulating a rank (bmx_engine_emulate): switch that off first");
    if (world < 1 || rank < 0 || rank >= world) throw Error(BMX_ERR_ARG, "invalid rank / world size");
    if (!unique_id) throw Error(BMX_ERR_ARG, "null RCCL unique id");
    rccl::Api& a = rccl::api();
    if (!a.ready()) throw Error(BMX_ERR_EXCHANGE, "RCCL is not loaded (bmx_rccl_load)");
    if (comm_) {
        BMX_HIP(hipStreamSynchronize(stream_));
        (void)a.CommDestroy(comm_);
        comm_ = nullptr;
    }
    rccl::UniqueId id;
    std::memcpy(id.internal, unique_id, sizeof(id.internal));
    const int rc = a.CommInitRank(&comm_, world, id, rank);
    if (rc != 0) {
        comm_ = nullptr;
        throw Error(BMX_ERR_EXCHANGE, std::string("ncclCommInitRank failed: ") +
                                          (a.GetErrorString ? a.GetErrorString(rc) : std::to_string(rc).c_str()));
    }
    rank_ = rank;
    world_ = world;
    gather_fn_ = nullptr;
    gather_ctx_ = nullptr;
}

// One rank of an N-rank run measured on ONE GPU (bmx_engine_emulate, bench.py --emulate-world): a single-rank run first
// RECORDS what every exchange would have gathered -- the complete array, which a single rank computes itself --, then the
// engine runs as rank r of N: every search covers its slice of the query rows only, every kernel that a multi-rank run
// replicates runs in full, and an exchange fills the OTHER ranks' slices from the recording (a device copy in place of the
// all-gather: what is timed is the rank's own work; the collective's time is modelled beside it from its byte count).
// The results are bit-identical to the recorded run's, so the sequence and the sizes of the exchanges are the same.
void Engine::emulate(int mode, int rank, int world) {
    if (mode < 0 || mode > 2) throw Error(BMX_ERR_ARG, "emulation mode: 0 off, 1 record, 2 replay");
    if (mode == 2 && (world < 1 || rank < 0 || rank >= world)) throw Error(BMX_ERR_ARG, "invalid rank / world size");
    if (comm_ || gather_fn_) throw Error(BMX_ERR_ARG, "emulation is for an engine without a transport");
    if (stream_) BMX_HIP(hipStreamSynchronize(stream_));
    emu_mode_ = mode;
    if (mode == 1) {
        emu_rec_.clear();
        rank_ = 0;
        world_ = 1;
    } else if (mode == 2) {
        rank_ = rank;
        world_ = world;
    } else {
        emu_rec_.clear();
        rank_ = 0;
        world_ = 1;
    }
}

bool Engine::transport_in_play() const {
    return world_ > 1 || emu_mode_ == 1 || (dev_knobs().exchange_always != 0 && (comm_ || gather_fn_));
}

// the other ranks' slices of an emulated exchange in ONE launch: bytes [0, lo) and [hi, total) of the recording (zeros when
// there is none: the optimistic-search flags), 16 bytes per thread where the pieces allow
__global__ void emu_fill_kernel(char* __restrict__ dst, const char* __restrict__ src, int64_t lo, int64_t hi, int64_t total) {
    const int64_t n16 = (lo >> 4) + ((total - hi + 15) >> 4);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t o = i < (lo >> 4) ? i << 4 : hi + ((i - (lo >> 4)) << 4);
        if (o + 16 <= total && ((reinterpret_cast<uintptr_t>(dst + o) | reinterpret_cast<uintptr_t>(src + o)) & 15) == 0) {
            *reinterpret_cast<int4*>(dst + o) = src ? *reinterpret_cast<const int4*>(src + o) : int4{0, 0, 0, 0};
        } else {
            for (int64_t b = o; b < o + 16 && b < total; ++b) dst[b] = src ? src[b] : 0;
        }
    }
    // (the ragged end of the first piece)
    if (blockIdx.x == 0 && threadIdx.x < (lo & 15)) {
        const int64_t b = (lo & ~(int64_t)15) + threadIdx.x;
        dst[b] = src ? src[b] : 0;
    }
}

void Engine::exchange(void* buf, int64_t bytes_per_rank, bool flags_only) {
    if (emu_mode_ == 1) {  // record: this (single) rank's slice is the whole array
        if (flags_only) return;
        if (emu_next_ >= emu_rec_.size()) emu_rec_.emplace_back();
        auto& r = emu_rec_[emu_next_++];
        r.second = bytes_per_rank;
        BMX_HIP(hipMemcpyAsync(r.first.reserve((size_t)std::max<int64_t>(bytes_per_rank, 1)), buf, (size_t)bytes_per_rank,
                               hipMemcpyDeviceToDevice, stream_));
        return;
    }
    if (emu_mode_ == 2) {
        ++xchg_calls_;
        xchg_bytes_ += bytes_per_rank * world_;
        char* base = static_cast<char*>(buf);
        const int64_t mine = (int64_t)rank_ * bytes_per_rank;
        if (flags_only) {  // the other ranks' optimistic-search flags: all clear (the recorded run went through)
            const int64_t total = (int64_t)world_ * bytes_per_rank;
            hipLaunchKernelGGL(emu_fill_kernel, dim3(1), dim3(256), 0, stream_, base, (const char*)nullptr, mine,
                               mine + bytes_per_rank, total);
            BMX_LAUNCH_CHECK();
            return;
        }
        if (emu_next_ >= emu_rec_.size()) throw Error(BMX_ERR_ARG, "emulated run: more exchanges than the recorded run made");
        const auto& r = emu_rec_[emu_next_++];
        // (the recording must be of THIS job: the same sequence of exchanges, each no larger than this call's padded array)
        if (r.second > (int64_t)world_ * bytes_per_rank)
            throw Error(BMX_ERR_ARG, "emulated run: an exchange of the recorded run is larger than this run's (other inputs, "
                                     "parameters or tree than the recording?)");
        // bytes [0, mine) and [mine + per, total) of the recording, where they exist
        const int64_t total = r.second, lo = std::min(mine, total), hi = std::min(mine + bytes_per_rank, total);
        const int64_t n16 = (lo >> 4) + ((total - hi + 15) >> 4);
        if (n16 > 0 || (lo & 15)) {
            hipLaunchKernelGGL(emu_fill_kernel, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(2048, (n16 + 255) / 256))),
                               dim3(256), 0, stream_, base, (const char*)r.first.p, lo, hi, total);
            BMX_LAUNCH_CHECK();
        }
        return;
    }
    // testing hook (bmx_dev_set "exchange_always"): a single rank goes through its transport too (an all-gather of one)
    const bool always = dev_knobs().exchange_always != 0;
    if (world_ == 1 && !(always && (comm_ || gather_fn_))) return;
    ++xchg_calls_;
    xchg_bytes_ += bytes_per_rank * world_;
    if (comm_) {
        // in place (send buffer = this rank's slice of the receive buffer), ordered on the engine's stream: no host
        // synchronisation, the next kernel simply queues behind the collective
        char* base = static_cast<char*>(buf);
        const int rc = rccl::api().AllGather(base + (int64_t)rank_ * bytes_per_rank, base, (size_t)bytes_per_rank,
                                             /* ncclUint8 */ 1, comm_, stream_);
        if (rc != 0)
            throw Error(BMX_ERR_EXCHANGE, std::string("ncclAllGather failed: ") +
                                              (rccl::api().GetErrorString ? rccl::api().GetErrorString(rc) : "?"));
        return;
    }
    BMX_HIP(hipStreamSynchronize(stream_));
    const int rc = gather_fn_(gather_ctx_, buf, bytes_per_rank);
    if (rc != 0) throw Error(BMX_ERR_EXCHANGE, "the all-gather callback failed with code " + std::to_string(rc));
}

// counts[t] is known on rank t % world only (0 elsewhere): every rank gets them all (an all-gather of the padded slices)
std::vector<int32_t> Engine::gather_counts(const std::vector<int32_t>& mine) {
    if (emu_mode_ == 2) throw Error(BMX_ERR_ARG, "the one-GPU emulation of a rank covers predefined merge trees, not auto-merge's dealt searches");
    if (world_ == 1) return mine;
    const int n = (int)mine.size();
    const int per = (n + world_ - 1) / world_ + 1;  // (+ 1: "one of my searches could not be completed optimistically")
    std::vector<int32_t> slice((size_t)per * world_, 0);
    for (int t = rank_; t < n; t += world_) slice[(size_t)rank_ * per + t / world_] = mine[t];
    slice[(size_t)rank_ * per + per - 1] = solo_flag_ ? 1 : 0;
    solo_flag_ = false;
    int32_t* dev = count_xchg_.reserve((size_t)per * world_);
    BMX_HIP(hipMemcpyAsync(dev, slice.data(), slice.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
    BMX_HIP(hipStreamSynchronize(stream_));
    exchange(dev, (int64_t)per * (int64_t)sizeof(int32_t));
    BMX_HIP(hipMemcpyAsync(slice.data(), dev, slice.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
    wait();
    for (int r = 0; r < world_; ++r)
        if (slice[(size_t)r * per + per - 1] != 0) throw OptimisticRetry();  // every rank sees the same slices: all restart here
    std::vector<int32_t> out((size_t)n);
    for (int t = 0; t < n; ++t) out[t] = slice[(size_t)(t % world_) * per + t / world_];
    return out;
}

std::vector<int32_t> Engine::solo_counts(int n, const std::function<int(int)>& count) {
    std::vector<int32_t> mine((size_t)n, 0);
    for (int t = 0; t < n; ++t) {
        if (t % world_ != rank_) continue;
        SoloRank solo(this);  // an unsharded search on this rank alone
        mine[t] = count(t);
    }
    return gather_counts(mine);
}

}  // namespace bmx
