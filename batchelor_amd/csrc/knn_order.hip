// The device side of the ordered references (knn_order.hpp has what they are and the pure part): from the keys that
// knn_prep_f16_norms left, the two index arrays of the search's reference image,
//   img_src[i]  the row of X that image row i is made from (composed with ref_rows where the caller gave one),
//   img_pos[i]  that row's reference position: what the caller's indices mean,
// by a stable counting sort in three launches.  A wave owns ORDER_UNIT consecutive reference positions:
//   ref_order_count   the wave's histogram over the buckets, hist[bucket][unit];
//   ref_order_scan    a workgroup per bucket: exclusive prefix over the units in place, the bucket's size;
//   ref_order_place   the wave's first image row per bucket = buckets before + units before; its rows are placed 64 at a
//                     time, a row behind the lower lanes of its bucket (ballots), so position order is kept.
// Every destination is a prefix sum: the image is the same however the hardware schedules the waves.
#include "knn_internal.hpp"
#include "knn_order.hpp"

namespace bmx {
namespace {

using namespace order;

// smallest and largest key of the search: the prep kernel's waves left them in the second 64-bit word of the 64 norm slots
// (low half: the largest bit pattern, high half: the largest complement; keys are >= 0, so patterns order like values).
// Called by one whole wave; every lane returns the buckets.
__device__ __forceinline__ KeyBuckets fold_key_range(const unsigned long long* __restrict__ slots) {
    const unsigned long long w = slots[(size_t)(threadIdx.x & 63) * 16 + 1];
    uint32_t mx = (uint32_t)w, mn = (uint32_t)(w >> 32);
    for (int o = 1; o < 64; o <<= 1) {
        mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
        mn = max(mn, (uint32_t)__shfl_xor((int)mn, o));
    }
    return key_buckets(__uint_as_float(~mn), __uint_as_float(mx));
}

__global__ __launch_bounds__(256) void ref_order_count(const float* __restrict__ key, int nr, int nunits,
                                                       const unsigned long long* __restrict__ slots,
                                                       uint32_t* __restrict__ hist) {
    __shared__ uint32_t cnt[4][ORDER_BUCKETS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int unit = blockIdx.x * 4 + w;
    const KeyBuckets kb = fold_key_range(slots);
    for (int b = lane; b < ORDER_BUCKETS; b += 64) cnt[w][b] = 0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (unit >= nunits) return;
    for (int it = 0; it < ORDER_UNIT / 64; ++it) {
        const int i = unit * ORDER_UNIT + it * 64 + lane;
        if (i < nr) atomicAdd(&cnt[w][key_bucket(kb, key[i])], 1u);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    for (int b = lane; b < ORDER_BUCKETS; b += 64) hist[(size_t)b * nunits + unit] = cnt[w][b];
}

// bucket blockIdx.x: hist[bucket][0 .. nunits) becomes its exclusive prefix, total[bucket] the sum
__global__ __launch_bounds__(256) void ref_order_scan(uint32_t* __restrict__ hist, int nunits, uint32_t* __restrict__ total) {
    __shared__ uint32_t wsum[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t* row = hist + (size_t)blockIdx.x * nunits;
    uint32_t carry = 0;
    for (int u0 = 0; u0 < nunits; u0 += 256) {
        const int u = u0 + threadIdx.x;
        const uint32_t mine = u < nunits ? row[u] : 0u;
        uint32_t inc = mine;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)inc, o);
            if (lane >= o) inc += t;
        }
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        uint32_t woff = 0, bsum = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t t = wsum[i];
            bsum += t;
            woff += i < w ? t : 0u;
        }
        if (u < nunits) row[u] = carry + woff + (inc - mine);
        carry += bsum;
        __syncthreads();
    }
    if (threadIdx.x == 0) total[blockIdx.x] = carry;
}

__global__ __launch_bounds__(256) void ref_order_place(const float* __restrict__ key, int nr, int nunits,
                                                       const unsigned long long* __restrict__ slots,
                                                       const uint32_t* __restrict__ hist, const uint32_t* __restrict__ total,
                                                       const int32_t* __restrict__ ref_rows, int32_t* __restrict__ img_src,
                                                       int32_t* __restrict__ img_pos) {
    __shared__ uint32_t next[4][ORDER_BUCKETS];  // per wave and bucket: the image row its next position goes to
    __shared__ uint32_t base[ORDER_BUCKETS];
    __shared__ uint32_t wsum[4];
    static_assert(ORDER_BUCKETS == 256, "a thread of the 256 per bucket: total[threadIdx.x], base[threadIdx.x]");
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int unit = blockIdx.x * 4 + w;
    const KeyBuckets kb = fold_key_range(slots);
    {  // first image row of every bucket: exclusive prefix of the 256 sizes, thread b its bucket's
        const uint32_t mine = total[threadIdx.x];
        uint32_t inc = mine;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)inc, o);
            if (lane >= o) inc += t;
        }
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        uint32_t woff = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) woff += i < w ? wsum[i] : 0u;
        base[threadIdx.x] = woff + (inc - mine);
        __syncthreads();
    }
    if (unit >= nunits) return;
    for (int b = lane; b < ORDER_BUCKETS; b += 64) next[w][b] = base[b] + hist[(size_t)b * nunits + unit];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    for (int it = 0; it < ORDER_UNIT / 64; ++it) {
        const int i = unit * ORDER_UNIT + it * 64 + lane;
        const bool live = i < nr;
        const int b = live ? key_bucket(kb, key[i]) : 0;
        // the lanes of this lane's bucket
        unsigned long long peers = __builtin_amdgcn_ballot_w64(live);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const unsigned long long has = __builtin_amdgcn_ballot_w64(((b >> bit) & 1) != 0);
            peers &= ((b >> bit) & 1) ? has : ~has;
        }
        const int rank = __builtin_popcountll(peers & ((1ull << lane) - 1ull));
        if (live) {
            const uint32_t dst = next[w][b] + (uint32_t)rank;
            img_src[dst] = ref_rows ? ref_rows[i] : i;
            img_pos[dst] = i;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (live && rank == 0) next[w][b] += (uint32_t)__builtin_popcountll(peers);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
}

}  // namespace

size_t ref_order_scratch_words(int nr) { return (size_t)ORDER_BUCKETS * cdiv(nr, ORDER_UNIT) + ORDER_BUCKETS; }

void ref_order_build(hipStream_t stream, const float* key, int nr, const int32_t* ref_rows, const unsigned long long* slots,
                     uint32_t* scratch, int32_t* img_src, int32_t* img_pos) {
    const int nunits = cdiv(nr, ORDER_UNIT);
    uint32_t* hist = scratch;
    uint32_t* total = scratch + (size_t)ORDER_BUCKETS * nunits;
    hipLaunchKernelGGL(ref_order_count, dim3(cdiv(nunits, 4)), dim3(256), 0, stream, key, nr, nunits, slots, hist);
    BMX_LAUNCH_CHECK();
    hipLaunchKernelGGL(ref_order_scan, dim3(ORDER_BUCKETS), dim3(256), 0, stream, hist, nunits, total);
    BMX_LAUNCH_CHECK();
    hipLaunchKernelGGL(ref_order_place, dim3(cdiv(nunits, 4)), dim3(256), 0, stream, key, nr, nunits, slots,
                       (const uint32_t*)hist, (const uint32_t*)total, ref_rows, img_src, img_pos);
    BMX_LAUNCH_CHECK();
}

}  // namespace bmx
