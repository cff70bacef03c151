// "Ordered references" of the fp16 candidate tier (knn.hip: candidate_pass): the reference image is written in ascending order
// of a key -- the squared distance of a reference row from the centre of the queries --, so that the rows most queries find
// their neighbours among are swept first: the threshold sample (image rows [0, S)) then holds the best rows instead of
// arbitrary ones, and the running thresholds of the full pass are nearly final after its first few per cent.  Any order of the
// rows is valid for the pass; the re-rank translates image rows back to reference positions (knn_refine.hip: img_pos).
//
// The order is a stable counting sort over ORDER_BUCKETS equal-width buckets between the smallest and the largest key: buckets
// ascending, reference position order kept inside a bucket (an exact sort gained nothing over it on the CPU replay,
// scripts/ref_order_replay.py).  This header is the pure part -- the bucket of a key, the degenerate case, the offsets, and
// the whole permutation as the host computes it -- with no HIP in it: tests/host/knn_ref_order_host.cpp checks it with a
// plain C++ compiler.  The kernels of knn_order.hip share key_buckets and key_bucket with it, i.e. which bucket a row goes to;
// bucket_offsets and order_positions are the host's statement of the sort, the device has scans of its own, so the device
// permutation is pinned by the GPU tests (tests/test_gpu_knn_ref_order.py: every row its own neighbour, ties by position).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BMX_ORDER_HD __host__ __device__ __forceinline__
#else
#define BMX_ORDER_HD inline
#endif

namespace bmx {
namespace order {

constexpr int ORDER_BUCKETS = 256;
constexpr int ORDER_UNIT = 1024;  // reference positions a wave of the device sort counts and places: one row of its histogram

// the buckets of a search: bucket(key) = floor((key - lo) * scale), clamped.  scale == 0: one bucket (all keys equal, or a
// range that is not a positive finite number: the order is then the identity)
struct KeyBuckets {
    float lo, scale;
};

BMX_ORDER_HD KeyBuckets key_buckets(float kmin, float kmax) {
    const float w = kmax - kmin;
    if (!(w > 0.f) || !(w <= 3.0e38f)) return KeyBuckets{kmin, 0.f};
    const float scale = (float)ORDER_BUCKETS / w;
    if (!(scale <= 3.0e38f)) return KeyBuckets{kmin, 0.f};
    return KeyBuckets{kmin, scale};
}

BMX_ORDER_HD int key_bucket(const KeyBuckets& kb, float key) {
    if (kb.scale == 0.f) return 0;
    const float t = (key - kb.lo) * kb.scale;
    if (!(t > 0.f)) return 0;  // (a NaN key too)
    if (t >= (float)(ORDER_BUCKETS - 1)) return ORDER_BUCKETS - 1;
    return (int)t;
}

// first image row of every bucket from the buckets' sizes
inline void bucket_offsets(const uint32_t* counts, uint32_t* offsets) {
    uint32_t run = 0;
    for (int b = 0; b < ORDER_BUCKETS; ++b) {
        offsets[b] = run;
        run += counts[b];
    }
}

// The permutation as a whole, the way the host computes it: img_pos[i] = reference position of image row i, for the keys of
// the nr reference positions; image rows [nr, nr_pad) are padding and hold themselves.  Returns the number of buckets in use.
inline int order_positions(const float* key, int nr, int nr_pad, int32_t* img_pos) {
    float kmin = 0.f, kmax = 0.f;
    for (int i = 0; i < nr; ++i) {
        if (i == 0 || key[i] < kmin) kmin = key[i];
        if (i == 0 || key[i] > kmax) kmax = key[i];
    }
    const KeyBuckets kb = key_buckets(kmin, kmax);
    uint32_t counts[ORDER_BUCKETS] = {0}, offsets[ORDER_BUCKETS];
    for (int i = 0; i < nr; ++i) ++counts[key_bucket(kb, key[i])];
    bucket_offsets(counts, offsets);
    int used = 0;
    for (int b = 0; b < ORDER_BUCKETS; ++b) used += counts[b] > 0;
    for (int i = 0; i < nr; ++i) img_pos[offsets[key_bucket(kb, key[i])]++] = i;
    for (int i = nr; i < nr_pad; ++i) img_pos[i] = i;
    return used;
}

}  // namespace order
}  // namespace bmx
