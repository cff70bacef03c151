// The summation orders of the dense per-gene passes, stated once (device only).  Every handle promises that any blocking
// of the upload and any run give the same bits; that rests on three rules, and this header is where they live:
//   1. within a chunk, the terms are added in list order into ONE accumulator (ordered_walk4);
//   2. the chunks' partial sums are added in ascending chunk order (fold_ascending), the chunk edges being fixed positions
//      of the list, never of the upload blocks;
//   3. no floating-point atomics: a sum has one writer.  Where a workgroup's threads must meet, they meet in a tree of
//      fixed shape (block_tree_sum).
// coef_partial_kernel (linear_correct.hip: one load in flight by design) and pair_pass_kernel (delta_variance.hip: its
// kept-left-cell branches make it a different loop) keep their own loops; so does sum_partial_kernel (linear_correct.hip),
// whose pow forms were 3 % slower on ordered_walk4 (MEASUREMENTS.md).
#pragma once
#include <hip/hip_runtime.h>

namespace bmx {

// cosineNorm's pmax(1e-8, .) (R/cosineNorm.R:80)
__host__ __device__ __forceinline__ double cos_clamp(double v) { return v < 1e-8 ? 1e-8 : v; }

// The positions [b, e) in order, four loads in flight: load(i) .. load(i + 3) are all issued before the first add, the
// adds follow in that order, and the one to three positions left over go one by one.  What load returns (a double, a
// double2, a small struct) is what add takes; a flag computed in load rides along.  Arithmetic that branches or waits for
// the value (pow, a division) belongs in add: inside load it would stand between the loads.
template <class I, class Load, class Add>
__device__ __forceinline__ void ordered_walk4(I b, I e, Load&& load, Add&& add) {
    I i = b;
    for (; i + 4 <= e; i += 4) {
        const auto v0 = load(i), v1 = load(i + 1), v2 = load(i + 2), v3 = load(i + 3);
        add(v0);
        add(v1);
        add(v2);
        add(v3);
    }
    for (; i < e; ++i) add(load(i));
}

// seed + at(f) + at(f + 1) + ... + at(l - 1), in that order.  The seed is explicit because it shows in the bits: a fold
// that starts from the first partial (seed = at(f), f + 1) keeps a sum of -0.0, one that starts from 0.0 gives +0.0 and is
// defined for an empty range.  UNROLL > 0: the loop carries `#pragma unroll UNROLL`.
template <int UNROLL = 0, class T, class At>
__device__ __forceinline__ T fold_ascending(T seed, int f, int l, At&& at) {
    T s = seed;
    if constexpr (UNROLL > 0) {
#pragma unroll UNROLL
        for (int ch = f; ch < l; ++ch) s += at(ch);
    } else {
        for (int ch = f; ch < l; ++ch) s += at(ch);
    }
    return s;
}

// The sum of every thread's v over a workgroup of T threads (a power of two) by a halving tree through red [T]: thread t
// adds red[t + k] for k = T / 2, T / 4, ..., 1.  Every thread gets the sum; red is free again on return.
template <int T>
__device__ __forceinline__ double block_tree_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int k = T / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

}  // namespace bmx
