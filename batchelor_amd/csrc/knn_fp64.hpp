// FP64 device pieces that more than one unit of the exact kNN uses (knn_refine.hip, knn_exact.hip, knn_large_k.hip): the
// reference's squared distance, the (distance, position) order, and the block-wide sort in that order.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bmx {

__device__ __forceinline__ double exact_d2(const double* __restrict__ a, const double* __restrict__ b, int d) {
    double s = 0.0;
    int c = 0;
    if ((d & 1) == 0) {  // rows of an even number of doubles are 16-byte aligned: half as many load instructions
        typedef double d2 __attribute__((ext_vector_type(2)));
        const d2* a2 = reinterpret_cast<const d2*>(a);
        const d2* b2 = reinterpret_cast<const d2*>(b);
        // eight 16-byte pieces of the (randomly placed) row b in flight at a time; the sum itself stays strictly left
        // to right (compiled with -ffp-contract=off: the reference's sum, bit for bit)
        for (; c + 16 <= d; c += 16) {
            d2 y[8], x[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) y[i] = b2[(c >> 1) + i];
#pragma unroll
            for (int i = 0; i < 8; ++i) x[i] = a2[(c >> 1) + i];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const double t0 = x[i][0] - y[i][0];
                s += t0 * t0;
                const double t1 = x[i][1] - y[i][1];
                s += t1 * t1;
            }
        }
        for (; c < d; c += 2) {
            const d2 x = a2[c >> 1], y = b2[c >> 1];
            const double t0 = x[0] - y[0];
            s += t0 * t0;
            const double t1 = x[1] - y[1];
            s += t1 * t1;
        }
        return s;
    }
    for (; c < d; ++c) {
        const double t = a[c] - b[c];
        s += t * t;
    }
    return s;
}

__device__ __forceinline__ bool key_less(double da, int ia, double db, int ib) {
    return da < db || (da == db && ia < ib);
}

// Block-wide bitonic sort of np2 (a power of two) pairs (distance, position) in the LDS, ascending by key_less; T threads,
// all of which call it.  A thread takes PAIRS (t < np2 / 2): every thread that is inside the bound compares in every step.
// The caller has written the arrays and synchronised; they are sorted and visible to the block on return.  Keys are unique
// apart from the padding entries (+inf, 0x7fffffff), which are identical: the sorted arrays do not depend on the network.
template <int T>
__device__ __forceinline__ void block_bitonic_sort(double* sd, int* si, int np2) {
    for (int size = 2; size <= np2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < (np2 >> 1); t += T) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const double a = sd[i], b = sd[j];
                const int ai = si[i], bi = si[j];
                if (key_less(b, bi, a, ai) == ((i & size) == 0)) {
                    sd[i] = b;
                    sd[j] = a;
                    si[i] = bi;
                    si[j] = ai;
                }
            }
            __syncthreads();
        }
}

}  // namespace bmx
