// What the two candidate tiers of the exact kNN (knn_f16.hip, knn_bf16.hip) share on the device: the decode of a work item,
// the relaxed LDS load the hand-over words are read with, the lane position inside a ballot, and the cycle stamps of the
// developer build (make STAMPS=1).  Included by those two units only.
#pragma once
#include "knn_internal.hpp"

namespace bmx {
namespace {

// Work items in launch order: first the query blocks that sweep the whole reference as one range (best selection
// efficiency), then the remaining query blocks split into `nranges` ranges each (short items that fill the last round of
// workgroups evenly), range-major: the workgroups in flight at any time stream the same stretch of the reference (L2 reuse).
struct WorkItem {
    int qblock, rng, nrng;  // query block; its reference range and how many ranges the block is split into (1: one range)
    int r_begin, r_end;     // reference rows of the range
};
__device__ __forceinline__ WorkItem decode_work_item(int first_begin, int range_len, int r_limit, int n_full, int nranges) {
    int qblock = blockIdx.x, rng = 0, nrng = 1, r_begin = first_begin, r_end = r_limit;
    if ((int)blockIdx.x >= n_full) {
        const int nsplit = (gridDim.x - n_full) / nranges, jx = blockIdx.x - n_full;
        rng = jx / nsplit;
        qblock = n_full + (jx - rng * nsplit);
        nrng = nranges;
        r_begin = first_begin + rng * range_len;
        r_end = min(r_limit, r_begin + range_len);
    }
    return WorkItem{qblock, rng, nrng, r_begin, r_end};
}

__device__ __forceinline__ int lds_load_volatile(const int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ int mbcnt64(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Per-wave cycle accounting.  A role owns one Stamps and calls it unconditionally: st.count(Stamps::NCOMP), const auto t0 =
// st.now(); ... st.since(Stamps::COMP, t0).  In the product build the type has no state and every member is empty, so
// nothing of it reaches the ISA; under BMX_STAMPS it holds the counters and now() reads the cycle counter.
struct Stamps {
    enum Counter { NCOMP, COMP, ROUNDS, DRAIN, NDRAIN, IDLE, SPIN, EVT, GRP, EVC, QWAIT, NSPIN, NFLUSH, PWAIT, NCOUNTERS };
#ifdef BMX_STAMPS
    unsigned long long v[NCOUNTERS] = {};
    unsigned long long t0 = 0;
    unsigned long long rt0 = 0, sweep_cycles = 0, sweep_ticks = 0;
    __device__ __forceinline__ static unsigned long long now() { return __builtin_readcyclecounter(); }
    // the constant 100 MHz counter (s_memrealtime) beside the cycle counter (s_memtime), read where a consumer's sweep
    // starts and where it ends: cycles / ticks x 100 MHz is the clock the sweep ran at
    __device__ __forceinline__ void begin() {
        rt0 = __builtin_amdgcn_s_memrealtime();
        t0 = now();
    }
    __device__ __forceinline__ void sweep_end() {
        sweep_cycles = now() - t0;
        sweep_ticks = __builtin_amdgcn_s_memrealtime() - rt0;
    }
    __device__ __forceinline__ unsigned long long elapsed() const { return now() - t0; }
    __device__ __forceinline__ void add(Counter c, unsigned long long x) { v[c] += x; }
    __device__ __forceinline__ unsigned long long get(Counter c) const { return v[c]; }
#else
    __device__ __forceinline__ static unsigned long long now() { return 0; }
    __device__ __forceinline__ void begin() {}
    __device__ __forceinline__ void sweep_end() {}
    __device__ __forceinline__ unsigned long long elapsed() const { return 0; }
    __device__ __forceinline__ void add(Counter, unsigned long long) {}
    __device__ __forceinline__ unsigned long long get(Counter) const { return 0; }
#endif
    __device__ __forceinline__ void count(Counter c) { add(c, 1ull); }
    __device__ __forceinline__ void since(Counter c, unsigned long long from) { add(c, now() - from); }
};

}  // namespace
}  // namespace bmx
