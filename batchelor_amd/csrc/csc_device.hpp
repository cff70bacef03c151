// Device helpers of the kernels that read a batch kept as CSC (indptr absolute, rows ascending within a column): NormSparse
// (multi_batch_norm.hip), PcaSparse (pca_sparse.hip), DeltaSparse (delta_variance.hip: two arbitrary columns per pair, one
// wave a tile), GeneVarSparse (gene_var.hip, over one block at a time) and ClusterSparse (cluster_mnn.hip: the tile walk
// over a list of cells, and the wave gather it shares with PcaSparse).  The store and the host's checks are in
// resident_batches.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bmx {

// Entry k (row r) of the column that begins at kb: a row that is not above the one stored before it sets bad_order, a row
// outside [0, G) sets bad_row.  Whether the row is outside: the entry then addresses nothing and is left out.
__device__ __forceinline__ bool csc_entry_flags(const int32_t* __restrict__ idx, int64_t k, int64_t kb, int32_t r, int G,
                                                int& bad_row, int& bad_order) {
    if (k > kb && idx[k - 1] >= r) bad_order = 1;
    if (r >= 0 && r < G) return false;
    bad_row = 1;
    return true;
}

// the first position in [lo, hi) whose row is not below g (rows ascending; on rows in any order it still ends, somewhere
// in [lo, hi])
__device__ __forceinline__ int64_t first_row_at_least(const int32_t* __restrict__ idx, int64_t lo, int64_t hi, int g) {
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (idx[mid] < g) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// A workgroup of 256 threads walks the cells [chunk * CELLS, min(n, (chunk + 1) * CELLS)) x the rows [g0, g1): thread t
// first finds the tile's entries in the chunk's column t (lo / hi: the caller's shared arrays [CELLS]); after a barrier
// the columns are taken one after the other, col_begin(c) at the start of cell c's column, then the threads stride over
// the column's entries in the tile, entry(c, k, r) for position k with row r, and a barrier before the next column.  Rows
// are unique within a canonical column, so no two threads meet at a row; on any pattern r stays inside [g0, g1).  (The
// callbacks get the cell and not its number in the chunk: handed the number, sp_sort_kernel<true> came out 1.5 % slower.)
//
// cols (nullable): the chunk is then the positions [list_b, list_b + list_ncol) of that list of cells, list_ncol <= CELLS
// (ClusterSparse: the restricted cells sorted by cluster; n and chunk play no part).  A pointer in this one body and not a
// second walk under both forms: with the mapping of a position to its cell handed in as a callable, the kernels of the
// callers that pass no list came out with another loop test; this way their code is what it was, instruction for instruction.
template <int CELLS, class ColBegin, class Entry>
__device__ __forceinline__ void csc_tile_walk(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx, int64_t n,
                                              int64_t chunk, int g0, int g1, int64_t* lo, int64_t* hi, ColBegin&& col_begin,
                                              Entry&& entry, const int32_t* __restrict__ cols = nullptr, int list_b = 0,
                                              int list_ncol = 0) {
    const int64_t b = cols ? (int64_t)list_b : chunk * CELLS;
    const int ncol = cols ? list_ncol : (int)((b + CELLS < n ? b + CELLS : n) - b);
    if ((int)threadIdx.x < ncol) {
        const int64_t c = cols ? (int64_t)cols[b + threadIdx.x] : b + threadIdx.x;
        const int64_t kb = indptr[c], ke = indptr[c + 1];
        const int64_t first = first_row_at_least(idx, kb, ke, g0);
        lo[threadIdx.x] = first;
        hi[threadIdx.x] = first_row_at_least(idx, first, ke, g1);
    }
    __syncthreads();
    for (int j = 0; j < ncol; ++j) {
        const int64_t c = cols ? (int64_t)cols[b + j] : b + j;
        col_begin(c);
        const int64_t ke = hi[j];
        for (int64_t k = lo[j] + threadIdx.x; k < ke; k += 256) {
            const int r = idx[k];
            if (r >= g0 && r < g1) entry(c, k, r);
        }
        __syncthreads();
    }
}
template <int CELLS, class Entry>
__device__ __forceinline__ void csc_tile_walk(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx, int64_t n,
                                              int64_t chunk, int g0, int g1, int64_t* lo, int64_t* hi, Entry&& entry) {
    csc_tile_walk<CELLS>(indptr, idx, n, chunk, g0, g1, lo, hi, [](int64_t) {}, entry);
}

// A column whose address came out of memory (DeltaSparse's pair records): say that it is global memory, or the loads are
// flat ones.
typedef const __attribute__((address_space(1))) int32_t* csc_rows_ptr;
typedef const __attribute__((address_space(1))) double* csc_vals_ptr;

// ONE wave takes the n entries at idx / val -- a column's entries inside the rows [g0, g1) -- lane l the entries l,
// l + 64, ...  The lane's first entry comes in as r0 / v0: the caller loads it, with other columns' loads in flight
// (r0 < 0: the lane has none).  entry(r - g0, value); on any pattern r stays inside [g0, g1).
template <class Entry>
__device__ __forceinline__ void csc_wave_walk(csc_rows_ptr idx, csc_vals_ptr val, int n, int lane, int g0, int g1, int r0,
                                              double v0, Entry&& entry) {
    if (r0 >= g0 && r0 < g1) entry(r0 - g0, v0);
    for (int k = lane + 64; k < n; k += 64) {
        const int r = idx[k];
        if (r >= g0 && r < g1) entry(r - g0, val[k]);
    }
}

// ---- one wave a column (or a row of PcaSparse's companion) against a dense row-major matrix, a lane per matrix column
__device__ __forceinline__ int64_t wave_uniform(int64_t v) {  // v is the same in every lane: keep it in scalar registers
    const int lo = __builtin_amdgcn_readfirstlane((int)(v & 0xffffffffll));
    const int hi = __builtin_amdgcn_readfirstlane((int)(v >> 32));
    return ((int64_t)hi << 32) | (int64_t)(unsigned)lo;
}
__device__ __forceinline__ double lane_value(double x, int l) {  // lane l's x, l the same in every lane
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), l);
    return __hiloint2double(hi, lo);
}

// Lane j's  sum over the entries k in [kb, ke), in order, of val[k] * M[idx[k] * ldm + j]  (j < 64; kb, ke wave-uniform).
// An entry whose index is outside [0, bound) is skipped.  The wave reads 64 entries at once, then takes them one after
// the other, four gathers in flight.
__device__ __forceinline__ double gather_rows64(const int32_t* __restrict__ idx, const double* __restrict__ val, int64_t kb,
                                                int64_t ke, const double* __restrict__ M, int64_t ldm, int64_t bound,
                                                int lane) {
    double acc = 0.0;
    for (int64_t k0 = kb; k0 < ke; k0 += 64) {
        const int64_t k = k0 + lane;
        int32_t r = -1;
        double v = 0.0;
        if (k < ke) {
            r = idx[k];
            v = val[k];
        }
        const int cnt = (int)(ke - k0 < 64 ? ke - k0 : 64);
        for (int i = 0; i < cnt; i += 4) {  // (lanes at and after cnt hold r = -1: skipped)
            int ri[4];
            double vi[4], q[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                ri[u] = __builtin_amdgcn_readlane(r, i + u);
                vi[u] = lane_value(v, i + u);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) q[u] = (ri[u] >= 0 && ri[u] < bound) ? M[(int64_t)ri[u] * ldm + lane] : 0.0;
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (ri[u] >= 0 && ri[u] < bound) acc += vi[u] * q[u];
        }
    }
    return acc;
}

}  // namespace bmx
