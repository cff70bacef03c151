// The parts of the gene-variance handles (gene_var.hip, bmx_genevar_*) that need no device: the argument checks and the
// arithmetic that folds a chunk's (count, mean, M2) into a gene's running state.  The merge is compiled for the device by
// gene_var.hip and for the host by gene_var_host_check.cpp, which runs it under the host sanitizers.
#pragma once
#include <cstdint>

#include "resident_batches.hpp"

#if defined(__HIPCC__)
#define BMX_GENEVAR_HD __host__ __device__ __forceinline__
#else
#define BMX_GENEVAR_HD inline
#endif

namespace bmx {

constexpr int GENEVAR_CHUNK = 256;                // cells per chunk, at fixed positions within a batch
constexpr int GENEVAR_MAX_GENES = 65535 * 256;    // (the gene tiles are the second grid dimension)

// (count, mean, M2 = sum of squared deviations from the mean) of a run of cells, for one gene.  Counts are whole numbers
// below 2^31, exact in FP64.
struct GeneVarState {
    double n, mean, m2;
};

// A followed by B (Chan, Golub and LeVeque's pairwise update), in this order of operations:
//   delta = mB - mA;  n = nA + nB;  mean = mA + (delta * nB) / n;  M2 = (M2A + M2B) + (((delta * delta) * nA) * nB) / n
// An empty A gives B itself, bit for bit: a batch's first chunk starts its state.
BMX_GENEVAR_HD GeneVarState genevar_merge(GeneVarState a, GeneVarState b) {
    if (a.n == 0.0) return b;
    if (b.n == 0.0) return a;
    const double n = a.n + b.n;
    const double delta = b.mean - a.mean;
    GeneVarState r;
    r.n = n;
    r.mean = a.mean + (delta * b.n) / n;
    r.m2 = (a.m2 + b.m2) + (((delta * delta) * a.n) * b.n) / n;
    return r;
}

// the sample variance of a finished state: M2 / (n - 1), NaN for a single cell (0 / 0)
BMX_GENEVAR_HD double genevar_total(GeneVarState s) { return s.m2 / (s.n - 1.0); }

// ---- argument checks (throw Error(BMX_ERR_ARG))
inline void genevar_check_create(int G) {
    if (G < 1) throw Error(BMX_ERR_ARG, "modelGeneVar needs at least one gene");
    if (G > GENEVAR_MAX_GENES) throw Error(BMX_ERR_ARG, "at most 16 776 960 genes");
}

// a block of m cells for a batch of n cells of which `filled` have arrived: it fits, and unless it ends the batch it
// holds whole chunks (the chunk edges are positions within the batch, and a chunk is reduced from one block)
inline void genevar_check_block(int64_t n, int64_t filled, int64_t m) {
    check_cell_count(n);
    if (filled < 0 || m < 1 || m > n || filled > n - m)
        throw Error(BMX_ERR_ARG, "the block does not fit into the batch announced");
    if (filled % GENEVAR_CHUNK != 0 || (filled + m != n && m % GENEVAR_CHUNK != 0))
        throw Error(BMX_ERR_ARG, "a block that does not end its batch must hold whole chunks of 256 cells");
}

inline void genevar_check_sparse_block(int64_t n, int64_t filled, int64_t m, const int64_t* indptr, const int32_t* indices,
                                       const double* data, int64_t nnz) {
    genevar_check_block(n, filled, m);
    check_csc_block(n, filled, m, indptr, indices, data, nnz);
}

}  // namespace bmx
