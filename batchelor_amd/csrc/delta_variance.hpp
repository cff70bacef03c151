// mnnDeltaVariance() on the device (delta_variance.hip): the batches stay resident, the per-gene mean and variance of the
// MNN-pair deltas of every merge step come out of one run.  Host-side interface behind the bmx_delta_* entry points.
#pragma once
#include <cstdint>

namespace bmx {

class Delta;
constexpr int DELTA_GENE_TILE = 256;   // genes a workgroup of the pair passes owns
constexpr int DELTA_PAIR_CHUNK = 128;  // pairs of one step a workgroup walks (fixed: the results do not depend on the grid)
constexpr int DELTA_STAGES = 5;

struct DeltaRun {
    int cos_norm = 0;
    const int32_t* norm_genes0 = nullptr;  // 0-based genes the cosine norms are taken over (null: all genes)
    int n_norm_genes = 0;
    int nsteps = 0;
    const int32_t* const* left = nullptr;   // per step: 1-based columns of the batches in upload order
    const int32_t* const* right = nullptr;
    const int64_t* npairs = nullptr;
    double* mean = nullptr;   // [G x nsteps] column-major
    double* total = nullptr;  // [G x nsteps] column-major
};

// argument checks of delta_begin_batch / delta_run without a device (throw Error): G genes, N cells uploaded so far
void delta_check_batch(int64_t n, int64_t cells_before);
void delta_check_run(int G, int64_t N, const DeltaRun& a);

Delta* delta_create(int device, int G);
void delta_destroy(Delta* h);
void delta_begin_batch(Delta* h, int64_t n);
void delta_add_block(Delta* h, const double* x_block_host, int64_t m);
void delta_run(Delta* h, const DeltaRun& a);
// milliseconds since the handle was made: upload (host wall time), HIP-event time of the cell norms, of the two pair
// passes, of the pair preparation and the reductions over chunks, and the host wall time of the runs
void delta_stage_ms(const Delta* h, double* out5);

}  // namespace bmx
