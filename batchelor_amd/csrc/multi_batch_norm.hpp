// multiBatchNorm() on the device (multi_batch_norm.hip): the count batches stay resident between the passes that need
// every cell (library sizes, per-gene averages), the ratio stage and the pass that writes the normalized values.
// Host-side interface behind the bmx_norm_* entry points.
#pragma once
#include <cstdint>

namespace bmx {

class Norm;

// stat_rows: 1-based rows the size factors, averages and ratios are taken over (in the order given, a row named twice
// counts twice), n_stat of them; null / n_stat < 0: all G rows.  The values are written for all G rows either way.
Norm* norm_create(int device, int G, const int32_t* stat_rows, int64_t n_stat);
void norm_destroy(Norm* h);
// argument checks of norm_create / norm_begin_batch / norm_run without a device (throw Error(BMX_ERR_ARG))
void norm_check_create(int G, const int32_t* stat_rows, int64_t n_stat);
void norm_check_batch(int64_t n, const double* size_factors);
void norm_check_run(double min_mean, int log, double pseudo_count);
// a batch of n cells, size_factors [n] (any scale; null: library sizes over the statistic rows); its columns follow in
// blocks, in order
void norm_begin_batch(Norm* h, int64_t n, const double* size_factors);
void norm_add_block(Norm* h, const double* x_block_host, int64_t m);
// outs[b]: [G x n_b] column-major host memory.  Nullable: sf_out [cells of all batches in upload order] the size factors
// the values were divided by, ave_out [n_stat x B] column-major, ratios_out [B x B] row-major (ratios_out[i * B + j] is
// the median over the kept genes of ave_j / ave_i), smallest_out the 1-based reference batch.
void norm_run(Norm* h, double min_mean, int log, double pseudo_count, double* const* outs, double* sf_out,
              double* ave_out, double* ratios_out, int32_t* smallest_out);
// milliseconds since the handle was made: upload (host wall time), HIP-event time of the statistics passes (column sums,
// per-gene sums, size factors, averages), of the ratio stage, of the output kernels, and the host wall time of the output
// pass with its downloads
void norm_stage_ms(const Norm* h, double* out5);

// ---- the same for sparse counts: a batch is kept as CSC (indptr int64, 0-based int32 rows, FP64 values), its cells
// arrive in column blocks, and the values are written for the stored entries only.
class NormSparse;
NormSparse* norm_sparse_create(int device, int G, const int32_t* stat_rows, int64_t n_stat);
void norm_sparse_destroy(NormSparse* h);
// a block of m cells for a batch of n cells that holds `filled` so far, without a device (throws Error(BMX_ERR_ARG)):
// indptr [m + 1] relative to the block (starts at 0, never decreases, ends at nnz); indices / data [nnz]
void norm_check_sparse_block(int64_t n, int64_t filled, int64_t m, const int64_t* indptr, const int32_t* indices,
                             const double* data, int64_t nnz);
// a batch of n cells with nnz stored entries in all; size_factors as for norm_begin_batch
void norm_sparse_begin_batch(NormSparse* h, int64_t n, const double* size_factors, int64_t nnz);
void norm_sparse_add_block(NormSparse* h, int64_t m, const int64_t* indptr, const int32_t* indices, const double* data,
                           int64_t nnz);
// outs[b]: [nnz_b] the values of batch b's stored entries, in their order.  zero_out (nullable): what the same pass
// makes of a count of zero, log2(pseudo_count) by the device's log2 or 0.  The rest as for norm_run.
void norm_sparse_run(NormSparse* h, double min_mean, int log, double pseudo_count, double* const* outs, double* sf_out,
                     double* ave_out, double* ratios_out, int32_t* smallest_out, double* zero_out);
void norm_sparse_stage_ms(const NormSparse* h, double* out5);

}  // namespace bmx
