// rescaleBatches() / regressBatches() on the device (linear_correct.hip): the batches stay resident between the pass that
// needs every cell (the per-gene statistics) and the pass that writes the result.  Host-side interface behind the
// bmx_linear_* entry points.
#pragma once
#include <cstdint>

namespace bmx {

class Linear;
constexpr int LINEAR_MAX_P = 64;  // columns a design may have

Linear* linear_create(int device, int G);
void linear_destroy(Linear* h);
// What the caller is going to ask for, said before the upload so that the per-gene sums of a column block run behind the
// upload of the next one: kind 0 nothing, 1 plain sums (regressBatches, default design), 2 sums of log_base^x -
// pseudo_count (rescaleBatches).  keep_unlogged != 0 (kind 2): the unlogged values are kept in HBM for the second pass.
void linear_expect(Linear* h, int kind, double log_base, double pseudo_count, int keep_unlogged);
// argument checks of linear_begin_batch / linear_rescale / linear_regress without a device (throw Error(BMX_ERR_ARG))
void linear_check_batch(int64_t n, const int32_t* restrict_idx, int64_t n_restrict);
void linear_check_rescale(double log_base, double pseudo_count);
void linear_check_regress(const double* design, int p, const double* w, const int32_t* keep, int n_keep);
// a batch of n cells, restrict_idx 1-based cells (null / n_restrict < 0: all); its columns follow in blocks, in order
void linear_begin_batch(Linear* h, int64_t n, const int32_t* restrict_idx, int64_t n_restrict);
void linear_add_block(Linear* h, const double* x_block_host, int64_t m);
// outs[b]: [G x n_b] column-major host memory; avg_out [G x B], ref_out [G] (nullable)
void linear_rescale(Linear* h, double log_base, double pseudo_count, double* const* outs, double* avg_out, double* ref_out);
// design null: one indicator column per batch, coef_out [G x B] (the batch means).  Otherwise design [N x p] column-major
// over the cells of all batches in upload order, w [R x p] column-major with coef = X[:, restricted] %*% w (R: the
// restricted cells, batch by batch, ascending within a batch), keep 1-based columns that are not regressed out;
// coef_out [G x p] (nullable)
void linear_regress(Linear* h, const double* design, int p, const double* w, const int32_t* keep, int n_keep,
                    double* const* outs, double* coef_out);
// the batches as they were uploaded, back through the download ring with no kernel in between: what moving a call's
// bytes in and out costs at the least
void linear_fetch(Linear* h, double* const* outs);
// milliseconds since the handle was made: upload (host wall time), HIP-event time of the first pass (chunk sums or the
// product with w), of the statistics kernels, of the second pass's kernels, and the host wall time of the second pass
// with its downloads
void linear_stage_ms(const Linear* h, double* out5);

}  // namespace bmx
