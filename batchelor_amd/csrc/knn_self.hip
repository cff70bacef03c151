// findKNN's last step: the lists of a search of X against itself at k + 1 lose the query's own row.
//   own row among the k + 1 entries: that entry goes, the later ones move up;
//   own row not among them: the last entry goes -- k + 1 rows with lower numbers coincide with the query at distance 0 (ties
//   go to the lower row), so the first k of the list are its k nearest OTHER rows.
// No floating-point arithmetic: the distances that leave are the search's own bits.
#include "bmx_ops.hpp"

namespace bmx {

namespace {

constexpr int KS_WAVES = 4;  // queries (waves) a workgroup

// One wave a query: a ballot per 64 entries finds the own row's place, then the lanes stride over the row (coalesced reads
// and writes).  in [nq][k + 1] and out [nq][k] overlap row by row: they are different buffers.
__global__ __launch_bounds__(64 * KS_WAVES) void drop_self_kernel(const int32_t* __restrict__ idx_in, const double* __restrict__ dist_in,
                                                                  const int32_t* __restrict__ q_rows, int nq, int k,
                                                                  int32_t* __restrict__ idx_out, double* __restrict__ dist_out) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * KS_WAVES + (threadIdx.x >> 6);
    if (q >= nq) return;  // (whole waves leave: no barrier below)
    const int self = q_rows ? q_rows[q] : q;
    const int32_t* ii = idx_in + (int64_t)q * (k + 1);
    int pos = k;  // the entry that goes
    for (int j0 = 0; j0 <= k; j0 += 64) {
        const int j = j0 + lane;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(j <= k && ii[j] == self);
        if (m) {
            pos = j0 + __builtin_ctzll(m);
            break;
        }
    }
    int32_t* io = idx_out + (int64_t)q * k;
    for (int j = lane; j < k; j += 64) io[j] = ii[j + (j >= pos ? 1 : 0)];
    if (dist_out) {
        const double* di = dist_in + (int64_t)q * (k + 1);
        double* dout = dist_out + (int64_t)q * k;
        for (int j = lane; j < k; j += 64) dout[j] = di[j + (j >= pos ? 1 : 0)];
    }
}

}  // namespace

void knn_drop_self(hipStream_t stream, const int32_t* idx_in, const double* dist_in, const int32_t* q_rows, int nq, int k,
                   int32_t* idx_out, double* dist_out) {
    if (nq <= 0 || k <= 0) return;
    hipLaunchKernelGGL(drop_self_kernel, dim3((unsigned)((nq + KS_WAVES - 1) / KS_WAVES)), dim3(64 * KS_WAVES), 0, stream, idx_in,
                       dist_in, q_rows, nq, k, idx_out, dist_out);
    BMX_LAUNCH_CHECK();
}

}  // namespace bmx
