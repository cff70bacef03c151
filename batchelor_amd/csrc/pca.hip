// multiBatchPCA on the device (R/multiBatchPCA.R:211-322): the step directly upstream of the merge engine in fastMNN()
// (R/fastMNN.R:353-354), "often the most time-consuming step" (R/reducedMNN.R:25).
//
// The reference takes an SVD of the scaled genes x cells matrix  A = [ C_1 sqrt(w_1/n_1) | C_2 sqrt(w_2/n_2) | ... ],
// C_b = x_b - mu 1^T with mu the weighted mean of the batch means, and projects the UNSCALED centred batches on the top
// d left singular vectors u.  At 20 000 genes x 800 000 cells A is 128 GB; here it is never formed, and neither is the
// genes x genes Gram matrix: the batches stay in HBM as uploaded (genes x cells column-major = one contiguous gene
// vector per cell), and the top subspace of  M = A A^T = sum_b (w_b/n_b) C_b C_b^T  is found by blocked subspace
// iteration with L = 64 vectors (d <= 50 wanted + oversampling):
//     Z_b = C_b^T Q            (cells x 64)   -- "NT" product, K = genes
//     Y  += (w_b/n_b) C_b Z_b  (genes x 64)   -- "TN" product, K = cells
//     Q   = orth(Y)            (Cholesky QR, twice)
// and a Rayleigh-Ritz step on the last pair (Q, Y = M Q) gives the rotation and the singular values.  Cosine
// normalisation (R/cosineNorm.R, fastMNN's cos.norm=TRUE) is a per-cell factor folded into the two products, the
// centring a rank-one correction -- the normalised, centred data is never written.
// Both products run on the FP64 matrix cores (v_mfma_f64_16x16x4_f64): 64 x 64 output tiles per workgroup, operands
// brought in by whole-row 16-byte loads one K step ahead (registers) and staged in the LDS with pitches that keep the
// 32-lane fragment reads conflict-free.
// The iteration itself (start block, Cholesky QR 2, Rayleigh-Ritz, Chebyshev filter, residual) is SubspaceIteration
// (pca_iteration.hpp), shared with the sparse handle; this file has the dense operator, the centre, the rotation and the
// projections.
//
// subset.row / get.all.genes / get.variance (R/multiBatchPCA.R:401-432): the handle holds the subset rows only; PcaGenes
// (bmx_pca_genes_*) borrows it once fitted and streams the other rows through gemm_tn64_sums for their rotation rows and
// centres, keeping none of them, and sums var.total over the resident rows.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "bmx_ops.hpp"
#include "host_xfer.hpp"
#include "pca_iteration.hpp"
#include "resident_batches.hpp"

namespace bmx {

// ---------------------------------------------------------------------------------------------------
struct PcaBatch : ResidentBatch {
    DevBuf<double> inv;  // [n] 1 / max(1e-8, l2), empty without cosine normalisation
    double weight = 1.0;
    bool cos_norm = false;
};

class Pca : ResidentBatches<PcaBatch> {
  public:
    Pca(int device, int G) : ResidentBatches(device, G, "bmx_pca_begin_batch") {}
    ~Pca() { retire(); }

    // a batch of n cells whose columns arrive in one or more blocks (add_block), in order
    void begin_batch(int64_t n, double weight, bool cos_norm) {
        check_cell_count(n, false);
        begin(n, [&](PcaBatch& b) {
            b.weight = weight;
            b.cos_norm = cos_norm;
            if (cos_norm) b.inv.reserve((size_t)n);
        });
        fitted_ = false;
        ++generation_;
    }
    void add_block(const double* x_block, int64_t m) {
        add(x_block, m, [&](PcaBatch& b, double* p) {
            if (!b.cos_norm) return;
            cell_l2_device(stream_, p, G_, m, nullptr, 0, true, b.inv.p + (b.filled - m));
        });
    }
    void add_batch(const double* x, int64_t n, double weight, bool cos_norm) {
        begin_batch(n, weight, cos_norm);
        add_block(x, n);
    }

    // multiBatchPCA: centres [G], rotation [G x d] column-major, sdev [d] (singular values of the scaled matrix).
    // Chebyshev-filtered subspace iteration on a block of L = 64 (d <= 56) or 128 (d <= 120) vectors until the Ritz
    // residuals max_j |M x_j - theta_j x_j| / theta_1 of the d wanted pairs are <= tol (tol > 0), at most max_applies
    // applications of M (throws if they do not reach it, after the results have been written); tol <= 0: exactly
    // max_applies plain subspace steps (the fixed-count form).  The handle is unfitted from here until the results have
    // been written: a fit that throws anything but the non-convergence error leaves it so.
    void fit(int d, double tol, int max_applies, double* centers, double* rotation, double* sdev, int* applies_used,
             double* resid_out) {
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        fitted_ = false;
        ++generation_;
        if (batches_.empty()) throw Error(BMX_ERR_ARG, "at least one batch must be specified");
        if (batches_.back()->filled != batches_.back()->n)
            throw Error(BMX_ERR_ARG, "the last batch has not received all its cells");
        int64_t ncells = 0;
        for (auto& bp : batches_) ncells += bp->n;
        const int L = SubspaceIteration::width_for(d, G_, ncells, max_applies);
        const int G = G_;
        // ---- grand centre: weighted mean of the batch means (R/multiBatchPCA.R:268-281)
        double* mu = mu_.reserve((size_t)G);
        BMX_HIP(hipMemsetAsync(mu, 0, (size_t)G * sizeof(double), stream_));
        double wsum = 0.0;
        for (auto& bp : batches_) wsum += bp->weight;
        for (auto& bp : batches_) {
            PcaBatch& b = *bp;
            const int nchunk = (int)std::min<int64_t>(512, std::max<int64_t>(1, b.n / 256));
            const int64_t per = (b.n + nchunk - 1) / nchunk;
            double* part = part_.reserve((size_t)nchunk * G + (size_t)G);
            double* mean = part + (size_t)nchunk * G;
            hipLaunchKernelGGL(genesum_partial, dim3(cdiv(G, 256), nchunk), dim3(256), 0, stream_, b.x.p,
                               b.cos_norm ? b.inv.p : nullptr, b.n, G, per, part);
            hipLaunchKernelGGL(reduce_parts, dim3((unsigned)cdiv(G, 256)), dim3(256), 0, stream_, part, nchunk, (int64_t)G,
                               1.0 / (double)b.n, 0.0, mean, G, (int64_t)G);
            hipLaunchKernelGGL(axpy_kernel, dim3((unsigned)cdiv(G, 256)), dim3(256), 0, stream_, mu, mean, b.weight / wsum,
                               (int64_t)G);
            BMX_LAUNCH_CHECK();
        }
        qt_.reserve((size_t)G * PL);
        off_.reserve(4 * (size_t)PL);
        const SubspaceIteration::Outcome outcome =
            it_.run(stream_, G, d, tol, max_applies, [&](const double* Q, double* Y) { apply_operator(Q, Y); });
        // ---- results: rotation = the first d Ritz vectors
        const double* Xr = it_.ritz_vectors();
        double* Ut = ut_.reserve((size_t)G * L);  // [L][G]: the B operand of the projection
        for (int h = 0; h < L / PL; ++h) {
            hipLaunchKernelGGL(transpose64, dim3((unsigned)cdiv(G, 64)), dim3(256), 0, stream_, (const double*)(Xr + h * PL),
                               (int64_t)L, (int64_t)G, Ut + (size_t)h * PL * G);
            BMX_LAUNCH_CHECK();
        }
        // mu . u_j for the projection's centring
        double* muU = off_.p + 2 * PL;
        for (int h = 0; h < L / PL; ++h) {
            hipLaunchKernelGGL(gemm_nt64, dim3(1), dim3(256), 0, stream_, (const double*)mu, (int64_t)1, G, (int64_t)G,
                               (const double*)(Ut + (size_t)h * PL * G), (int64_t)G, (const double*)nullptr,
                               (const double*)nullptr, muU + h * PL, (int64_t)PL);  // one row: Z[0][j] = mu . Ut[j]
            BMX_LAUNCH_CHECK();
        }
        if (centers) BMX_HIP(hipMemcpyAsync(centers, mu, (size_t)G * sizeof(double), hipMemcpyDeviceToHost, stream_));
        if (rotation)  // the first d rows of Ut are the d columns of the rotation, column-major
            BMX_HIP(hipMemcpyAsync(rotation, Ut, (size_t)G * d * sizeof(double), hipMemcpyDeviceToHost, stream_));
        BMX_HIP(hipStreamSynchronize(stream_));
        fitted_ = true;
        it_.report(tol, outcome, sdev, applies_used, resid_out);
    }

    // crossprod(x_b - centers, rotation): [n_b x d] column-major
    void project(int b, double* out) {
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        if (!fitted_) throw Error(BMX_ERR_ARG, "bmx_pca_fit has not been run");
        if (b < 0 || b >= (int)batches_.size()) throw Error(BMX_ERR_ARG, "batch index out of range");
        PcaBatch& B = *batches_[b];
        double* Z = z_.reserve((size_t)B.n * PL);
        double* Zt = zt_.reserve((size_t)B.n * PL);
        const double* muU = mu_dot_u();
        const int d = it_.d();
        for (int h = 0; h * PL < d; ++h) {
            hipLaunchKernelGGL(gemm_nt64, dim3((unsigned)cdiv(B.n, 64)), dim3(256), 0, stream_, (const double*)B.x.p, B.n, G_,
                               (int64_t)G_, (const double*)(ut_.p + (size_t)h * PL * G_), (int64_t)G_,
                               (const double*)(B.cos_norm ? B.inv.p : nullptr), (const double*)(muU + h * PL), Z, (int64_t)PL);
            BMX_LAUNCH_CHECK();
            hipLaunchKernelGGL(transpose64, dim3((unsigned)cdiv(B.n, 64)), dim3(256), 0, stream_, (const double*)Z, (int64_t)PL,
                               B.n, Zt);
            BMX_LAUNCH_CHECK();
            const int cols = std::min(PL, d - h * PL);
            BMX_HIP(hipMemcpyAsync(out + (size_t)h * PL * B.n, Zt, (size_t)B.n * cols * sizeof(double), hipMemcpyDeviceToHost,
                                   stream_));
            BMX_HIP(hipStreamSynchronize(stream_));  // Z / Zt are reused by the next half
        }
    }
    // ---- what PcaGenes reads of a fitted Pca
    int device() const { return device_; }
    int nbatches() const { return (int)batches_.size(); }
    int genes() const { return G_; }
    const std::vector<std::unique_ptr<PcaBatch>>& batches() const { return batches_; }
    bool fitted() const { return fitted_; }
    unsigned long long generation() const { return generation_; }
    int d() const { return it_.d(); }
    const std::vector<double>& theta() const { return it_.theta(); }  // the eigenvalues s^2, descending
    const double* centre() const { return mu_.p; }                    // [G]
    const double* rotation_t() const { return ut_.p; }                // [L][G]: row j is u_j
    const double* mu_dot_u() const { return off_.p + 2 * PL; }        // [L]: mu . u_j

  private:
    // Y = M Q = sum_b (w_b / n_b) C_b C_b^T Q for a block of L vectors, 64 at a time
    void apply_operator(const double* Q, double* Y) {
        const int G = G_, L = it_.L();
        double* Qt = qt_.p;
        double* muQ = off_.p;
        double* zsum = off_.p + PL;
        BMX_HIP(hipMemsetAsync(Y, 0, (size_t)G * L * sizeof(double), stream_));
        for (int h = 0; h < L / PL; ++h) {
            hipLaunchKernelGGL(transpose64, dim3((unsigned)cdiv(G, 64)), dim3(256), 0, stream_, Q + h * PL, (int64_t)L, (int64_t)G,
                               Qt);
            BMX_LAUNCH_CHECK();
            hipLaunchKernelGGL(gemm_nt64, dim3(1), dim3(256), 0, stream_, (const double*)mu_.p, (int64_t)1, G, (int64_t)G,
                               (const double*)Qt, (int64_t)G, (const double*)nullptr, (const double*)nullptr, muQ, (int64_t)PL);
            BMX_LAUNCH_CHECK();
            double* Yh = Y + h * PL;
            for (auto& bp : batches_) {
                PcaBatch& b = *bp;
                const double* rs = b.cos_norm ? b.inv.p : nullptr;
                double* Z = z_.reserve((size_t)b.n * PL);
                // Z = C_b^T Q = diag(rs) X Q - 1 (mu^T Q)
                hipLaunchKernelGGL(gemm_nt64, dim3((unsigned)cdiv(b.n, 64)), dim3(256), 0, stream_, (const double*)b.x.p, b.n, G,
                                   (int64_t)G, (const double*)Qt, (int64_t)G, rs, (const double*)muQ, Z, (int64_t)PL);
                BMX_LAUNCH_CHECK();
                // Y += coef (X^T diag(rs) Z - mu (1^T Z))
                const double coef = b.weight / (double)b.n;
                const int gtiles = cdiv(G, 64);
                int nsplit = (int)std::min<int64_t>(std::max<int64_t>(1, (int64_t)1024 / gtiles), std::max<int64_t>(1, b.n / 2048));
                nsplit = std::max(1, nsplit);
                const int64_t per = round_up((b.n + nsplit - 1) / nsplit, KC);
                nsplit = (int)((b.n + per - 1) / per);
                double* part = part_.reserve((size_t)nsplit * G * PL + (size_t)4096 * PL);
                hipLaunchKernelGGL(gemm_tn64, dim3(gtiles, nsplit), dim3(256), 0, stream_, (const double*)b.x.p, b.n, G, (int64_t)G,
                                   (const double*)Z, (int64_t)PL, rs, per, part);
                hipLaunchKernelGGL(reduce_parts, dim3((unsigned)cdiv((int64_t)G * PL, 256)), dim3(256), 0, stream_,
                                   (const double*)part, nsplit, (int64_t)G * PL, coef, 1.0, Yh, PL, (int64_t)L);
                BMX_LAUNCH_CHECK();
                // column sums of Z (no row factor: the centring term is mu 1^T Z)
                column_sums64(stream_, Z, b.n, part + (size_t)nsplit * G * PL, 1.0, 0.0, zsum);
                hipLaunchKernelGGL(rank1_sub, dim3((unsigned)cdiv((int64_t)G * PL, 256)), dim3(256), 0, stream_, Yh, (int64_t)L,
                                   (const double*)mu_.p, (const double*)zsum, coef, G);
                BMX_LAUNCH_CHECK();
            }
        }
    }

    SubspaceIteration it_;
    unsigned long long generation_ = 0;  // counts begin_batch and fit: what a PcaGenes was made for
    // off_: mu . Q of the block being applied [PL], the column sums of Z [PL], mu . u_j [2 PL]
    DevBuf<double> mu_, qt_, ut_, z_, zt_, part_, off_;
    bool fitted_ = false;
};

// ---------------------------------------------------------------------------------------------------
// The genes outside subset.row (R/multiBatchPCA.R:401-414, .make_pca_metadata with get.all.genes): their centres mu_L and
// rotation rows  U_L = L_scaled V diag(1 / s),  V = S_scaled^T U diag(1 / s),  which with coef_b = w_b / n_b is
//     U_L[g][j] = ( sum_b coef_b sum_c scale_c x_gc Z_b[c][j]  -  mu_L[g] sum_b coef_b sum_c Z_b[c][j] ) / s_j^2,
// Z_b = C_b^T U the batch's projections.  The leftover rows of every batch stream through in column blocks and are not
// kept: a block lands in one of two device buffers on the copy stream while the kernels of the block before it run on the
// other.  The projections of a block's cells come from the RESIDENT subset rows of the borrowed, fitted Pca (gemm_nt64 on
// its rotation_t() / mu_dot_u(), as Pca::project), so nothing but the leftover rows crosses the link.  scale is the batch's inv: the norms
// over the subset rows (R/fastMNN.R:348-351).  The Pca must outlive this handle; one that was re-fitted or given another
// batch since makes every later call an error.
// ---------------------------------------------------------------------------------------------------
class PcaGenes {
  public:
    PcaGenes(int GL, Pca* pca) : pca_(*pca), made_for_(pca->generation()), GL_(GL), device_(pca->device()) {
        if (!pca_.fitted()) throw Error(BMX_ERR_ARG, "bmx_pca_fit has not been run");
        nh_ = cdiv(pca_.d(), PL);
        for (auto& bp : pca_.batches()) wsum_ += bp->weight;
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        BMX_HIP(hipStreamCreateWithFlags(&copy_, hipStreamNonBlocking));
        BMX_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
        for (int i = 0; i < 2; ++i) {
            BMX_HIP(hipEventCreateWithFlags(&landed_[i], hipEventDisableTiming));
            BMX_HIP(hipEventCreateWithFlags(&used_[i], hipEventDisableTiming));
        }
        const size_t GLn = (size_t)std::max(GL_, 1);
        acc_.reserve((size_t)nh_ * GLn * PL);
        sums_.reserve(GLn);
        mu_.reserve(GLn);
        tsum_.reserve((size_t)nh_ * PL + 2 * (size_t)PL * 2);
        BMX_HIP(hipMemsetAsync(acc_.p, 0, (size_t)nh_ * GLn * PL * sizeof(double), stream_));
        BMX_HIP(hipMemsetAsync(mu_.p, 0, GLn * sizeof(double), stream_));
        BMX_HIP(hipMemsetAsync(tsum_.p, 0, (size_t)nh_ * PL * sizeof(double), stream_));
    }
    PcaGenes(const PcaGenes&) = delete;
    PcaGenes& operator=(const PcaGenes&) = delete;
    ~PcaGenes() {
        (void)hipSetDevice(device_);
        for (hipStream_t s : {copy_, stream_})
            if (s) {
                (void)hipStreamSynchronize(s);
                (void)hipStreamDestroy(s);
            }
        for (int i = 0; i < 2; ++i) {
            if (landed_[i]) (void)hipEventDestroy(landed_[i]);
            if (used_[i]) (void)hipEventDestroy(used_[i]);
        }
        DevBlockCache::current() = &cache_;  // as ResidentBatches::retire(): the buffers below go back to cache_
    }

    // the leftover rows of batch b (0-based) follow in blocks; batches come 0, 1, ... in order
    void begin_batch(int b) {
        check_fresh();
        check_begin(batch_ < 0 ? nullptr : &ledger_);
        if (b < 0 || b >= pca_.nbatches()) throw Error(BMX_ERR_ARG, "batch index out of range");
        if (b != batch_ + 1) throw Error(BMX_ERR_ARG, "the batches must be begun in order");
        batch_ = b;
        ledger_.n = pca_.batches()[(size_t)b]->n;
        ledger_.filled = 0;
    }
    // the next m cells of the batch begun last: x_left_block is GL x m column-major host memory
    void add_block(const double* x_left_block, int64_t m) {
        check_fresh();
        check_block(batch_ < 0 ? nullptr : &ledger_, x_left_block, m, "bmx_pca_genes_begin_batch");
        if (GL_ < 1) throw Error(BMX_ERR_ARG, "the handle was made for no leftover genes");
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        const PcaBatch& B = *pca_.batches()[(size_t)batch_];
        const int64_t first = ledger_.filled;
        const double coef = B.weight / (double)B.n;
        const double* rs = B.cos_norm ? B.inv.p + first : nullptr;
        const int G = GL_, GS = pca_.genes();
        // ---- the shapes of this block's launches
        const int gtiles = cdiv(G, 64);
        int nsplit = (int)std::min<int64_t>(std::max<int64_t>(1, (int64_t)1024 / gtiles), std::max<int64_t>(1, m / 2048));
        const int64_t per = round_up((m + nsplit - 1) / nsplit, KC);
        nsplit = (int)((m + per - 1) / per);
        if (m > cap_) {  // (a grown buffer may change hands: nothing of ours is in flight when it does)
            BMX_HIP(hipStreamSynchronize(copy_));
            BMX_HIP(hipStreamSynchronize(stream_));
            for (int i = 0; i < 2; ++i) xl_[i].reserve((size_t)m * G);
            z_.reserve((size_t)nh_ * m * PL);
            cap_ = m;
            busy_[0] = busy_[1] = false;
        }
        double* part = part_.reserve((size_t)nsplit * nh_ * G * PL + (size_t)nsplit * G + (size_t)colsum_blocks(m) * PL);
        double* spart = part + (size_t)nsplit * nh_ * G * PL;
        double* zpart = spart + (size_t)nsplit * G;
        // ---- upload into the buffer the block before the last one has left
        const int s = slot_;
        slot_ ^= 1;
        if (busy_[s]) BMX_HIP(hipStreamWaitEvent(copy_, used_[s], 0));
        upload_pageable(xl_[s].p, x_left_block, (size_t)m * G * sizeof(double), copy_);
        BMX_HIP(hipEventRecord(landed_[s], copy_));
        ledger_.filled += m;
        // ---- Z = C_b^T U for these cells, from the resident subset rows
        const double* muU = pca_.mu_dot_u();
        const int64_t zhalf = (int64_t)cap_ * PL;
        for (int h = 0; h < nh_; ++h) {
            hipLaunchKernelGGL(gemm_nt64, dim3((unsigned)cdiv(m, 64)), dim3(256), 0, stream_,
                               (const double*)(B.x.p + first * GS), m, GS, (int64_t)GS,
                               pca_.rotation_t() + (size_t)h * PL * GS, (int64_t)GS, rs,
                               (const double*)(muU + h * PL), z_.p + h * zhalf, (int64_t)PL);
            BMX_LAUNCH_CHECK();
            column_sums64(stream_, z_.p + h * zhalf, m, zpart, coef, 1.0, tsum_.p + h * PL);
        }
        // ---- one read of the leftover block: the product and the gene sums
        BMX_HIP(hipStreamWaitEvent(stream_, landed_[s], 0));
        if (nh_ == 1)
            hipLaunchKernelGGL(gemm_tn64_sums<1>, dim3(gtiles, nsplit), dim3(256), 0, stream_, (const double*)xl_[s].p, m, G,
                               (const double*)z_.p, zhalf, rs, per, part, spart);
        else
            hipLaunchKernelGGL(gemm_tn64_sums<2>, dim3(gtiles, nsplit), dim3(256), 0, stream_, (const double*)xl_[s].p, m, G,
                               (const double*)z_.p, zhalf, rs, per, part, spart);
        BMX_LAUNCH_CHECK();
        BMX_HIP(hipEventRecord(used_[s], stream_));
        busy_[s] = true;
        for (int h = 0; h < nh_; ++h)
            hipLaunchKernelGGL(reduce_parts, dim3((unsigned)cdiv((int64_t)G * PL, 256)), dim3(256), 0, stream_,
                               (const double*)(part + (size_t)h * nsplit * G * PL), nsplit, (int64_t)G * PL, coef, 1.0,
                               acc_.p + (size_t)h * G * PL, PL, (int64_t)PL);
        hipLaunchKernelGGL(reduce_parts, dim3((unsigned)cdiv(G, 256)), dim3(256), 0, stream_, (const double*)spart, nsplit,
                           (int64_t)G, 1.0, first == 0 ? 0.0 : 1.0, sums_.p, G, (int64_t)G);
        BMX_LAUNCH_CHECK();
        if (ledger_.complete()) {  // mu_L += (w_b / W) mean_b, as fit forms mu
            hipLaunchKernelGGL(axpy_kernel, dim3((unsigned)cdiv(G, 256)), dim3(256), 0, stream_, mu_.p, (const double*)sums_.p,
                               (B.weight / wsum_) / (double)B.n, (int64_t)G);
            BMX_LAUNCH_CHECK();
        }
    }
    // centers_left [GL], rotation_left [GL x d] column-major; either may be null
    void finish(double* centers_left, double* rotation_left) {
        check_fresh();
        if (batch_ != pca_.nbatches() - 1 || !ledger_.complete())
            throw Error(BMX_ERR_ARG, "the last batch has not received all its cells");
        if (GL_ < 1) return;
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        const int d = pca_.d(), G = GL_;
        double* rot = part_.reserve((size_t)G * d);  // (the stream orders this after the last block's reductions)
        leftover_rotation(stream_, pca_.theta(), d, acc_.p, mu_.p, tsum_.p, tsum_.p + (size_t)nh_ * PL, G, rot, centers_left,
                          rotation_left);
    }
    // sum_b coef_b |C_b|_F^2 over the resident (subset) rows, in the centred form; the caller divides by the batches
    void total_variance(double* var_total) {
        check_fresh();
        if (!var_total) throw Error(BMX_ERR_ARG, "null output pointer");
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        double total = 0.0;
        for (auto& bp : pca_.batches()) {
            const PcaBatch& B = *bp;
            const int nb = (int)std::min<int64_t>(1024, std::max<int64_t>(1, B.n / 64));
            const int64_t cpb = (B.n + nb - 1) / nb;
            BMX_HIP(hipStreamSynchronize(stream_));  // part_ may grow
            double* part = part_.reserve((size_t)nb);
            hipLaunchKernelGGL(centred_sq_partial, dim3(nb), dim3(256), 0, stream_, (const double*)B.x.p,
                               (const double*)(B.cos_norm ? B.inv.p : nullptr), pca_.centre(), B.n, pca_.genes(), cpb,
                               part);
            BMX_LAUNCH_CHECK();
            std::vector<double> h((size_t)nb);
            BMX_HIP(hipMemcpyAsync(h.data(), part, h.size() * sizeof(double), hipMemcpyDeviceToHost, stream_));
            BMX_HIP(hipStreamSynchronize(stream_));
            double s = 0.0;
            for (double v : h) s += v;
            total += (B.weight / (double)B.n) * s;
        }
        *var_total = total;
    }

  private:
    void check_fresh() const {
        if (pca_.generation() != made_for_ || !pca_.fitted())
            throw Error(BMX_ERR_ARG, "the PCA was re-fitted or given a batch after bmx_pca_genes_create");
    }

    DevBlockCache cache_;  // first: destroyed after every DevBuf below (see ResidentBatches::retire)
    const Pca& pca_;
    const unsigned long long made_for_;
    int GL_, device_, nh_ = 1;
    double wsum_ = 0.0;
    hipStream_t copy_ = nullptr, stream_ = nullptr;  // uploads; kernels and downloads
    hipEvent_t landed_[2] = {nullptr, nullptr}, used_[2] = {nullptr, nullptr};
    bool busy_[2] = {false, false};
    int slot_ = 0;
    int batch_ = -1;      // the batch begun last
    BlockLedger ledger_;  // its cells
    int64_t cap_ = 0;     // cells xl_ and z_ hold
    DevBuf<double> xl_[2], z_, part_, acc_, sums_, mu_, tsum_;
};

}  // namespace bmx

/* ---------------------------------------------------------------- bmx_pca_* ------------------------------------- */
struct bmx_pca final : bmx::Pca {
    using Pca::Pca;
};
struct bmx_pca_genes final : bmx::PcaGenes {
    using PcaGenes::PcaGenes;
};

extern "C" {

int32_t bmx_pca_create(int32_t device, int32_t G, bmx_pca_t** out) {
    return bmx::guarded([&] {
        if (!out) throw bmx::Error(BMX_ERR_ARG, "null output pointer");
        if (G < 1) throw bmx::Error(BMX_ERR_ARG, "the PCA needs at least one gene");
        *out = new bmx_pca(device, G);
    });
}

void bmx_pca_destroy(bmx_pca_t* p) { delete p; }

int32_t bmx_pca_add_batch(bmx_pca_t* p, const double* x, int64_t n, double weight, int32_t cos_norm) {
    return bmx::guarded([&] { bmx::live(p).add_batch(x, n, weight, cos_norm != 0); });
}

int32_t bmx_pca_begin_batch(bmx_pca_t* p, int64_t n, double weight, int32_t cos_norm) {
    return bmx::guarded([&] { bmx::live(p).begin_batch(n, weight, cos_norm != 0); });
}

int32_t bmx_pca_add_block(bmx_pca_t* p, const double* x_block, int64_t n_block) {
    return bmx::guarded([&] { bmx::live(p).add_block(x_block, n_block); });
}

int32_t bmx_pca_fit(bmx_pca_t* p, int32_t d, int32_t iters, double* centers, double* rotation, double* sdev) {
    return bmx::guarded([&] { bmx::live(p).fit(d, 0.0, iters, centers, rotation, sdev, nullptr, nullptr); });
}

int32_t bmx_pca_fit_tol(bmx_pca_t* p, int32_t d, double tol, int32_t max_iters, double* centers, double* rotation,
                        double* sdev, int32_t* iters_used, double* residual) {
    return bmx::guarded([&] {
        bmx::fit_to_tolerance(bmx::live(p), d, tol, max_iters, centers, rotation, sdev, iters_used, residual);
    });
}

int32_t bmx_pca_project(bmx_pca_t* p, int32_t batch, double* out) {
    return bmx::guarded([&] { bmx::live(p).project(batch, out); });
}

/* ---------------------------------------------------------------- bmx_pca_genes_* ------------------------------- */
int32_t bmx_pca_genes_create(int32_t n_genes_left, bmx_pca_t* fitted, bmx_pca_genes_t** out) {
    return bmx::guarded([&] {
        if (!out) throw bmx::Error(BMX_ERR_ARG, "null output pointer");
        if (n_genes_left < 0) throw bmx::Error(BMX_ERR_ARG, "the number of leftover genes is negative");
        *out = new bmx_pca_genes(n_genes_left, &bmx::live(fitted));
    });
}

void bmx_pca_genes_destroy(bmx_pca_genes_t* h) { delete h; }

int32_t bmx_pca_genes_begin_batch(bmx_pca_genes_t* h, int32_t batch) {
    return bmx::guarded([&] { bmx::live(h).begin_batch(batch); });
}

int32_t bmx_pca_genes_add_block(bmx_pca_genes_t* h, const double* x_left_block, int64_t n_block) {
    return bmx::guarded([&] { bmx::live(h).add_block(x_left_block, n_block); });
}

int32_t bmx_pca_genes_finish(bmx_pca_genes_t* h, double* centers_left, double* rotation_left) {
    return bmx::guarded([&] { bmx::live(h).finish(centers_left, rotation_left); });
}

int32_t bmx_pca_genes_total_variance(bmx_pca_genes_t* h, double* var_total) {
    return bmx::guarded([&] { bmx::live(h).total_variance(var_total); });
}

}  // extern "C"
