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
#include "pca_kernels.hpp"
#include "resident_batches.hpp"

namespace bmx {

// ---------------------------------------------------------------------------------------------------
struct PcaBatch : ResidentBatch {
    DevBuf<double> inv;  // [n] 1 / max(1e-8, l2), empty without cosine normalisation
    double weight = 1.0;
    bool cos_norm = false;
};

class Pca : ResidentBatches<PcaBatch> {
    friend class PcaGenes;  // the streaming pass over the genes outside subset.row borrows a fitted Pca (below)

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
            hipLaunchKernelGGL(inv_l2_kernel, dim3((unsigned)cdiv(m, 4)), dim3(256), 0, stream_, p, m, G_,
                               b.inv.p + (b.filled - m));
            BMX_LAUNCH_CHECK();
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
    // max_applies plain subspace steps (the fixed-count form).
    void fit(int d, double tol, int max_applies, double* centers, double* rotation, double* sdev, int* applies_used,
             double* resid_out) {
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        ++generation_;
        if (batches_.empty()) throw Error(BMX_ERR_ARG, "at least one batch must be specified");
        if (batches_.back()->filled != batches_.back()->n)
            throw Error(BMX_ERR_ARG, "the last batch has not received all its cells");
        if (d < 1 || d > 2 * PL - 8) throw Error(BMX_ERR_ARG, "the device PCA takes 1 <= d <= 120");
        if (d > G_) throw Error(BMX_ERR_ARG, "d exceeds the number of genes");
        if (max_applies < 1) throw Error(BMX_ERR_ARG, "the PCA needs at least one iteration");
        const int L = d <= PL - 8 ? PL : 2 * PL;
        int64_t ncells = 0;
        for (auto& bp : batches_) ncells += bp->n;
        if (G_ < L || ncells <= L)
            throw Error(BMX_ERR_ARG, "PCA: the data has rank below the subspace width (fewer genes or cells than the block)");
        L_ = L;
        d_ = d;
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
        // ---- starting block: a fixed pseudo-random G x L matrix, orthonormalised
        const size_t GL = (size_t)G * L;
        double* Q = q_.reserve(GL);
        double* Y = y_.reserve(GL);
        double* Xr = xr_.reserve(GL);  // Ritz vectors Q V
        double* Yr = yr_.reserve(GL);  // their images Y V
        double* W = w_.reserve(GL);    // filter scratch
        qt_.reserve((size_t)G * PL);
        small_.reserve((size_t)L * L * 3 + 4 * (size_t)L);
        {
            std::vector<double> h(GL);
            unsigned long long st = 0x9E3779B97F4A7C15ull;
            for (auto& v : h) {  // splitmix64 -> uniform in (-1, 1): any full-rank start will do
                st += 0x9E3779B97F4A7C15ull;
                unsigned long long z = st;
                z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
                z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
                z ^= z >> 31;
                v = (double)(z >> 11) * (1.0 / 4503599627370496.0) - 1.0;
            }
            BMX_HIP(hipMemcpyAsync(Y, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, stream_));
            BMX_HIP(hipStreamSynchronize(stream_));
        }
        orthonormalise(Y, Q);
        std::vector<double>& theta = theta_;  // kept: the eigenvalues s^2 the leftover rotation is divided by
        theta.assign(L, 0.0);
        std::vector<double> V;
        std::vector<int> order(L);
        int applies = 0;
        double resid = std::numeric_limits<double>::infinity();
        const bool fixed = !(tol > 0.0);
        for (;;) {
            apply_operator(Q, Y);  // Y = M Q
            ++applies;
            const bool last_fixed = fixed && applies >= max_applies;
            if (fixed && !last_fixed) {  // plain subspace iteration, no convergence test
                orthonormalise(Y, Q);
                continue;
            }
            // ---- Rayleigh-Ritz on (Q, Y = M Q): T = Q^T Y = V diag(theta) V^T; Ritz vectors Xr = Q V, images Yr = Y V
            rayleigh_ritz(Q, Y, theta, V, order);
            rotate(Q, V, order, Xr);
            rotate(Y, V, order, Yr);
            resid = residual(Yr, Xr, theta, d);
            if (last_fixed || resid <= tol || applies >= max_applies) break;
            // ---- next block: p(M) Xr with p the Chebyshev polynomial that is bounded on [0, theta_L] (everything the
            // block does not want) and grows above it; the degree is capped so that the largest wanted direction
            // outgrows the smallest by at most ~1e5 (Cholesky QR squares the block's condition number)
            const double lam = theta[0], cut = theta[L - 1];
            int deg = 1;
            if (cut > 0.0 && lam > cut * (1.0 + 1e-12)) {
                const double x = 2.0 * lam / cut - 1.0;  // (lam - c) / e with c = e = cut / 2
                deg = (int)std::floor(std::log(1e5) / std::acosh(x));
                deg = std::max(1, std::min({deg, 12, max_applies - applies + 1}));
            }
            if (deg <= 1) {
                orthonormalise(Yr, Q);  // plain step from the Ritz basis (same subspace as Y)
                continue;
            }
            // scaled three-term recurrence (p(lam) = 1):
            //   X0 = Xr, X1 = (s1 / e)(M - c) X0, X_{i+1} = 2 (s_{i+1} / e)(M - c) X_i - s_i s_{i+1} X_{i-1}
            const double c = 0.5 * cut, e = 0.5 * cut;
            const double sg1 = e / (lam - c);
            double sg = sg1;
            const int64_t nel = (int64_t)GL;
            const unsigned nblk = (unsigned)cdiv(nel, 256);
            double* X0 = Xr;
            double* X1 = W;
            hipLaunchKernelGGL(lincomb3, dim3(nblk), dim3(256), 0, stream_, X1, sg1 / e, (const double*)Yr, -c * sg1 / e,
                               (const double*)Xr, 0.0, (const double*)nullptr, nel);
            BMX_LAUNCH_CHECK();
            double* spare = Yr;  // Yr is free once X1 exists
            for (int i = 2; i <= deg; ++i) {
                const double sg2 = 1.0 / (2.0 / sg1 - sg);
                apply_operator(X1, Y);  // Y = M X1
                ++applies;
                hipLaunchKernelGGL(lincomb3, dim3(nblk), dim3(256), 0, stream_, spare, 2.0 * sg2 / e, (const double*)Y,
                                   -2.0 * c * sg2 / e, (const double*)X1, -sg * sg2, (const double*)X0, nel);
                BMX_LAUNCH_CHECK();
                double* t = X0;
                X0 = X1;
                X1 = spare;
                spare = t;
                sg = sg2;
            }
            orthonormalise(X1, Q);
        }
        // ---- results: rotation = the first d Ritz vectors
        double* Ut = ut_.reserve(GL);  // [L][G]: the B operand of the projection
        for (int h = 0; h < L / PL; ++h) {
            hipLaunchKernelGGL(transpose64, dim3((unsigned)cdiv(G, 64)), dim3(256), 0, stream_, (const double*)(Xr + h * PL),
                               (int64_t)L, (int64_t)G, Ut + (size_t)h * PL * G);
            BMX_LAUNCH_CHECK();
        }
        // mu . u_j for the projection's centring
        double* muU = small_.p + (size_t)3 * L * L;
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
        if (sdev)
            for (int j = 0; j < d; ++j) sdev[j] = std::sqrt(std::max(0.0, theta[j]));
        if (applies_used) *applies_used = applies;
        if (resid_out) *resid_out = resid;
        fitted_ = true;
        if (!fixed && !(resid <= tol)) {
            char msg[256];
            std::snprintf(msg, sizeof(msg),
                          "PCA: the subspace iteration did not reach the tolerance within %d applications of the operator "
                          "(relative residual %.3g, tolerance %.3g)", applies, resid, tol);
            throw Error(BMX_ERR_ARG, msg);
        }
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
        double* muU = small_.p + (size_t)3 * L_ * L_;
        for (int h = 0; h * PL < d_; ++h) {
            hipLaunchKernelGGL(gemm_nt64, dim3((unsigned)cdiv(B.n, 64)), dim3(256), 0, stream_, (const double*)B.x.p, B.n, G_,
                               (int64_t)G_, (const double*)(ut_.p + (size_t)h * PL * G_), (int64_t)G_,
                               (const double*)(B.cos_norm ? B.inv.p : nullptr), (const double*)(muU + h * PL), Z, (int64_t)PL);
            BMX_LAUNCH_CHECK();
            hipLaunchKernelGGL(transpose64, dim3((unsigned)cdiv(B.n, 64)), dim3(256), 0, stream_, (const double*)Z, (int64_t)PL,
                               B.n, Zt);
            BMX_LAUNCH_CHECK();
            const int cols = std::min(PL, d_ - h * PL);
            BMX_HIP(hipMemcpyAsync(out + (size_t)h * PL * B.n, Zt, (size_t)B.n * cols * sizeof(double), hipMemcpyDeviceToHost,
                                   stream_));
            BMX_HIP(hipStreamSynchronize(stream_));  // Z / Zt are reused by the next half
        }
    }
    int nbatches() const { return (int)batches_.size(); }
    int64_t ncells(int b) const { return batches_[b]->n; }

  private:
    // out [L][L] row-major = A^T B for A, B [rows][L]
    void product_tn(const double* A, const double* Bm, int64_t rows, double* out) {
        const int L = L_;
        const int nsplit = (int)std::min<int64_t>(256, std::max<int64_t>(1, rows / 512));
        const int64_t per = round_up((rows + nsplit - 1) / nsplit, KC);
        double* part = part_.reserve((size_t)nsplit * L * PL);
        for (int h = 0; h < L / PL; ++h) {  // 64 columns of B at a time
            hipLaunchKernelGGL(gemm_tn64, dim3(L / PL, nsplit), dim3(256), 0, stream_, A, rows, L, (int64_t)L, Bm + h * PL,
                               (int64_t)L, (const double*)nullptr, per, part);
            hipLaunchKernelGGL(reduce_parts, dim3((unsigned)cdiv(L * PL, 256)), dim3(256), 0, stream_, (const double*)part,
                               nsplit, (int64_t)L * PL, 1.0, 0.0, out + h * PL, PL, (int64_t)L);
            BMX_LAUNCH_CHECK();
        }
    }
    // dst [G][L] = src [G][L] * Bt^T for a host matrix Bt [L][L] row-major (dst[g][j] = sum_i src[g][i] Bt[j][i])
    void times_small(const double* src, const std::vector<double>& Bt, double* dst) {
        const int L = L_;
        double* dB = small_.p + (size_t)L * L;
        BMX_HIP(hipMemcpyAsync(dB, Bt.data(), Bt.size() * sizeof(double), hipMemcpyHostToDevice, stream_));
        for (int h = 0; h < L / PL; ++h) {
            hipLaunchKernelGGL(gemm_nt64, dim3((unsigned)cdiv(G_, 64)), dim3(256), 0, stream_, src, (int64_t)G_, L, (int64_t)L,
                               (const double*)(dB + (size_t)h * PL * L), (int64_t)L, (const double*)nullptr,
                               (const double*)nullptr, dst + h * PL, (int64_t)L);
            BMX_LAUNCH_CHECK();
        }
        BMX_HIP(hipStreamSynchronize(stream_));  // Bt may go out of scope
    }
    // Q = Y R^-1 with R^T R = Y^T Y, twice (Cholesky QR 2: orthonormal to rounding for any reasonable Y).  Y is
    // overwritten (it holds the first pass's result).
    void orthonormalise(double* Y, double* Q) {
        const int L = L_;
        double* S = small_.p;
        double* src = Y;
        double* dst = Q;
        for (int pass = 0; pass < 2; ++pass) {
            product_tn(src, src, (int64_t)G_, S);
            std::vector<double> h((size_t)L * L);
            BMX_HIP(hipMemcpyAsync(h.data(), S, h.size() * sizeof(double), hipMemcpyDeviceToHost, stream_));
            BMX_HIP(hipStreamSynchronize(stream_));
            if (!cholesky_upper(h, L)) throw Error(BMX_ERR_ARG, "PCA: the data has rank below the subspace width");
            invert_upper(h, L);  // Rinv (upper); Q[g][j] = sum_i Y[g][i] Rinv[i][j] -> Bt[j][i] = Rinv[i][j]
            std::vector<double> bt((size_t)L * L);
            for (int i = 0; i < L; ++i)
                for (int j = 0; j < L; ++j) bt[(size_t)j * L + i] = h[(size_t)i * L + j];
            times_small(src, bt, dst);
            std::swap(src, dst);
        }
        // two passes: Y -> Q -> Y; the result is back in Y's storage, bring it to Q
        BMX_HIP(hipMemcpyAsync(Q, Y, (size_t)G_ * L * sizeof(double), hipMemcpyDeviceToDevice, stream_));
    }
    void rayleigh_ritz(const double* Q, const double* Y, std::vector<double>& theta, std::vector<double>& V,
                       std::vector<int>& order) {
        const int L = L_;
        double* T = small_.p;
        product_tn(Q, Y, (int64_t)G_, T);
        std::vector<double> hT((size_t)L * L);
        BMX_HIP(hipMemcpyAsync(hT.data(), T, hT.size() * sizeof(double), hipMemcpyDeviceToHost, stream_));
        BMX_HIP(hipStreamSynchronize(stream_));
        for (int i = 0; i < L; ++i)
            for (int j = i + 1; j < L; ++j) {
                const double v = 0.5 * (hT[(size_t)i * L + j] + hT[(size_t)j * L + i]);
                hT[(size_t)i * L + j] = hT[(size_t)j * L + i] = v;
            }
        jacobi_eigen(hT, V, L);
        for (int i = 0; i < L; ++i) order[i] = i;
        std::sort(order.begin(), order.end(), [&](int a, int b) { return hT[(size_t)a * L + a] > hT[(size_t)b * L + b]; });
        for (int j = 0; j < L; ++j) theta[j] = hT[(size_t)order[j] * L + order[j]];
    }
    // dst = src V with the columns of V taken in `order`
    void rotate(const double* src, const std::vector<double>& V, const std::vector<int>& order, double* dst) {
        const int L = L_;
        std::vector<double> Bt((size_t)L * L);
        for (int j = 0; j < L; ++j)
            for (int i = 0; i < L; ++i) Bt[(size_t)j * L + i] = V[(size_t)i * L + order[j]];
        times_small(src, Bt, dst);
    }
    // max_j<d |Yr_j - theta_j Xr_j| / theta_0
    double residual(const double* Yr, const double* Xr, const std::vector<double>& theta, int d) {
        const int L = L_;
        double* dth = small_.p + (size_t)3 * L * L + L;
        double* dres = dth + L;
        BMX_HIP(hipMemcpyAsync(dth, theta.data(), (size_t)L * sizeof(double), hipMemcpyHostToDevice, stream_));
        const int nb = cdiv(G_, 256);
        double* part = part_.reserve((size_t)nb * L);
        hipLaunchKernelGGL(resid_partial, dim3(nb), dim3(256), 0, stream_, Yr, Xr, (const double*)dth, (int64_t)G_, L, part);
        hipLaunchKernelGGL(reduce_parts, dim3((unsigned)cdiv(L, 256)), dim3(256), 0, stream_, (const double*)part, nb, (int64_t)L,
                           1.0, 0.0, dres, L, (int64_t)L);
        BMX_LAUNCH_CHECK();
        std::vector<double> h(L);
        BMX_HIP(hipMemcpyAsync(h.data(), dres, (size_t)L * sizeof(double), hipMemcpyDeviceToHost, stream_));
        BMX_HIP(hipStreamSynchronize(stream_));
        double worst = 0.0;
        for (int j = 0; j < d; ++j) worst = std::max(worst, std::sqrt(std::max(0.0, h[j])));
        return theta[0] > 0.0 ? worst / theta[0] : 0.0;
    }
    // Y = M Q = sum_b (w_b / n_b) C_b C_b^T Q for a block of L vectors, 64 at a time
    void apply_operator(const double* Q, double* Y) {
        const int G = G_, L = L_;
        double* Qt = qt_.p;
        BMX_HIP(hipMemsetAsync(Y, 0, (size_t)G * L * sizeof(double), stream_));
        for (int h = 0; h < L / PL; ++h) {
            hipLaunchKernelGGL(transpose64, dim3((unsigned)cdiv(G, 64)), dim3(256), 0, stream_, Q + h * PL, (int64_t)L, (int64_t)G,
                               Qt);
            BMX_LAUNCH_CHECK();
            double* muQ = small_.p + (size_t)2 * L * L;
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
                double* part = part_.reserve((size_t)nsplit * G * PL + (size_t)4096 * PL + PL);
                hipLaunchKernelGGL(gemm_tn64, dim3(gtiles, nsplit), dim3(256), 0, stream_, (const double*)b.x.p, b.n, G, (int64_t)G,
                                   (const double*)Z, (int64_t)PL, rs, per, part);
                hipLaunchKernelGGL(reduce_parts, dim3((unsigned)cdiv((int64_t)G * PL, 256)), dim3(256), 0, stream_,
                                   (const double*)part, nsplit, (int64_t)G * PL, coef, 1.0, Yh, PL, (int64_t)L);
                BMX_LAUNCH_CHECK();
                // column sums of Z (no row factor: the centring term is mu 1^T Z)
                const int nb = (int)std::min<int64_t>(4096, std::max<int64_t>(1, b.n / 256));
                const int64_t rpb = (b.n + nb - 1) / nb;
                double* zpart = part + (size_t)nsplit * G * PL;
                double* zsum = zpart + (size_t)nb * PL;
                hipLaunchKernelGGL(colsum64_partial, dim3(nb), dim3(256), 0, stream_, (const double*)Z, (const double*)nullptr,
                                   b.n, rpb, zpart);
                hipLaunchKernelGGL(reduce_parts, dim3(1), dim3(64), 0, stream_, (const double*)zpart, nb, (int64_t)PL, 1.0, 0.0,
                                   zsum, PL, (int64_t)PL);
                hipLaunchKernelGGL(rank1_sub, dim3((unsigned)cdiv((int64_t)G * PL, 256)), dim3(256), 0, stream_, Yh, (int64_t)L,
                                   (const double*)mu_.p, (const double*)zsum, coef, G);
                BMX_LAUNCH_CHECK();
            }
        }
    }

    int d_ = 0, L_ = PL;
    std::vector<double> theta_;          // [L] Ritz values of the last fit, descending
    unsigned long long generation_ = 0;  // counts begin_batch and fit: what a PcaGenes was made for
    DevBuf<double> mu_, q_, y_, xr_, yr_, w_, qt_, ut_, z_, zt_, part_, small_;
    bool fitted_ = false;
};

// ---------------------------------------------------------------------------------------------------
// The genes outside subset.row (R/multiBatchPCA.R:401-414, .make_pca_metadata with get.all.genes): their centres mu_L and
// rotation rows  U_L = L_scaled V diag(1 / s),  V = S_scaled^T U diag(1 / s),  which with coef_b = w_b / n_b is
//     U_L[g][j] = ( sum_b coef_b sum_c scale_c x_gc Z_b[c][j]  -  mu_L[g] sum_b coef_b sum_c Z_b[c][j] ) / s_j^2,
// Z_b = C_b^T U the batch's projections.  The leftover rows of every batch stream through in column blocks and are not
// kept: a block lands in one of two device buffers on the copy stream while the kernels of the block before it run on the
// other.  The projections of a block's cells come from the RESIDENT subset rows of the borrowed, fitted Pca (gemm_nt64 on
// its ut_ / muU, as Pca::project), so nothing but the leftover rows crosses the link.  scale is the batch's inv: the norms
// over the subset rows (R/fastMNN.R:348-351).  The Pca must outlive this handle; one that was re-fitted or given another
// batch since makes every later call an error.
// ---------------------------------------------------------------------------------------------------
class PcaGenes {
  public:
    PcaGenes(int GL, Pca* pca) : pca_(*pca), made_for_(pca->generation_), GL_(GL), device_(pca->device_) {
        if (!pca_.fitted_) throw Error(BMX_ERR_ARG, "bmx_pca_fit has not been run");
        nh_ = cdiv(pca_.d_, PL);
        for (auto& bp : pca_.batches_) wsum_ += bp->weight;
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
        ledger_.n = pca_.ncells(b);
        ledger_.filled = 0;
    }
    // the next m cells of the batch begun last: x_left_block is GL x m column-major host memory
    void add_block(const double* x_left_block, int64_t m) {
        check_fresh();
        check_block(batch_ < 0 ? nullptr : &ledger_, x_left_block, m, "bmx_pca_genes_begin_batch");
        if (GL_ < 1) throw Error(BMX_ERR_ARG, "the handle was made for no leftover genes");
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        PcaBatch& B = *pca_.batches_[(size_t)batch_];
        const int64_t first = ledger_.filled;
        const double coef = B.weight / (double)B.n;
        const double* rs = B.cos_norm ? B.inv.p + first : nullptr;
        const int G = GL_, GS = pca_.G_;
        // ---- the shapes of this block's launches
        const int gtiles = cdiv(G, 64);
        int nsplit = (int)std::min<int64_t>(std::max<int64_t>(1, (int64_t)1024 / gtiles), std::max<int64_t>(1, m / 2048));
        const int64_t per = round_up((m + nsplit - 1) / nsplit, KC);
        nsplit = (int)((m + per - 1) / per);
        const int nb = (int)std::min<int64_t>(4096, std::max<int64_t>(1, m / 256));
        const int64_t rpb = (m + nb - 1) / nb;
        if (m > cap_) {  // (a grown buffer may change hands: nothing of ours is in flight when it does)
            BMX_HIP(hipStreamSynchronize(copy_));
            BMX_HIP(hipStreamSynchronize(stream_));
            for (int i = 0; i < 2; ++i) xl_[i].reserve((size_t)m * G);
            z_.reserve((size_t)nh_ * m * PL);
            cap_ = m;
            busy_[0] = busy_[1] = false;
        }
        double* part = part_.reserve((size_t)nsplit * nh_ * G * PL + (size_t)nsplit * G + (size_t)nb * PL);
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
        const double* muU = pca_.small_.p + (size_t)3 * pca_.L_ * pca_.L_;
        const int64_t zhalf = (int64_t)cap_ * PL;
        for (int h = 0; h < nh_; ++h) {
            hipLaunchKernelGGL(gemm_nt64, dim3((unsigned)cdiv(m, 64)), dim3(256), 0, stream_,
                               (const double*)(B.x.p + first * GS), m, GS, (int64_t)GS,
                               (const double*)(pca_.ut_.p + (size_t)h * PL * GS), (int64_t)GS, rs,
                               (const double*)(muU + h * PL), z_.p + h * zhalf, (int64_t)PL);
            hipLaunchKernelGGL(colsum64_partial, dim3(nb), dim3(256), 0, stream_, (const double*)(z_.p + h * zhalf),
                               (const double*)nullptr, m, rpb, zpart);
            hipLaunchKernelGGL(reduce_parts, dim3(1), dim3(64), 0, stream_, (const double*)zpart, nb, (int64_t)PL, coef, 1.0,
                               tsum_.p + h * PL, PL, (int64_t)PL);
            BMX_LAUNCH_CHECK();
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
        const int d = pca_.d_, G = GL_;
        std::vector<double> s2((size_t)d);
        for (int j = 0; j < d; ++j) {
            const double sd = std::sqrt(std::max(0.0, pca_.theta_[(size_t)j]));  // the sdev fit reports
            s2[(size_t)j] = sd * sd;
        }
        double* ds2 = tsum_.p + (size_t)nh_ * PL;
        BMX_HIP(hipMemcpyAsync(ds2, s2.data(), (size_t)d * sizeof(double), hipMemcpyHostToDevice, stream_));
        double* rot = part_.reserve((size_t)G * d);  // (the stream orders this after the last block's reductions)
        hipLaunchKernelGGL(genes_rotation, dim3((unsigned)cdiv((int64_t)G * d, 256)), dim3(256), 0, stream_,
                           (const double*)acc_.p, (const double*)mu_.p, (const double*)tsum_.p, (const double*)ds2, G, d, rot);
        BMX_LAUNCH_CHECK();
        if (centers_left)
            BMX_HIP(hipMemcpyAsync(centers_left, mu_.p, (size_t)G * sizeof(double), hipMemcpyDeviceToHost, stream_));
        if (rotation_left)
            BMX_HIP(hipMemcpyAsync(rotation_left, rot, (size_t)G * d * sizeof(double), hipMemcpyDeviceToHost, stream_));
        BMX_HIP(hipStreamSynchronize(stream_));
    }
    // sum_b coef_b |C_b|_F^2 over the resident (subset) rows, in the centred form; the caller divides by the batches
    void total_variance(double* var_total) {
        check_fresh();
        if (!var_total) throw Error(BMX_ERR_ARG, "null output pointer");
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        double total = 0.0;
        for (auto& bp : pca_.batches_) {
            PcaBatch& B = *bp;
            const int nb = (int)std::min<int64_t>(1024, std::max<int64_t>(1, B.n / 64));
            const int64_t cpb = (B.n + nb - 1) / nb;
            BMX_HIP(hipStreamSynchronize(stream_));  // part_ may grow
            double* part = part_.reserve((size_t)nb);
            hipLaunchKernelGGL(centred_sq_partial, dim3(nb), dim3(256), 0, stream_, (const double*)B.x.p,
                               (const double*)(B.cos_norm ? B.inv.p : nullptr), (const double*)pca_.mu_.p, B.n, pca_.G_, cpb,
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
        if (pca_.generation_ != made_for_ || !pca_.fitted_)
            throw Error(BMX_ERR_ARG, "the PCA was re-fitted or given a batch after bmx_pca_genes_create");
    }

    DevBlockCache cache_;  // first: destroyed after every DevBuf below (see ResidentBatches::retire)
    Pca& pca_;
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
        if (!(tol > 0.0)) throw bmx::Error(BMX_ERR_ARG, "the PCA tolerance must be positive");
        int used = 0;
        double res = 0.0;
        try {
            bmx::live(p).fit(d, tol, max_iters, centers, rotation, sdev, &used, &res);
        } catch (...) {
            if (iters_used) *iters_used = used;
            if (residual) *residual = res;
            throw;
        }
        if (iters_used) *iters_used = used;
        if (residual) *residual = res;
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
