// The eigen-solver of multiBatchPCA, once for the dense handle (pca.hip) and the sparse one (pca_sparse.hip):
// Chebyshev-filtered subspace iteration on a block of L = 64 or 128 vectors over [rows][L] row-major blocks -- the start
// block, Cholesky QR 2, Rayleigh-Ritz, the filter and its degree cap, the residual -- on the kernels of pca_kernels.hpp.
// A handle brings its operator Y = M Q as a callable and keeps what is its own: the grand centre, the rotation
// transposed, the mu . u_j offsets, the projections.  SubspaceIteration owns the buffers only the iteration uses; none of
// its scratch is shared with a handle.  Unnamed namespace, as pca_kernels.hpp: each of the two files gets its own copy.
#pragma once
#include <cstdio>
#include <limits>

#include "pca_kernels.hpp"

namespace bmx {
namespace {

class SubspaceIteration {
  public:
    struct Outcome {
        int applies;   // applications of the operator
        double resid;  // max_j<d |M x_j - theta_j x_j| / theta_1 at the last Rayleigh-Ritz step
    };

    // The checks of fit's arguments; returns the block width L: 64 (d <= 56) or 128 (d <= 120).
    static int width_for(int d, int rows, int64_t cells, int max_applies) {
        if (d < 1 || d > 2 * PL - 8) throw Error(BMX_ERR_ARG, "the device PCA takes 1 <= d <= 120");
        if (d > rows) throw Error(BMX_ERR_ARG, "d exceeds the number of genes");
        if (max_applies < 1) throw Error(BMX_ERR_ARG, "the PCA needs at least one iteration");
        const int L = width(d);
        if (rows < L || cells <= L)
            throw Error(BMX_ERR_ARG, "PCA: the data has rank below the subspace width (fewer genes or cells than the block)");
        return L;
    }

    // The d leading eigenpairs of the symmetric positive semi-definite M of order `rows`; apply(Q, Y) queues Y = M Q on
    // `stream` for [rows][L()] blocks.  tol > 0: until the Ritz residuals of the d wanted pairs are <= tol, at most
    // max_applies applications; else exactly max_applies plain subspace steps.  (d, rows, max_applies) have passed
    // width_for.  Throws when the block loses rank.
    template <class Apply>
    Outcome run(hipStream_t stream, int rows, int d, double tol, int max_applies, Apply&& apply) {
        stream_ = stream;
        rows_ = rows;
        d_ = d;
        const int L = L_ = width(d);
        // ---- starting block: a fixed pseudo-random rows x L matrix, orthonormalised
        const size_t GL = (size_t)rows * L;
        double* Q = q_.reserve(GL);
        double* Y = y_.reserve(GL);
        double* Xr = xr_.reserve(GL);  // Ritz vectors Q V
        double* Yr = yr_.reserve(GL);  // their images Y V
        double* W = w_.reserve(GL);    // filter scratch
        small_.reserve((size_t)L * L * 2 + 2 * (size_t)L);
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
        std::vector<double>& theta = theta_;
        theta.assign(L, 0.0);
        std::vector<double> V;
        std::vector<int> order(L);
        int applies = 0;
        double resid = std::numeric_limits<double>::infinity();
        const bool fixed = !(tol > 0.0);
        for (;;) {
            apply(Q, Y);  // Y = M Q
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
                apply(X1, Y);  // Y = M X1
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
        return {applies, resid};
    }

    // ---- what the last run left
    const double* ritz_vectors() const { return xr_.p; }       // [rows][L] row-major, the first d columns wanted
    const std::vector<double>& theta() const { return theta_; }  // [L] Ritz values (eigenvalues s^2), descending
    int L() const { return L_; }
    int d() const { return d_; }

    // The last step of a fit, after the handle has written its own results: sdev [d] (singular values of the scaled
    // matrix), the counts, and the error of a run that did not reach its tolerance.  The pointers may be null.
    void report(double tol, const Outcome& o, double* sdev, int* applies_used, double* resid_out) const {
        if (sdev)
            for (int j = 0; j < d_; ++j) sdev[j] = std::sqrt(std::max(0.0, theta_[j]));
        if (applies_used) *applies_used = o.applies;
        if (resid_out) *resid_out = o.resid;
        if (tol > 0.0 && !(o.resid <= tol)) {
            char msg[256];
            std::snprintf(msg, sizeof(msg),
                          "PCA: the subspace iteration did not reach the tolerance within %d applications of the operator "
                          "(relative residual %.3g, tolerance %.3g)", o.applies, o.resid, tol);
            throw Error(BMX_ERR_ARG, msg);
        }
    }

  private:
    static int width(int d) { return d <= PL - 8 ? PL : 2 * PL; }
    // out [L][L] row-major = A^T B for A, B [rows][L]
    void product_tn(const double* A, const double* Bm, double* out) {
        const int L = L_;
        const int64_t rows = rows_;
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
    // dst [rows][L] = src [rows][L] * Bt^T for a host matrix Bt [L][L] row-major (dst[g][j] = sum_i src[g][i] Bt[j][i])
    void times_small(const double* src, const std::vector<double>& Bt, double* dst) {
        const int L = L_;
        double* dB = small_.p + (size_t)L * L;
        BMX_HIP(hipMemcpyAsync(dB, Bt.data(), Bt.size() * sizeof(double), hipMemcpyHostToDevice, stream_));
        for (int h = 0; h < L / PL; ++h) {
            hipLaunchKernelGGL(gemm_nt64, dim3((unsigned)cdiv(rows_, 64)), dim3(256), 0, stream_, src, (int64_t)rows_, L,
                               (int64_t)L, (const double*)(dB + (size_t)h * PL * L), (int64_t)L, (const double*)nullptr,
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
            product_tn(src, src, S);
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
        BMX_HIP(hipMemcpyAsync(Q, Y, (size_t)rows_ * L * sizeof(double), hipMemcpyDeviceToDevice, stream_));
    }
    void rayleigh_ritz(const double* Q, const double* Y, std::vector<double>& theta, std::vector<double>& V,
                       std::vector<int>& order) {
        const int L = L_;
        double* T = small_.p;
        product_tn(Q, Y, T);
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
        double* dth = small_.p + (size_t)2 * L * L;
        double* dres = dth + L;
        BMX_HIP(hipMemcpyAsync(dth, theta.data(), (size_t)L * sizeof(double), hipMemcpyHostToDevice, stream_));
        const int nb = cdiv(rows_, 256);
        double* part = part_.reserve((size_t)nb * L);
        hipLaunchKernelGGL(resid_partial, dim3(nb), dim3(256), 0, stream_, Yr, Xr, (const double*)dth, (int64_t)rows_, L, part);
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

    hipStream_t stream_ = nullptr;  // of the run in progress
    int rows_ = 0, d_ = 0, L_ = PL;
    std::vector<double> theta_;
    // the blocks [rows][L]; part_: the split partials of product_tn and residual; small_: S / T [L][L], the small factor
    // on its way to times_small [L][L], theta [L], the squared residuals [L]
    DevBuf<double> q_, y_, xr_, yr_, w_, part_, small_;
};

// The body of a *_fit_tol entry point: iters_used / residual (nullable) are written whether fit returns or throws.
template <class Handle>
void fit_to_tolerance(Handle& h, int d, double tol, int max_iters, double* centers, double* rotation, double* sdev,
                      int32_t* iters_used, double* residual) {
    if (!(tol > 0.0)) throw Error(BMX_ERR_ARG, "the PCA tolerance must be positive");
    int used = 0;
    double res = 0.0;
    auto write = [&] {
        if (iters_used) *iters_used = used;
        if (residual) *residual = res;
    };
    try {
        h.fit(d, tol, max_iters, centers, rotation, sdev, &used, &res);
    } catch (...) {
        write();
        throw;
    }
    write();
}

}  // namespace
}  // namespace bmx
