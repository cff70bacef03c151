// The host-only parts of the gene-variance handles under the host sanitizers (`make hostcheck`): the argument checks on
// good and bad blocks, and the chunk merge against a two-pass reference in long double.  Needs no device.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gene_var_host.hpp"

namespace {

int failures = 0;

template <class F>
void expect_throw(const char* what, F&& fn) {
    try {
        fn();
    } catch (const bmx::Error& e) {
        if (e.code == BMX_ERR_ARG) return;
    }
    std::printf("FAIL: %s was not refused\n", what);
    ++failures;
}

template <class F>
void expect_ok(const char* what, F&& fn) {
    try {
        fn();
    } catch (const std::exception& e) {
        std::printf("FAIL: %s was refused: %s\n", what, e.what());
        ++failures;
    }
}

// the chunked two-sweep reduction of x[0, n) as the kernels take it, merged in ascending order
bmx::GeneVarState chunked(const std::vector<double>& x) {
    bmx::GeneVarState s{0.0, 0.0, 0.0};
    for (size_t b = 0; b < x.size(); b += bmx::GENEVAR_CHUNK) {
        const size_t e = std::min(x.size(), b + (size_t)bmx::GENEVAR_CHUNK);
        double sum = 0.0, sq = 0.0;
        for (size_t i = b; i < e; ++i) sum += x[i];
        const double mean = sum / (double)(e - b);
        for (size_t i = b; i < e; ++i) sq += (x[i] - mean) * (x[i] - mean);
        s = bmx::genevar_merge(s, bmx::GeneVarState{(double)(e - b), mean, sq});
    }
    return s;
}

void check_merge(size_t n, double offset, double scale) {
    std::vector<double> x(n);
    unsigned long long r = 88172645463325252ull + n;
    for (double& v : x) {
        r ^= r << 13;
        r ^= r >> 7;
        r ^= r << 17;
        v = offset + scale * ((double)(r >> 11) / 9007199254740992.0 - 0.5);
    }
    long double sum = 0.0L, sq = 0.0L;
    for (double v : x) sum += v;
    const long double mean = sum / (long double)n;
    for (double v : x) sq += ((long double)v - mean) * ((long double)v - mean);
    const bmx::GeneVarState s = chunked(x);
    const double total = bmx::genevar_total(s);
    if (s.n != (double)n) {
        std::printf("FAIL: merged count %g for %zu cells\n", s.n, n);
        ++failures;
    }
    // The allowances of tests/model_gene_var_ref.py: gamma_k = k u / (1 - k u), K chunks; the mean within
    // gamma_(256 + 4 K) * max|x|, the squared deviations within gamma_(259 + 7 K) of themselves, and E, the error of a
    // difference of two means, enters M2 through the merge's delta: 2 sqrt(M2 n) E + n E^2.
    const double u = 1.1102230246251565e-16, K = std::ceil((double)n / bmx::GENEVAR_CHUNK);
    auto gamma = [&](double k) { return k * u / (1.0 - k * u); };
    double amax = 0.0;
    for (double v : x) amax = std::max(amax, std::fabs(v));
    const double mean_allow = gamma(256 + 4 * K) * amax, E = 2 * mean_allow;
    const double mean_err = std::fabs((double)((long double)s.mean - mean));
    if (mean_err > mean_allow) {
        std::printf("FAIL: mean of %zu cells off by %g\n", n, mean_err);
        ++failures;
    }
    if (n == 1) {
        if (!std::isnan(total)) {
            std::printf("FAIL: one cell should have a NaN variance\n");
            ++failures;
        }
        return;
    }
    const long double ref = sq / (long double)(n - 1);
    const double m2 = (double)sq;
    const double allow = (gamma(259 + 7 * K) * m2 + 2 * std::sqrt(m2 * (double)n) * E + (double)n * E * E) / (double)(n - 1);
    if (std::fabs((double)((long double)total - ref)) > allow) {
        std::printf("FAIL: variance of %zu cells %.17g, reference %.17Lg\n", n, total, ref);
        ++failures;
    }
}

}  // namespace

int main() {
    using namespace bmx;
    expect_ok("one gene", [] { genevar_check_create(1); });
    expect_ok("the most genes", [] { genevar_check_create(GENEVAR_MAX_GENES); });
    expect_throw("no gene", [] { genevar_check_create(0); });
    expect_throw("too many genes", [] { genevar_check_create(GENEVAR_MAX_GENES + 1); });

    expect_ok("a whole batch", [] { genevar_check_block(1000, 0, 1000); });
    expect_ok("a first block of whole chunks", [] { genevar_check_block(1000, 0, 512); });
    expect_ok("a last block", [] { genevar_check_block(1000, 768, 232); });
    expect_throw("a ragged first block", [] { genevar_check_block(1000, 0, 300); });
    expect_throw("a block past the batch", [] { genevar_check_block(1000, 768, 233); });
    expect_throw("an empty block", [] { genevar_check_block(1000, 0, 0); });
    expect_throw("a block of an empty batch", [] { genevar_check_block(0, 0, 1); });
    expect_throw("a negative fill", [] { genevar_check_block(1000, -256, 256); });
    expect_throw("a huge block", [] { genevar_check_block(1000, 256, INT64_MAX); });

    const int64_t indptr[4] = {0, 2, 2, 3};
    const int32_t indices[3] = {0, 4, 1};
    const double data[3] = {1.0, 2.0, 3.0};
    expect_ok("a sparse block", [&] { genevar_check_sparse_block(3, 0, 3, indptr, indices, data, 3); });
    expect_ok("a block without entries", [] {
        const int64_t empty[3] = {0, 0, 0};
        genevar_check_sparse_block(2, 0, 2, empty, nullptr, nullptr, 0);
    });
    expect_throw("a missing indptr", [&] { genevar_check_sparse_block(3, 0, 3, nullptr, indices, data, 3); });
    expect_throw("missing indices", [&] { genevar_check_sparse_block(3, 0, 3, indptr, nullptr, data, 3); });
    expect_throw("an indptr that ends elsewhere", [&] { genevar_check_sparse_block(3, 0, 3, indptr, indices, data, 2); });
    expect_throw("an indptr that decreases", [&] {
        const int64_t down[4] = {0, 2, 1, 3};
        genevar_check_sparse_block(3, 0, 3, down, indices, data, 3);
    });
    expect_throw("an indptr that starts late", [&] {
        const int64_t late[4] = {1, 2, 2, 3};
        genevar_check_sparse_block(3, 0, 3, late, indices, data, 3);
    });
    expect_throw("a ragged sparse block", [&] { genevar_check_sparse_block(1000, 0, 3, indptr, indices, data, 3); });

    for (size_t n : {1u, 2u, 255u, 256u, 257u, 513u, 5000u}) {
        check_merge(n, 0.0, 1.0);
        check_merge(n, 10.0, 1e-3);
        check_merge(n, 1e6, 1.0);
    }
    // an empty state in front changes no bit
    const GeneVarState b{7.0, 3.25, 0.125};
    const GeneVarState m = genevar_merge(GeneVarState{0.0, 0.0, 0.0}, b);
    if (m.n != b.n || m.mean != b.mean || m.m2 != b.m2) {
        std::printf("FAIL: an empty state in front changed the chunk\n");
        ++failures;
    }
    std::printf(failures ? "gene_var host check: %d failure(s)\n" : "gene_var host check: ok\n", failures);
    return failures ? 1 : 0;
}
