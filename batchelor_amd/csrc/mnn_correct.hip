// mnnCorrect() on the device: .mnn_correct / .mnn_correct_core (R/mnnCorrect.R:179-393) with .prepare_input_data
// (:398-445), in gene space.  The host decides the merge order and sizes; every cell x gene value stays in HBM from upload
// to download.
//
// Memory: the input-gene matrix In [N][Gs] (and, when the output genes differ -- same.set false -- the output-gene matrix
// Out [N][Go]) is one pool whose rows are the cells in the binarised tree's left-to-right leaf order.  Every node of the
// predefined tree is then a contiguous slice, the two children of a merge are adjacent slices, and rbind(left, right)
// (:357) costs nothing.  A merge:
//   1. .restricted_mnn (R/MNN_tree.R:113-138) through Engine::find_mnn on views of the two slices;
//   2. the pairs (:298), 1-based rows in the nodes;
//   3. .compute_correction_vectors (:451-460): averaging (average_correction, the wide form above 256 genes), then
//      smooth_gaussian_kernel_device with the weights from the right node's input-gene rows, for correction.in and
//      correction.out alike (:300-304);
//   4. var.adj (:331-342, :462-481): adjust_shift_variance_device on the input genes, and on the subset.row genes of the
//      output matrix for correction.out; both take the nodes' restrict lists;
//   5. right += pmax(scaling, 1) * correction in place (:345-348), .combine_restrict on the host.
// The pairs are reindexed and the rows put back in input order at the end (:364-381).
//
// Batches given as CSC (bmx_mnn_correct_sparse) differ in .prepare_input_data alone: one batch's CSC at a time goes up and
// csc_expand_kernel writes its pool rows from the stored entries -- the subset.row genes, and all genes only for the
// output matrix of correct.all.  The merges then run on the bits the dense call would have made of toarray().
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "bmx_common.hpp"
#include "bmx_ops.hpp"
#include "csc_device.hpp"
#include "engine.hpp"
#include "host_xfer.hpp"
#include "merge_plan.hpp"
#include "mnn_correct.hpp"
#include "ordered_sums.hpp"
#include "resident_batches.hpp"

namespace bmx {
namespace {

// Pool rows straight from ONE batch's CSC (bmx_mnn_correct_sparse): indptr [m + 1] from 0, idx / val the batch's stored
// entries, dst [m][W] the batch's slice of the pool.  One wave a cell c, four cells a workgroup:
//   dst[c * W + j] = 0.0 + the stored value of row rows[j] (rows null: of row j) in column c, else +0.0
// which are toarray()'s bits: scipy adds the entries into a matrix of zeros, so a stored -0.0 comes out as +0.0 there and
// here, and every other value as it is.  l2 (nullable, the slice's norms): every element is divided by
// cos_clamp(l2[c]), apply_cosnorm_kernel's expression, so the bits are that kernel's.
// The wave first takes every stored entry of the column once, lane l the entries l, l + 64, ..., for the pattern flags
// (csc_entry_flags, to flags[CSC_F_ROW] / flags[CSC_F_ORDER]).  Then
//   SEARCH   lane l takes the positions l, l + 64, ... of the row and finds each by first_row_at_least: coalesced stores,
//            every element written once by one lane, rows that repeat or come in any order cost nothing.  A row index
//            out of memory is only ever compared, never an address; rows[] is the host's (checked there).
//   !SEARCH  (rows null, W = G) the slice has been zeroed by hipMemsetAsync on the same stream, and the walk over the
//            entries stores each at its row -- an entry whose row is outside [0, G) is left out.  Rows are unique in a
//            canonical column: no two lanes meet; a column where they do is flagged and the call ends with that error.
//            A cell whose norm is NaN takes the search form, which writes 0 / NaN where the memset left +0.
template <bool SEARCH>
__global__ __launch_bounds__(256) void csc_expand_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                         const double* __restrict__ val, int G, int64_t m,
                                                         const int32_t* __restrict__ rows, int W,
                                                         const double* __restrict__ l2, double* __restrict__ dst,
                                                         int32_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= m) return;  // (a whole wave leaves)
    const int64_t kb = wave_uniform(indptr[c]), ke = wave_uniform(indptr[c + 1]);
    const double L = l2 ? cos_clamp(l2[c]) : 1.0;
    const bool search = SEARCH || L != L;
    double* out = dst + c * W;
    int bad_row = 0, bad_order = 0;
    for (int64_t k = kb + lane; k < ke; k += 64) {
        const int32_t r = idx[k];
        if (csc_entry_flags(idx, k, kb, r, G, bad_row, bad_order) || search) continue;
        const double v = 0.0 + val[k];
        out[r] = l2 ? v / L : v;
    }
    if (search)
        for (int j = lane; j < W; j += 64) {
            const int g = rows ? rows[j] : j;
            const int64_t p = first_row_at_least(idx, kb, ke, g);
            double v = 0.0;
            if (p < ke && idx[p] == g) v += val[p];
            out[j] = l2 ? v / L : v;
        }
    if (bad_row) flags[CSC_F_ROW] = 1;
    if (bad_order) flags[CSC_F_ORDER] = 1;
}

// rows null: all G rows in order (W = G), the scatter form; else the search form over rows [W] (0-based, inside [0, G))
void expand_csc(hipStream_t s, const int64_t* indptr, const int32_t* idx, const double* val, int G, int64_t m,
                const int32_t* rows, int W, const double* l2, double* dst, int32_t* flags) {
    if (!rows && W != G) throw Error(BMX_ERR_ARG, "internal: the scatter form writes all genes");
    const dim3 grid((unsigned)((m + 3) / 4));
    if (rows) {
        hipLaunchKernelGGL(csc_expand_kernel<true>, grid, dim3(256), 0, s, indptr, idx, val, G, m, rows, W, l2, dst, flags);
    } else {
        BMX_HIP(hipMemsetAsync(dst, 0, (size_t)m * W * sizeof(double), s));
        hipLaunchKernelGGL(csc_expand_kernel<false>, grid, dim3(256), 0, s, indptr, idx, val, G, m, rows, W, l2, dst, flags);
    }
    BMX_LAUNCH_CHECK();
}

// out [n][ns] = X [n][ld] restricted to the columns cols [ns] (0-based): the subset.row genes of the output matrix
// (R/mnnCorrect.R:466-471).  One thread per output element.
__global__ void gather_cols_kernel(const double* __restrict__ X, int64_t n, int ld, const int32_t* __restrict__ cols, int ns,
                                   double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * ns) return;
    const int64_t r = e / ns;
    out[e] = X[r * ld + cols[e % ns]];
}

// out [dst[r]] = X [r] for rows of d doubles: the pool's leaf order back to the caller's batch order
// (.restore_original_order, R/mnnCorrect.R:373-378).  One thread per element.
__global__ void permute_rows_kernel(const double* __restrict__ X, int64_t n, int d, const int32_t* __restrict__ dst,
                                    double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * d) return;
    const int64_t r = e / d;
    out[(int64_t)dst[r] * d + e % d] = X[e];
}

void gather_cols(hipStream_t s, const double* X, int64_t n, int ld, const int32_t* cols, int ns, double* out) {
    if (n * ns <= 0) return;
    hipLaunchKernelGGL(gather_cols_kernel, dim3((unsigned)((n * ns + 255) / 256)), dim3(256), 0, s, X, n, ld, cols, ns, out);
    BMX_LAUNCH_CHECK();
}

template <class T>
T* put(DevBuf<T>& b, const T* host, size_t n, hipStream_t s) {
    T* p = b.reserve(std::max<size_t>(n, 1));
    if (n) BMX_HIP(hipMemcpyAsync(p, host, n * sizeof(T), hipMemcpyHostToDevice, s));
    return p;
}

// what a leaf or a finished merge of the plan (merge_plan.hpp: its slice of the pool) carries on the host
struct TNode {
    std::vector<int> index;     // batch ids (1-based), in row order
    bool has_restrict = false;
    std::vector<int32_t> restrict_rows;  // 0-based rows of the node, in the caller's order
};

// a Node view of a slice, with the restrict list and its dup chains (as Engine::upload builds them)
void make_view(Node& v, double* base, const PlanNode& at, const TNode& t, int d, hipStream_t s) {
    v.n = (int)at.n;
    v.data.alias(base + at.row0 * d, (size_t)std::max(1, v.n) * d);
    v.has_restrict = t.has_restrict;
    v.restrict_dups = false;
    if (!t.has_restrict) return;
    const int m = (int)t.restrict_rows.size();
    v.n_restrict = m;
    const RestrictChains rc = restrict_chains(t.restrict_rows.data(), m, v.n, 0);
    v.restrict_dups = rc.dups;
    put(v.restrict_rows, rc.rows.data(), (size_t)m, s);
    if (rc.dups) {
        put(v.dup_next, rc.next(), (size_t)m, s);
        put(v.dup_head, rc.head(), (size_t)m, s);
    }
    BMX_HIP(hipStreamSynchronize(s));  // (the host vectors go out of scope)
}

// all n rows in order on the device: the restrict list adjust_shift_variance takes of a side without restriction
const int32_t* identity_rows(DevBuf<int32_t>& b, int n, hipStream_t s) {
    std::vector<int32_t> io((size_t)n);
    for (int i = 0; i < n; ++i) io[i] = i;
    const int32_t* p = put(b, io.data(), io.size(), s);
    BMX_HIP(hipStreamSynchronize(s));
    return p;
}

}  // namespace

void mnn_correct_check(const MnnCorrectArgs& a) {
    if (a.B < 2) throw Error(BMX_ERR_ARG, "at least two batches must be specified");  // R/mnnCorrect.R:187
    if (a.svd_dim > 0) throw Error(BMX_ERR_ARG, "svd.dim > 0 is not supported (the biological subspace, R/mnnCorrect.R:313-329)");
    if (a.auto_merge) throw Error(BMX_ERR_ARG, "auto.merge=TRUE is not supported by mnnCorrect on the device");
    if (a.G < 1) throw Error(BMX_ERR_ARG, "every batch needs at least one gene");
    for (int b = 0; b < a.B; ++b) {
        if (a.ncells[b] < 1) throw Error(BMX_ERR_ARG, "every batch needs at least one cell");
        if (a.sparse()) {
            // one block that is the whole batch; its number of stored entries is where indptr ends
            const int64_t n = a.ncells[b];
            if (!a.indptr[b]) throw Error(BMX_ERR_ARG, "the block's 'indptr' is missing");
            check_csc_block(n, 0, n, a.indptr[b], a.indices ? a.indices[b] : nullptr, a.data ? a.data[b] : nullptr,
                            a.indptr[b][n]);
        } else if (!a.data[b]) {
            throw Error(BMX_ERR_ARG, "null batch matrix");
        }
        const bool has = a.restrict_idx && a.restrict_idx[b] && a.n_restrict && a.n_restrict[b] >= 0;
        if (!has) continue;
        if (a.n_restrict[b] == 0) throw Error(BMX_ERR_ARG, "no cells remaining in a batch after restriction");
        (void)restrict_chains(a.restrict_idx[b], a.n_restrict[b], a.ncells[b], 1);  // (its range check)
    }
    if (a.subset)
        for (int i = 0; i < a.nsubset; ++i)
            if (a.subset[i] < 1 || a.subset[i] > a.G) throw Error(BMX_ERR_SUBSET, "subset indices out of range");
    if (a.subset && a.nsubset < 1) throw Error(BMX_ERR_ARG, "'subset.row' selects no genes");
    if (a.subset && !a.correct_all && (a.cos_in != 0) != (a.cos_out != 0) && a.var_adj)
        // R/mnnCorrect.R:466-471 indexes the already subset output genes with subset.row again
        for (int i = 0; i < a.nsubset; ++i)
            if (a.subset[i] > a.nsubset) throw Error(BMX_ERR_SUBSET, "subscript out of bounds");
    if (a.k < 1) throw Error(BMX_ERR_ARG, "'k' must be positive");
    if (!(a.sigma > 0.0)) throw Error(BMX_ERR_ARG, "'sigma' must be positive");
    (void)plan_merges(a.tree, a.tree_len, a.B, a.ncells);  // the tree: post-order code, leaf = batch id, 0 = merge
}

void mnn_correct_run(const MnnCorrectArgs& a, MnnCorrectResult& res) {
    mnn_correct_check(a);
    const int B = a.B, G = a.G;
    int dev = 0;
    BMX_HIP(hipGetDevice(&dev));
    Engine e(dev);
    CacheScope cache_scope(e.cache());
    hipStream_t s = e.stream();

    // ---- the tree and the pool's row order (leaves left to right) ----
    const MergePlan plan = plan_merges(a.tree, a.tree_len, B, a.ncells);
    std::vector<TNode> t(plan.nodes.size());
    std::vector<int64_t> in_off((size_t)B + 1, 0), pool_off((size_t)B, 0);
    for (int b = 0; b < B; ++b) in_off[b + 1] = in_off[b] + a.ncells[b];
    const int64_t N = in_off[B];
    if (N > (int64_t)1 << 30) throw Error(BMX_ERR_ARG, "too many cells for int32 indices");
    for (size_t i = 0; i < t.size(); ++i) {
        const int b = plan.nodes[i].batch;
        if (b < 0) continue;
        pool_off[b] = plan.nodes[i].row0;
        t[i].index = {b + 1};
        t[i].has_restrict = a.restrict_idx && a.restrict_idx[b] && a.n_restrict && a.n_restrict[b] >= 0;
        if (t[i].has_restrict) t[i].restrict_rows = restrict_chains(a.restrict_idx[b], a.n_restrict[b], a.ncells[b], 1).rows;
    }

    // ---- .prepare_input_data (R/mnnCorrect.R:398-445) ----
    DevBuf<double> raw, subb, inb, outb, l2b;
    // subset.row equal to every gene in order is no subset (:404)
    bool subset = a.subset != nullptr && a.nsubset > 0;
    if (subset && a.nsubset == G) {
        bool ident = true;
        for (int i = 0; i < G && ident; ++i) ident = a.subset[i] == i + 1;
        if (ident) subset = false;
    }
    std::vector<int32_t> sub0;
    DevBuf<int32_t> subd;
    const int32_t* cols = nullptr;
    if (subset) {
        for (int i = 0; i < a.nsubset; ++i) sub0.push_back(a.subset[i] - 1);
        cols = put(subd, sub0.data(), sub0.size(), s);
    }
    const int Gs = subset ? a.nsubset : G;
    // S: the subset genes; In = S cosine-normalised with cos.norm.in; Out = all genes (correct.all) or S, cosine-normalised with
    // cos.norm.out by the l2 norms of S (:419-431).  same.set: one matrix serves both.
    const bool out_all = subset && a.correct_all;
    const bool same = !out_all && (a.cos_in != 0) == (a.cos_out != 0);
    const bool norms = a.cos_in || a.cos_out;
    double* l2 = l2b.reserve((size_t)N);
    double* S = nullptr;
    double* X = nullptr;  // all genes: the dense call's upload; of CSC batches only the output genes of correct.all
    if (!a.sparse()) {
        X = raw.reserve((size_t)N * G);  // the caller's genes, pool order: a cell's G genes are contiguous in R's layout
        for (int b = 0; b < B; ++b)
            upload_pageable(X + pool_off[b] * G, a.data[b], (size_t)a.ncells[b] * G * sizeof(double), s);
        S = X;
        if (subset) {
            S = subb.reserve((size_t)N * Gs);
            gather_cols(s, X, N, G, cols, Gs, S);
        }
        if (norms) cosine_l2_device(s, S, Gs, (int)N, l2);
    } else {
        // One batch's CSC at a time, in buffers sized for the largest batch: its rows of S (the subset's, or all) come
        // straight from the stored entries, then their norms, then -- correct.all with a subset -- its rows of the output
        // genes, already divided by those norms with cos.norm.out.  Without correct.all nothing here is [N][G] under a
        // subset; with it, X is the one such buffer.
        int64_t max_n = 0, max_nnz = 0;
        for (int b = 0; b < B; ++b) {
            max_n = std::max<int64_t>(max_n, a.ncells[b]);
            max_nnz = std::max(max_nnz, a.indptr[b][a.ncells[b]]);
        }
        DevBuf<int64_t> ipb;
        DevBuf<int32_t> ixb, flagb;
        DevBuf<double> valb;
        int64_t* ip = ipb.reserve((size_t)max_n + 1);
        int32_t* ix = ixb.reserve((size_t)std::max<int64_t>(max_nnz, 1));
        double* val = valb.reserve((size_t)std::max<int64_t>(max_nnz, 1));
        int32_t* flags = flagb.reserve(CSC_F_WORDS);
        BMX_HIP(hipMemsetAsync(flags, 0, CSC_F_WORDS * sizeof(int32_t), s));
        S = subb.reserve((size_t)N * Gs);
        if (out_all) X = raw.reserve((size_t)N * G);
        for (int b = 0; b < B; ++b) {
            const int64_t n = a.ncells[b], nnz = a.indptr[b][n], off = pool_off[b];
            upload_pageable(ip, a.indptr[b], (size_t)(n + 1) * sizeof(int64_t), s);
            upload_pageable(ix, a.indices[b], (size_t)nnz * sizeof(int32_t), s);
            upload_pageable(val, a.data[b], (size_t)nnz * sizeof(double), s);
            expand_csc(s, ip, ix, val, G, n, cols, Gs, nullptr, S + off * Gs, flags);
            if (norms) cosine_l2_device(s, S + off * Gs, Gs, (int)n, l2 + off);
            if (out_all) expand_csc(s, ip, ix, val, G, n, nullptr, G, a.cos_out ? l2 + off : nullptr, X + off * G, flags);
        }
        int32_t hflags[CSC_F_WORDS] = {0, 0};
        BMX_HIP(hipMemcpyAsync(hflags, flags, sizeof(hflags), hipMemcpyDeviceToHost, s));
        BMX_HIP(hipStreamSynchronize(s));
        throw_if_bad_pattern(hflags);
    }
    double* In = S;
    if (a.cos_in) {
        In = inb.reserve((size_t)N * Gs);
        apply_cosine_norm_device(s, S, Gs, (int)N, l2, In);
    }
    double* Out = In;
    int Go = Gs;
    if (!same) {
        Out = out_all ? X : S;
        Go = out_all ? G : Gs;
        if (a.cos_out && !(a.sparse() && out_all)) {  // (the CSC batches' output genes came out normalised)
            double* o = outb.reserve((size_t)N * Go);
            apply_cosine_norm_device(s, Out, Go, (int)N, l2, o);
            Out = o;
        }
    }

    // ---- the merges ----
    const int nm = B - 1;
    res.left.assign(nm, {});
    res.right.assign(nm, {});
    res.pairs_left.assign(nm, {});
    res.pairs_right.assign(nm, {});
    res.strict_cells.assign((size_t)nm * 2, -1);
    std::vector<int> pl0(nm), pr0(nm);
    DevBuf<double> avg, avg_out, corr_in, corr_out, dens, dens_out, scal, scal2, asv_ws, subL, subR, subC;
    DevBuf<int32_t> first, second, idx, iota1, iota2;
    std::vector<double> ones;
    // per-stage HIP events of a merge (search + pairs, averaging, smoothing, var.adj, apply), read after its final wait
    hipEvent_t ev[6];
    for (hipEvent_t& x : ev) BMX_HIP(hipEventCreate(&x));
    struct EvGuard {
        hipEvent_t* e;
        ~EvGuard() {
            for (int i = 0; i < 6; ++i) (void)hipEventDestroy(e[i]);
        }
    } ev_guard{ev};
    for (int mdx = 0; mdx < nm; ++mdx) {
        const int at = plan.merges[mdx];
        const PlanNode& Lp = plan.nodes[plan.nodes[at].left];
        const PlanNode& Rp = plan.nodes[plan.nodes[at].right];
        const TNode& L = t[plan.nodes[at].left];
        const TNode& R = t[plan.nodes[at].right];
        res.left[mdx] = L.index;
        res.right[mdx] = R.index;
        pl0[mdx] = (int)Lp.row0;
        pr0[mdx] = (int)Rp.row0;
        const int nl = (int)Lp.n, nr = (int)Rp.n;
        Node Lv, Rv;
        make_view(Lv, In, Lp, L, Gs, s);
        make_view(Rv, In, Rp, R, Gs, s);
        e.d_ = Gs;
        // 1. .restricted_mnn
        BMX_HIP(hipEventRecord(ev[0], s));
        const Engine::MnnOut mo = e.find_mnn(Lv, Rv, a.k, a.prop_k);
        const int nLs = L.has_restrict ? (int)L.restrict_rows.size() : nl;
        const int nRs = R.has_restrict ? (int)R.restrict_rows.size() : nr;
        const int32_t* lrows = L.has_restrict ? Lv.restrict_rows.p : nullptr;
        const int32_t* rrows = R.has_restrict ? Rv.restrict_rows.p : nullptr;
        const int32_t* rnext = Rv.restrict_dups ? Rv.dup_next.p : nullptr;
        // 2. the pairs: 1-based rows of the nodes
        int32_t* f = first.reserve((size_t)std::max<int64_t>(1, mo.P));
        int32_t* sc = second.reserve((size_t)std::max<int64_t>(1, mo.P));
        if (mo.P > 0)
            emit_pairs(s, e.idxLR_.p, mo.nsel, mo.k2, e.idxRL_.p, mo.k1, e.offL_.p, lrows, rrows, f, sc, e.lsel_.p, e.maskL_.p,
                       &e.sorted_);
        res.pairs_left[mdx].resize((size_t)mo.P);
        res.pairs_right[mdx].resize((size_t)mo.P);
        if (mo.P > 0) {
            BMX_HIP(hipMemcpyAsync(res.pairs_left[mdx].data(), f, (size_t)mo.P * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            BMX_HIP(hipMemcpyAsync(res.pairs_right[mdx].data(), sc, (size_t)mo.P * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        }
        // 3. averaging + smoothing (the kernel weights from the right node's input-gene rows)
        BMX_HIP(hipEventRecord(ev[1], s));
        const int U = mo.U;
        int32_t* ix = idx.reserve((size_t)std::max(1, U));
        if (U > 0) {
            if (rrows)
                compose_row_list(s, e.second_u_.p, U, rrows, ix);
            else
                BMX_HIP(hipMemcpyAsync(ix, e.second_u_.p, (size_t)U * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        }
        double* dw = dens.reserve((size_t)nr + std::max(1, U));
        double* av = avg.reserve((size_t)std::max(1, U) * Gs);
        double* ci = corr_in.reserve((size_t)nr * Gs);
        double* Lin = In + Lp.row0 * Gs;
        double* Rin = In + Rp.row0 * Gs;
        average_correction(s, e.red_ws_, Lin, lrows, Rin, rrows, Gs, e.second_u_.p, U, e.partR_.p, e.cntR_.p, mo.k1, av, false,
                           nullptr, nullptr, nullptr, nullptr, rnext);
        double* co = nullptr;
        double* avo = nullptr;
        double* Lout = Out + Lp.row0 * Go;
        double* Rout = Out + Rp.row0 * Go;
        if (!same) {
            avo = avg_out.reserve((size_t)std::max(1, U) * Go);
            average_correction(s, e.red_ws_, Lout, lrows, Rout, rrows, Go, e.second_u_.p, U, e.partR_.p, e.cntR_.p, mo.k1, avo,
                               false, nullptr, nullptr, nullptr, nullptr, rnext);
        }
        BMX_HIP(hipEventRecord(ev[2], s));
        smooth_gaussian_kernel_device(s, av, Gs, U, ix, Rin, Gs, nr, a.sigma, ci, dw);
        if (!same) {
            co = corr_out.reserve((size_t)nr * Go);
            double* dwo = dens_out.reserve((size_t)nr + std::max(1, U));
            smooth_gaussian_kernel_device(s, avo, Go, U, ix, Rin, Gs, nr, a.sigma, co, dwo);
        }
        // 4. var.adj
        BMX_HIP(hipEventRecord(ev[3], s));
        double* sv = scal.reserve((size_t)nr);
        if (a.var_adj) {
            const int32_t* r1 = lrows ? lrows : identity_rows(iota1, nl, s);
            const int32_t* r2 = rrows ? rrows : identity_rows(iota2, nr, s);
            const AsvPlan plan = adjust_shift_variance_plan(Gs, nr, nLs, nRs, 1);
            double* ws = asv_ws.reserve(adjust_shift_variance_scratch(plan, Gs, nr, nLs, nRs, a.var_adj_strict));
            int64_t counts[4];
            adjust_shift_variance_device(s, Lin, Gs, nl, Rin, nr, ci, a.sigma, r1, nLs, r2, nRs, sv, ws, plan, 1, 0, -1,
                                         a.var_adj_strict, counts);
            res.strict_cells[(size_t)mdx * 2] = counts[3];
            double* sv2 = nullptr;
            if (!same) {
                // locations from the subset.row genes of the output matrix (R/mnnCorrect.R:466-471).  R keeps subset.row
                // whenever it is not all genes, also when the output matrix is already the subset (correct.all = FALSE with
                // cos.norm.in != cos.norm.out): its indices then pick columns of that matrix, as R's cell.vect[, subset.row]
                // does (mnn_correct_check refuses indices beyond its width, where R fails with "subscript out of bounds").
                const double* l1 = Lout;
                const double* l2p = Rout;
                const double* cv = co;
                if (subset) {
                    double* a1 = subL.reserve((size_t)nl * Gs);
                    double* a2 = subR.reserve((size_t)nr * Gs);
                    double* a3 = subC.reserve((size_t)nr * Gs);
                    gather_cols(s, Lout, nl, Go, cols, Gs, a1);
                    gather_cols(s, Rout, nr, Go, cols, Gs, a2);
                    gather_cols(s, co, nr, Go, cols, Gs, a3);
                    l1 = a1;
                    l2p = a2;
                    cv = a3;
                }
                sv2 = scal2.reserve((size_t)nr);
                adjust_shift_variance_device(s, l1, Gs, nl, l2p, nr, cv, a.sigma, r1, nLs, r2, nRs, sv2, ws, plan, 1, 0, -1,
                                             a.var_adj_strict, counts);
                res.strict_cells[(size_t)mdx * 2 + 1] = counts[3];
            }
            BMX_HIP(hipEventRecord(ev[4], s));
            add_scaled_rows(s, Rin, nr, Gs, ci, sv);
            if (!same) add_scaled_rows(s, Rout, nr, Go, co, sv2);
        } else {
            BMX_HIP(hipEventRecord(ev[4], s));
            // right + correction: pmax(1, 1) * c = c exactly
            if ((int)ones.size() < nr) ones.assign((size_t)nr, 1.0);
            put(scal, ones.data(), (size_t)nr, s);
            add_scaled_rows(s, Rin, nr, Gs, ci, sv);
            if (!same) add_scaled_rows(s, Rout, nr, Go, co, sv);
        }
        BMX_HIP(hipEventRecord(ev[5], s));
        BMX_HIP(hipStreamSynchronize(s));
        for (int i = 0; i < 5; ++i) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) res.stage_ms[i] += ms;
        }
        // 5. UPDATE: rbind (the slices are adjacent), .combine_restrict (R/fastMNN.R:610-622)
        TNode m;
        m.index = L.index;
        m.index.insert(m.index.end(), R.index.begin(), R.index.end());
        m.has_restrict = L.has_restrict || R.has_restrict;
        if (m.has_restrict) {
            if (L.has_restrict)
                m.restrict_rows = L.restrict_rows;
            else
                for (int i = 0; i < nl; ++i) m.restrict_rows.push_back(i);
            if (R.has_restrict)
                for (int32_t v : R.restrict_rows) m.restrict_rows.push_back(v + nl);
            else
                for (int i = 0; i < nr; ++i) m.restrict_rows.push_back(nl + i);
        }
        t[at] = std::move(m);
    }

    // ---- outputs: input order (R/mnnCorrect.R:364-381) ----
    std::vector<int32_t> dst((size_t)N);
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < a.ncells[b]; ++i) dst[(size_t)(pool_off[b] + i)] = (int32_t)(in_off[b] + i);
    DevBuf<int32_t> dstd;
    DevBuf<double> fin;
    const int32_t* dd = put(dstd, dst.data(), dst.size(), s);
    double* fo = fin.reserve((size_t)N * Go);
    hipLaunchKernelGGL(permute_rows_kernel, dim3((unsigned)((N * Go + 255) / 256)), dim3(256), 0, s, (const double*)Out, N, Go,
                       dd, fo);
    BMX_LAUNCH_CHECK();
    res.Gout = Go;
    res.corrected.resize((size_t)N * Go);
    download_pageable(res.corrected.data(), fo, (size_t)N * Go * sizeof(double), s);
    BMX_HIP(hipStreamSynchronize(s));
    res.batch.resize((size_t)N);
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < a.ncells[b]; ++i) res.batch[(size_t)(in_off[b] + i)] = b + 1;
    for (int mdx = 0; mdx < nm; ++mdx) {
        for (int32_t& v : res.pairs_left[mdx]) v = dst[(size_t)(v - 1 + pl0[mdx])] + 1;
        for (int32_t& v : res.pairs_right[mdx]) v = dst[(size_t)(v - 1 + pr0[mdx])] + 1;
    }
}

}  // namespace bmx
