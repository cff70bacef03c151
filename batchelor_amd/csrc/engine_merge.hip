// Merge engine, one merge: node statistics and row passes, and Engine::merge_step with its phases (R/fastMNN.R:436-562).
#include "engine_internal.hpp"

namespace bmx {
namespace {

__global__ void gather_rows_i32(const int32_t* __restrict__ pos, int n, const int32_t* __restrict__ rows,
                                int32_t* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = rows ? rows[pos[i]] : pos[i];
}

__global__ void iota_offset(int32_t* __restrict__ out, int n, int off) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = off + i;
}

// the identity row list of a side without a restriction: out[i] = off + i (the caller checks the launch)
const int32_t* identity_rows(hipStream_t stream, int32_t* out, int n, int off) {
    hipLaunchKernelGGL(iota_offset, dim3(cdiv(n, 256)), dim3(256), 0, stream, out, n, off);
    return out;
}

// dup_next / dup_head of a merged node's restrict list = those of its children, the right child's positions shifted
__global__ void combine_dup_chains(const int32_t* __restrict__ lnext, const int32_t* __restrict__ lhead, int nl,
                                   const int32_t* __restrict__ rnext, const int32_t* __restrict__ rhead, int nr,
                                   int32_t* __restrict__ next, int32_t* __restrict__ head) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nl + nr) return;
    if (i < nl) {
        next[i] = lnext ? lnext[i] : -1;
        head[i] = lhead ? lhead[i] : 1;
    } else {
        const int32_t t = rnext ? rnext[i - nl] : -1;
        next[i] = t >= 0 ? t + nl : -1;
        head[i] = rhead ? rhead[i - nl] : 1;
    }
}

__global__ void add_offset_copy(const int32_t* __restrict__ in, int n, int off, int32_t* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i] + off;
}

// n doubles from src to dst (a device copy as a kernel: a hipMemcpyAsync between device buffers costs ~200 us of idle stream
// in front of it on this runtime, a launch ~5)
__global__ void copy_doubles_kernel(double* __restrict__ dst, const double* __restrict__ src, int64_t n) {
    const int64_t n2 = n >> 1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (int64_t)gridDim.x * blockDim.x)
        reinterpret_cast<double2*>(dst)[i] = reinterpret_cast<const double2*>(src)[i];
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) dst[n - 1] = src[n - 1];
}
void copy_doubles(hipStream_t stream, double* dst, const double* src, int64_t n) {
    if (n <= 0) return;
    if ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15) {  // (never for rows of an even d)
        BMX_HIP(hipMemcpyAsync(dst, src, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, stream));
        return;
    }
    hipLaunchKernelGGL(copy_doubles_kernel, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, (n / 2 + 255) / 256))),
                       dim3(256), 0, stream, dst, src, n);
    BMX_LAUNCH_CHECK();
}

void segment_layout(const Node& node, std::vector<int>& starts, std::vector<int>& ns) {
    int r0 = 0;
    for (const Segment& s : node.origin) {
        starts.push_back(r0);
        ns.push_back(s.n);
        r0 += s.n;
    }
}
}  // namespace

int Engine::take_slot() {
    if (n_slots_ + 1 > slot_cap_) throw Error(BMX_ERR_ARG, "internal: statistics slots exhausted");
    return n_slots_++;
}

void Engine::node_mean(const Node& node, double* mu) {
    bool fresh = !node.has_restrict && node.origin.size() <= 16 && node.stat_slot.size() == node.origin.size();
    for (int sl : node.stat_slot) fresh = fresh && sl >= 0;
    if (fresh) {
        std::vector<int> starts, ns;
        segment_layout(node, starts, ns);
        node_mean_from_segments(stream_, means_pool_.p, ns.data(), node.stat_slot.data(), (int)ns.size(), d_, mu);
    } else if (node.has_restrict) {
        col_reduce(stream_, red_ws_, node.data.p, node.restrict_rows.p, 0, node.n_restrict, d_, 0, nullptr,
                   1.0 / (double)node.n_restrict, mu);
    } else {
        col_reduce(stream_, red_ws_, node.data.p, nullptr, 0, node.n, d_, 0, nullptr, 1.0 / (double)node.n, mu);
    }
}

void Engine::row_pass(Node& node, const std::vector<int>& vec_ids, bool with_stats, const double* mu_known) {
    if (vec_ids.empty() && !with_stats) return;
    double* mu_own = vecs_.p + (size_t)(2 * B_ + 5) * d_;
    if (!vec_ids.empty() && !mu_known) node_mean(node, mu_own);
    const double* mu = mu_known ? mu_known : mu_own;
    std::vector<int> starts, ns, slots;
    segment_layout(node, starts, ns);
    if (with_stats)
        for (size_t i = 0; i < ns.size(); ++i) slots.push_back(take_slot());
    rows_apply_stats(stream_, red_ws_, node.data.p, d_, starts.data(), ns.data(), (int)ns.size(), mu, vecs_.p,
                     vec_ids.data(), (int)vec_ids.size(), with_stats ? slots.data() : nullptr, means_pool_.p, scal_.p);
    if (with_stats)
        node.stat_slot = slots;
    else
        node.stat_slot.assign(node.origin.size(), -1);  // the rows moved: their statistics are stale
}

void Engine::ensure_stats(Node& node) { ensure_stats2(node, nullptr); }

void Engine::ensure_stats2(Node& a, Node* b) {
    // .compute_perbatch_var (R/fastMNN.R:651-658) only for the segments whose rows changed since their last statistics; the
    // stale segments of both nodes of a merge go through ONE pass (+ one small launch that finishes the sums)
    std::vector<RowSeg> segs;
    std::vector<std::pair<Node*, int>> which;
    for (Node* node : {&a, b}) {
        if (!node) continue;
        if (node->stat_slot.size() != node->origin.size()) node->stat_slot.assign(node->origin.size(), -1);
        int r0 = 0;
        for (size_t i = 0; i < node->origin.size(); ++i) {
            if (node->stat_slot[i] < 0) {
                segs.push_back(RowSeg{node->data.p, r0, node->origin[i].n, nullptr, nullptr, take_slot()});
                which.emplace_back(node, (int)i);
            }
            r0 += node->origin[i].n;
        }
    }
    if (segs.empty()) return;
    rows_multi(stream_, red_ws_, d_, segs.data(), (int)segs.size(), vecs_.p, nullptr, 0, true, means_pool_.p, scal_.p);
    for (size_t i = 0; i < which.size(); ++i) which[i].first->stat_slot[which[i].second] = segs[i].slot;
}

void Engine::node_means(const Node& left, const Node& right, double* mu_l, double* mu_r) {
    auto fresh = [](const Node& n) {
        bool f = !n.has_restrict && n.stat_slot.size() == n.origin.size();
        for (int sl : n.stat_slot) f = f && sl >= 0;
        return f;
    };
    if (fresh(left) && fresh(right) && left.origin.size() + right.origin.size() <= 16) {
        std::vector<int> ns, slots;
        for (const Node* n : {&left, &right})
            for (size_t i = 0; i < n->origin.size(); ++i) {
                ns.push_back(n->origin[i].n);
                slots.push_back(n->stat_slot[i]);
            }
        node_means_from_segments(stream_, means_pool_.p, ns.data(), slots.data(), (int)left.origin.size(),
                                 (int)right.origin.size(), d_, mu_l, mu_r);
    } else {
        node_mean(left, mu_l);
        node_mean(right, mu_r);
    }
}

void Engine::centre_both(Node& left, Node& right, int vid, const double* mu_l, const double* mu_r) {
    // .center_along_batch_vector on both sides (R/fastMNN.R:496-497) with the "new" variances (:498-499) out of the same
    // pass.  The shift of a segment's one-pass variance: its old mean where its statistics are current, else (the side that
    // has just been orthogonalised) its node's mean -- any fixed vector inside the cloud serves
    std::vector<RowSeg> segs;
    for (Node* node : {&left, &right}) {
        int r0 = 0;
        for (size_t i = 0; i < node->origin.size(); ++i) {
            const double* mu = node == &left ? mu_l : mu_r;
            const bool cur = node->stat_slot.size() == node->origin.size() && node->stat_slot[i] >= 0;
            segs.push_back(RowSeg{node->data.p, r0, node->origin[i].n, mu,
                                  cur ? means_pool_.p + (size_t)node->stat_slot[i] * d_ : mu, take_slot()});
            r0 += node->origin[i].n;
        }
    }
    rows_multi(stream_, red_ws_, d_, segs.data(), (int)segs.size(), vecs_.p, &vid, 1, true, means_pool_.p, scal_.p);
    size_t j = 0;
    for (Node* node : {&left, &right}) {
        node->stat_slot.assign(node->origin.size(), -1);
        for (size_t i = 0; i < node->origin.size(); ++i) node->stat_slot[i] = segs[j++].slot;
    }
}

void Engine::orthogonalize(Node& node, const std::vector<int>& extras) {
    // .orthogonalize_other (R/fastMNN.R:642-647): sequentially, each on the result of the previous -- one pass
    row_pass(node, extras, false);
}

void Engine::copy_restrict(Node& node, int m, const int32_t* rows, const int32_t* next, const int32_t* head) {
    node.has_restrict = true;
    node.n_restrict = m;
    BMX_HIP(hipMemcpyAsync(node.restrict_rows.reserve(m), rows, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToDevice, stream_));
    if (next) {
        node.restrict_dups = true;
        BMX_HIP(hipMemcpyAsync(node.dup_next.reserve(m), next, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToDevice, stream_));
        BMX_HIP(hipMemcpyAsync(node.dup_head.reserve(m), head, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToDevice, stream_));
    }
}

std::unique_ptr<Node> Engine::clone_node(const Node& src) {
    auto n = std::make_unique<Node>();
    n->index = src.index;
    n->n = src.n;
    n->origin = src.origin;
    n->stat_slot = src.stat_slot;
    n->extras = src.extras;
    double* p = n->data.reserve((size_t)src.n * d_);
    BMX_HIP(hipMemcpyAsync(p, src.data.p, (size_t)src.n * d_ * sizeof(double), hipMemcpyDeviceToDevice, stream_));
    if (src.has_restrict)
        copy_restrict(*n, src.n_restrict, src.restrict_rows.p, src.restrict_dups ? src.dup_next.p : nullptr, src.dup_head.p);
    return n;
}

int Engine::count_mnn_pairs(const Node& left, const Node& right, const bmx_params_t& p) {
    // one (left, right) evaluation of .count_mnn_pairs (R/MNN_tree.R:171-193) on orthogonalised COPIES
    const Node* l = &left;
    const Node* r = &right;
    std::unique_ptr<Node> lc, rc;
    if (!left.extras.empty()) {
        rc = clone_node(right);
        orthogonalize(*rc, left.extras);
        r = rc.get();
    }
    if (!right.extras.empty()) {
        lc = clone_node(left);
        orthogonalize(*lc, right.extras);
        l = lc.get();
    }
    const MnnOut o = find_mnn(*l, *r, p.k, p.prop_k);
    return (int)o.P;
}

void Engine::merge_step(int mdx, Node& left, Node& right, const bmx_params_t& p, std::unique_ptr<Node>& merged) {
    MergeCtx c(mdx, left, right, p, merges_[mdx]);
    merge_prepare(c);
    c.mo = find_mnn(left, right, p.k, p.prop_k, c.mu_l, c.mu_r);  // R/fastMNN.R:476-477
    if (c.mo.P == 0) throw Error(BMX_ERR_NO_PAIRS, "no mutual nearest neighbours found between batches");
    merge_batch_vector(c);
    const bool corrected = !merge_is_skipped(c);
    if (corrected)
        merge_correct(c);
    else
        merge_skipped_stats(c);
    merged = merge_update(c, corrected);
    // the copies of the update read left / right data: the caller releases those nodes into this engine's block cache,
    // whose next user is ordered behind the copies by the stream
}

// streaming section 1: statistics, orthogonalisation
void Engine::merge_prepare(MergeCtx& c) {
    Node &left = c.left, &right = c.right;
    MergeRecord& rec = c.rec;
    rec.left_set = left.index;
    rec.right_set = right.index;
    rec.var_batches.clear();
    for (const Segment& s : left.origin) rec.var_batches.push_back(s.batch);
    for (const Segment& s : right.origin) rec.var_batches.push_back(s.batch);

    c.sec = std::make_unique<Section>(this);
    // "old" variances (R/fastMNN.R:467-468): a segment untouched since its last statistics keeps them (the left
    // node's segments carry the "new" variances of the merge that made it); the stale ones of both nodes in one pass
    ensure_stats2(left, &right);
    rec.old_slot = concat(left.stat_slot, right.stat_slot);

    // the restrict-row column means of both sides: centring along a vector never moves them, so the ones taken here
    // (from the fresh segment statistics where there is no restriction) serve every pass of this merge
    c.mu_l = vecs_.p + (size_t)(2 * B_ + 6) * d_;
    c.mu_r = vecs_.p + (size_t)(2 * B_ + 7) * d_;
    node_means(left, right, c.mu_l, c.mu_r);
    row_pass(right, left.extras, false, c.mu_r);  // .orthogonalize_other, R/fastMNN.R:473-474
    row_pass(left, right.extras, false, c.mu_l);

    if (c.mdx == snap_merge_) {
        snap_nl_ = left.n;
        snap_nr_ = right.n;
        BMX_HIP(hipMemcpyAsync(snap_l_.reserve((size_t)left.n * d_), left.data.p, (size_t)left.n * d_ * sizeof(double),
                               hipMemcpyDeviceToDevice, stream_));
        BMX_HIP(hipMemcpyAsync(snap_r_.reserve((size_t)right.n * d_), right.data.p,
                               (size_t)right.n * d_ * sizeof(double), hipMemcpyDeviceToDevice, stream_));
    }
    c.sec.reset();
}

// streaming section 2 (open until the tricube search): pairs, averaging, centring + statistics
void Engine::merge_batch_vector(MergeCtx& c) {
    const Node &left = c.left, &right = c.right;
    MergeRecord& rec = c.rec;
    const MnnOut& mo = c.mo;
    const bmx_params_t& p = c.p;
    c.sec = std::make_unique<Section>(this);
    rec.npairs = mo.P;
    rec.stats[0] = c.nLs;
    rec.stats[1] = c.nRs;
    rec.stats[2] = mo.U;
    rec.stats[3] = mo.P;
    rec.stats[4] = left.n;
    rec.stats[5] = right.n;
    int32_t* first = rec.first.reserve((size_t)mo.P);
    int32_t* second = rec.second.reserve((size_t)mo.P);
    emit_pairs(stream_, idxLR_.p, mo.nsel, mo.k2, idxRL_.p, mo.k1, offL_.p, c.lrows, c.rrows, first, second, lsel_.p,
               maskL_.p, &sorted_);

    // .average_correction + overall.batch (R/fastMNN.R:480-481); the column means of the averaged vectors, the mean squares
    // .get_batch_magnitude wants (R/fastMNN.R:582-595) and the magnitude itself come out of the same pass where its fused
    // form applies
    c.averaged = averaged_.reserve((size_t)mo.U * d_);
    c.vid = n_extras_;
    double* overall = vecs_.p + (size_t)c.vid * d_;
    double* msq = vecs_.p + (size_t)(2 * B_ + 4) * d_;
    rec.batch_size_na = std::isnan(p.min_batch_skip);
    rec.skipped = false;
    rec.bs_slot = rec.batch_size_na ? -1 : take_slot();
    double* mag = rec.bs_slot >= 0 ? scal_.p + rec.bs_slot : nullptr;
    // (several ranks: this averaging's workgroups are dealt over them, the column sums all-gathered -- see AvgShard)
    const bool avg_sharded = transport_in_play();
    AvgShard ash{rank_, world_, [this](void* buf, int64_t bytes) { exchange(buf, bytes); }};
    if (!average_correction(stream_, red_ws_, left.data.p, c.lrows, right.data.p, c.rrows, d_, second_u_.p, mo.U, partR_.p,
                            cntR_.p, mo.k1, c.averaged, true, overall, msq, mag, nullptr, c.rnext, avg_sharded ? &ash : nullptr)) {
        if (rec.batch_size_na) {
            col_reduce(stream_, red_ws_, c.averaged, nullptr, 0, mo.U, d_, 0, nullptr, 1.0 / (double)mo.U, overall);
        } else {
            col_reduce2(stream_, red_ws_, c.averaged, mo.U, d_, 1.0 / (double)mo.U, overall, msq);
            batch_magnitude(stream_, overall, msq, d_, mag);
        }
    }
}

bool Engine::merge_is_skipped(MergeCtx& c) {
    MergeRecord& rec = c.rec;
    if (rec.batch_size_na || !(c.p.min_batch_skip > 0.0)) return false;
    // the host only looks at the magnitude here when a merge can actually be skipped (min.batch.skip > 0), otherwise
    // with everything else at the end of the run
    double* hp = reinterpret_cast<double*>(knn_ws_.pinned_words() + 4);
    BMX_HIP(hipMemcpyAsync(hp, scal_.p + rec.bs_slot, sizeof(double), hipMemcpyDeviceToHost, stream_));
    wait();
    const double h = *hp;
    rec.skipped = h < c.p.min_batch_skip;
    return rec.skipped;
}

void Engine::merge_correct(MergeCtx& c) {
    Node &left = c.left, &right = c.right;
    const MnnOut& mo = c.mo;
    const bmx_params_t& p = c.p;
    // R/fastMNN.R:496-501: centre both sides along the batch vector; the "new" variances come out of the same pass
    centre_both(left, right, c.vid, c.mu_l, c.mu_r);
    c.rec.new_slot = concat(left.stat_slot, right.stat_slot);

    // R/fastMNN.R:505-507: re-average on the centred data, then the tricube-smoothed correction of the right batch;
    // the rows of the MNN-involved right cells (the reference list of the tricube search) are written on the way
    int32_t* srows = second_rows_.reserve(mo.U);
    if (!average_correction(stream_, red_ws_, left.data.p, c.lrows, right.data.p, c.rrows, d_, second_u_.p, mo.U, partR_.p,
                            cntR_.p, mo.k1, c.averaged, false, nullptr, nullptr, nullptr, srows, c.rnext)) {
        hipLaunchKernelGGL(gather_rows_i32, dim3(cdiv(mo.U, 256)), dim3(256), 0, stream_, second_u_.p, mo.U, c.rrows, srows);
        BMX_LAUNCH_CHECK();
    }
    const int k_tc = choose_k(p.k, p.prop_k, right.n);  // unrestricted size of the right batch
    const int safe_k = std::min(k_tc, mo.U);
    const int64_t per = bmx_shard_rows_per_rank(right.n, world_) * (int64_t)world_;
    int32_t* idxT = idxT_.reserve((size_t)per * safe_k);
    double* distT = distT_.reserve((size_t)per * safe_k);
    // Several ranks (without var_adj): every rank has the neighbour lists of ITS slice of the right cells from the search;
    // it corrects those rows and the CORRECTED ROWS are all-gathered (n x d x 8 bytes) instead of the lists (n x k x 12):
    // the same order of bytes, and the apply is sharded with the search instead of being repeated on every rank.
    // (testing hook "exchange_always": a single rank with a transport takes this way too, an all-gather of one)
    const bool rows_sharded = !p.var_adj && transport_in_play();
    c.sec.reset();
    knn(right.data.p, srows, mo.U, right.data.p, nullptr, right.n, safe_k, idxT, distT, nullptr, c.mu_r, nullptr, !rows_sharded,
        c.mu_r);
    c.sec = std::make_unique<Section>(this);  // streaming section 3: tricube apply, rbind
    if (rows_sharded)
        apply_rows_sharded(c, safe_k);
    else if (!p.var_adj)
        tricube_apply(stream_, right.data.p, right.n, d_, c.averaged, idxT, distT, safe_k, p.ndist);
    else
        apply_var_adj(c, safe_k);
    right.stat_slot.assign(right.origin.size(), -1);  // the corrected cells moved
    ++n_extras_;
}

// this rank's slice of the right rows corrected from its slice of the tricube search's lists, then the rows all-gathered
void Engine::apply_rows_sharded(MergeCtx& c, int safe_k) {
    Node& right = c.right;
    const int64_t per1 = bmx_shard_rows_per_rank(right.n, world_);
    const int64_t per = per1 * (int64_t)world_;
    int64_t b = 0, e = right.n;
    bmx_shard_range_impl(right.n, rank_, world_, &b, &e);
    if (e > b)
        tricube_apply(stream_, right.data.p + (size_t)b * d_, (int)(e - b), d_, c.averaged, idxT_.p + (size_t)b * safe_k,
                      distT_.p + (size_t)b * safe_k, safe_k, c.p.ndist);
    // (the node's rows sit in the run's arena, other leaves right behind them: the padded slices meet in a buffer)
    double* rows = corr_.reserve((size_t)per * d_);
    copy_doubles(stream_, rows + (size_t)b * d_, right.data.p + (size_t)b * d_, (e - b) * (int64_t)d_);
    exchange(rows, per1 * d_ * (int64_t)sizeof(double));
    copy_doubles(stream_, right.data.p, rows, b * (int64_t)d_);
    copy_doubles(stream_, right.data.p + (size_t)e * d_, rows + (size_t)e * d_, (right.n - e) * (int64_t)d_);
}

// mnnCorrect(var.adj=TRUE) on the fastMNN correction (R/mnnCorrect.R:331-342,462-481): every right cell's
// correction vector is stretched so that the cell lands on the matching quantile of the left batch
void Engine::apply_var_adj(MergeCtx& c, int safe_k) {
    Node &left = c.left, &right = c.right;
    const bmx_params_t& p = c.p;
    const int nLs = c.nLs, nRs = c.nRs;
    double* corr = corr_.reserve((size_t)right.n * d_);
    tricube_vectors(stream_, right.n, d_, c.averaged, idxT_.p, distT_.p, safe_k, p.ndist, corr);
    const int32_t* r1 = c.lrows;
    const int32_t* r2 = c.rrows;
    if (!r1) r1 = identity_rows(stream_, iota_l_.reserve(left.n), left.n, 0);
    if (!r2) r2 = identity_rows(stream_, iota_r_.reserve(right.n), right.n, 0);
    BMX_LAUNCH_CHECK();
    // The reference's loop is independent per right cell (src/adjust_shift_variance.cpp:51-161): each rank takes its
    // slice of them (the layout of the sharded searches, bmx_shard_range) and the scalings are all-gathered in place.
    // The form (exact / tiled) is decided from the WHOLE call's size, so every rank count gives the same numbers.
    AsvPlan plan = adjust_shift_variance_plan(d_, right.n, nLs, nRs, 1);
    int64_t cb = 0, ce = right.n;
    bmx_shard_range_impl(right.n, rank_, world_, &cb, &ce);
    const int64_t per_cells = bmx_shard_rows_per_rank(right.n, world_);
    // (params.var_adj_strict: the strict pass's scratch lies behind the plan's own)
    double* ws = asv_ws_.reserve(adjust_shift_variance_scratch(plan, d_, right.n, nLs, nRs, p.var_adj_strict));
    double* scaling = asv_scale_.reserve((size_t)per_cells * world_);
    c.sec.reset();  // (the variance adjustment is timed on its own: event tag 4, bmx_engine_profile_var_adj)
    std::pair<hipEvent_t, hipEvent_t> aev{nullptr, nullptr};
    if (knn_ws_.profile) {
        aev = knn_ws_.next_events(4);
        (void)hipEventRecord(aev.first, stream_);
    }
    // (testing hook "asv_modes": this merge's share of the tiled form's tallies, and the snapshot merge's per-cell ways --
    // both wait for the device, which a test may)
    const bool tallies = dev_knobs().asv_modes > 0 && !plan.exact;
    unsigned long long t0[3] = {0, 0, 0};
    if (tallies) asv_tally_read(t0, false);
    int64_t counts[4] = {-1, -1, -1, -1};  // (strict mode: the call waits once for the number of cells to recompute)
    adjust_shift_variance_device(stream_, left.data.p, d_, left.n, right.data.p, right.n, corr, p.sigma, r1, nLs, r2,
                                 nRs, scaling, ws, plan, /* vect_row_major */ 1, (int)cb, (int)ce, p.var_adj_strict, counts);
    c.rec.asv_strict = counts[3];
    if (aev.second) (void)hipEventRecord(aev.second, stream_);
    if (tallies) {
        unsigned long long t1[3] = {0, 0, 0};
        asv_tally_read(t1, false);
        for (int i = 0; i < 3; ++i) c.rec.asv_tally[i] = (int64_t)(t1[i] - t0[i]);
        if (c.mdx == snap_merge_) {
            snap_modes_.assign((size_t)right.n, 255);
            asv_modes_read(snap_modes_.data(), snap_modes_.size());
        }
    }
    asv_pairs_ += (double)(ce - cb) * ((double)nLs + (double)nRs);
    c.sec = std::make_unique<Section>(this);
    queued_work_s_ += 5e-8 * (double)(ce - cb) * ((double)nLs + (double)nRs);
    exchange(scaling, per_cells * (int64_t)sizeof(double));
    if (c.mdx == snap_merge_) {  // diagnostics: what adjust_shift_variance was handed at this merge, and what it returned
        snap_anl_ = left.n;
        snap_anr_ = right.n;
        snap_ar1_ = nLs;
        snap_ar2_ = nRs;
        auto keep = [&](DevBuf<double>& b, const double* src, size_t n) {
            BMX_HIP(hipMemcpyAsync(b.reserve(n), src, n * sizeof(double), hipMemcpyDeviceToDevice, stream_));
        };
        keep(snap_al_, left.data.p, (size_t)left.n * d_);
        keep(snap_ar_, right.data.p, (size_t)right.n * d_);
        keep(snap_ac_, corr, (size_t)right.n * d_);
        keep(snap_as_, scaling, (size_t)right.n);
        BMX_HIP(hipMemcpyAsync(snap_ai1_.reserve((size_t)std::max(nLs, 1)), r1, (size_t)nLs * sizeof(int32_t),
                               hipMemcpyDeviceToDevice, stream_));
        BMX_HIP(hipMemcpyAsync(snap_ai2_.reserve((size_t)std::max(nRs, 1)), r2, (size_t)nRs * sizeof(int32_t),
                               hipMemcpyDeviceToDevice, stream_));
    }
    add_scaled_rows(stream_, right.data.p, right.n, d_, corr, scaling);
}

void Engine::merge_skipped_stats(MergeCtx& c) {
    // skipped: the "new" variances are those of the (orthogonalised) data as it stands (R/fastMNN.R:500-501)
    ensure_stats(c.left);
    ensure_stats(c.right);
    c.rec.new_slot = concat(c.left.stat_slot, c.right.stat_slot);
}

// UPDATE (R/fastMNN.R:520-525): rbind, combine restrict, concatenate origin / extras
std::unique_ptr<Node> Engine::merge_update(MergeCtx& c, bool corrected) {
    const Node &left = c.left, &right = c.right;
    const int nLs = c.nLs, nRs = c.nRs;
    auto merged = std::make_unique<Node>();
    Node& m = *merged;
    m.index = concat(left.index, right.index);
    m.n = left.n + right.n;
    if (left.data.view && right.data.view && left.data.p + (size_t)left.n * d_ == right.data.p) {
        // both children sit next to each other in the run's arena (leaves laid out in tree order): the merged node IS
        // that stretch of rows, rbind copies nothing
        m.data.alias(left.data.p, (size_t)m.n * d_);
    } else {
        double* md = m.data.reserve((size_t)m.n * d_);
        BMX_HIP(hipMemcpyAsync(md, left.data.p, (size_t)left.n * d_ * sizeof(double), hipMemcpyDeviceToDevice, stream_));
        BMX_HIP(hipMemcpyAsync(md + (size_t)left.n * d_, right.data.p, (size_t)right.n * d_ * sizeof(double),
                               hipMemcpyDeviceToDevice, stream_));
    }
    m.origin = concat(left.origin, right.origin);
    m.stat_slot = concat(left.stat_slot, right.stat_slot);
    m.extras = concat(left.extras, right.extras);
    if (corrected) m.extras.push_back(c.vid);
    if (left.has_restrict || right.has_restrict) {  // .combine_restrict (R/fastMNN.R:610-622)
        m.has_restrict = true;
        m.n_restrict = nLs + nRs;
        int32_t* mr = m.restrict_rows.reserve(m.n_restrict);
        if (left.has_restrict)
            BMX_HIP(hipMemcpyAsync(mr, left.restrict_rows.p, (size_t)nLs * sizeof(int32_t), hipMemcpyDeviceToDevice,
                                   stream_));
        else
            identity_rows(stream_, mr, nLs, 0);
        if (right.has_restrict)
            hipLaunchKernelGGL(add_offset_copy, dim3(cdiv(nRs, 256)), dim3(256), 0, stream_, right.restrict_rows.p,
                               nRs, left.n, mr + nLs);
        else
            identity_rows(stream_, mr + nLs, nRs, left.n);
        BMX_LAUNCH_CHECK();
        if (left.restrict_dups || right.restrict_dups) {  // the chains of repeated cells: positions of the right part shift by nLs
            m.restrict_dups = true;
            int32_t* nx = m.dup_next.reserve(m.n_restrict);
            int32_t* hd = m.dup_head.reserve(m.n_restrict);
            hipLaunchKernelGGL(combine_dup_chains, dim3(cdiv(m.n_restrict, 256)), dim3(256), 0, stream_,
                               left.restrict_dups ? left.dup_next.p : nullptr, left.restrict_dups ? left.dup_head.p : nullptr, nLs,
                               right.restrict_dups ? right.dup_next.p : nullptr, right.restrict_dups ? right.dup_head.p : nullptr,
                               nRs, nx, hd);
            BMX_LAUNCH_CHECK();
        }
    }
    return merged;
}

}  // namespace bmx
