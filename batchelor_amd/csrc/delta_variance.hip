// mnnDeltaVariance() (R/mnnDeltaVariance.R:95-201) on the device: for every merge step the per-gene mean of the paired
// cells and the variance of their deltas, over genes x cells FP64 matrices in R's layout that are uploaded once and kept
// in HBM.  The hot path is a gather: every pair reads two whole gene vectors.
//   norms   cos.norm (:121-126): l2 of every cell over the norm genes, each batch's mean l2 by a fixed-order tree, ml2 the
//           mean of those; scale[c] = 1 / pmax(1e-8, l2[c] / ml2).
//   prep    one thread per pair: the two columns' addresses (a search of the batches' offset table) and scales.
//   pass 1  a workgroup owns DELTA_GENE_TILE genes (lanes along the genes, 16-byte loads where G is even) and one chunk
//           of DELTA_PAIR_CHUNK pairs of one step: the sums of s_l x_left and of s_r x_right in pair order.  Four pairs'
//           loads are in flight; a left cell that repeats stays in registers.  mean_reduce_kernel adds the chunk sums:
//           mean (:197) and the mean delta.
//   pass 2  the same walk: sum of (delta - mean delta)^2 (rowVars' two passes, :196); total_reduce_kernel adds the chunks
//           and divides by P - 1 (NaN below two pairs).
// The chunk edges are fixed positions of a step's pair list; the orders of the sums are those of ordered_sums.hpp.  All
// FP64 vector arithmetic, contraction off.
//
// DeltaSparse keeps the batches as CSC and runs the same stages over the stored entries:
//   check   every stored entry once, behind its upload: rows in [0, G) and strictly ascending, values finite.  A run
//           refuses a bad pattern before its pair passes start.
//   norms   one wave a cell over its stored entries (a G-long multiplicity mask stands for the norm genes), then
//           l2_mean_kernel and scale_kernel as above.
//   prep    one thread per pair: where the two columns' entries begin, how many there are, the two scales.
//   passes  a workgroup is ONE wave: it owns DELTA_SPARSE_GENE_TILE genes and a chunk (the dense chunks), keeps the
//           tile's sums in LDS and takes the pairs in order, lanes striding over a column's entries inside the tile.
//           Rows are unique within a column, so no two lanes meet; between two pairs stands a workgroup barrier, which
//           for a workgroup of one wave is a wait for the LDS queue and no s_barrier.  Pass 1 adds the dense pass's terms
//           with the +0 ones left out: the same bits.  Pass 2 combines the two entries of a gene through an LDS scratch
//           before it squares; the pairs where neither cell stores the gene enter once per chunk as
//           (pairs - touched) * mdelta * mdelta.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "bmx_ops.hpp"
#include "csc_device.hpp"
#include "host_xfer.hpp"
#include "ordered_sums.hpp"
#include "resident_batches.hpp"

namespace bmx {
namespace {

constexpr int GT = DELTA_GENE_TILE;
constexpr int PC = DELTA_PAIR_CHUNK;
constexpr int TPB = GT / 2;  // threads of a pair-pass workgroup: two genes each

struct PairRef {
    const double* l;  // the left cell's column
    const double* r;
    double sl, sr;    // their scales (1 without cos.norm)
};
struct ChunkRef {
    int64_t begin;  // first pair, counted over the steps' concatenated lists
    int32_t len, step;
};

// bmean[b] = mean of l2 over batch b's cells: 256 strided sums, then a tree in a fixed order
__global__ __launch_bounds__(256) void l2_mean_kernel(const double* __restrict__ l2, const int64_t* __restrict__ off,
                                                      double* __restrict__ bmean) {
    __shared__ double sh[256];
    const int b = blockIdx.x;
    const int64_t c0 = off[b], n = off[b + 1] - c0;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) s += l2[c0 + i];
    const double sum = block_tree_sum<256>(s, sh);
    if (threadIdx.x == 0) bmean[b] = sum / (double)n;
}

// scale[c] = 1 / pmax(1e-8, l2[c] / ml2), ml2 = mean over the batches of bmean (:123-125, R/cosineNorm.R:80)
__global__ __launch_bounds__(256) void scale_kernel(const double* __restrict__ l2, int64_t N,
                                                    const double* __restrict__ bmean, int B, double* __restrict__ scale) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= N) return;
    double m = 0.0;
    for (int b = 0; b < B; ++b) m += bmean[b];
    m /= (double)B;
    scale[c] = 1.0 / cos_clamp(l2[c] / m);
}

// left / right: 1-based columns of the batches side by side; off [B + 1] the batches' first columns, base [B] their
// matrices.  The batch of a column is looked up here, once per pair.
__global__ __launch_bounds__(256) void pair_prep_kernel(const int32_t* __restrict__ left, const int32_t* __restrict__ right,
                                                        int64_t P, const int64_t* __restrict__ off, int B,
                                                        const double* const* __restrict__ base, int G,
                                                        const double* __restrict__ scale, PairRef* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    auto column = [&](int64_t c) {
        int lo = 0, hi = B - 1;  // the last batch that starts at or before c
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (off[mid] <= c) lo = mid; else hi = mid - 1;
        }
        return base[lo] + (c - off[lo]) * G;
    };
    const int64_t cl = (int64_t)left[p] - 1, cr = (int64_t)right[p] - 1;
    PairRef q;
    q.l = column(cl);
    q.r = column(cr);
    q.sl = scale ? scale[cl] : 1.0;
    q.sr = scale ? scale[cr] : 1.0;
    out[p] = q;
}

// this thread's two genes of a column: VEC 2 adjacent ones in one 16-byte load, VEC 1 the genes g0 and g1
template <int VEC>
__device__ __forceinline__ void load2(const double* __restrict__ col, int g0, int g1, double& a, double& b) {
    // (the column's address came out of memory: say that it is global memory, or the loads are flat ones)
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    typedef const __attribute__((address_space(1))) double* gptr;
    typedef const __attribute__((address_space(1))) f64x2* gptr2;
    if (VEC == 2) {
        const f64x2 v = *(gptr2)(col + g0);
        a = v.x;
        b = v.y;
    } else {
        a = *(gptr)(col + g0);
        b = *(gptr)(col + g1);
    }
}

// PASS 1: acc = {sum s_l x_left, sum s_r x_right} for both genes; PASS 2: acc = {sum (delta - mean delta)^2}
template <int PASS>
__device__ __forceinline__ void add_pair(const PairRef& q, double l0, double l1, double r0, double r1, double m0, double m1,
                                         double (&acc)[4]) {
    const double vl0 = q.sl * l0, vl1 = q.sl * l1, vr0 = q.sr * r0, vr1 = q.sr * r1;
    if (PASS == 1) {
        acc[0] += vl0;
        acc[1] += vl1;
        acc[2] += vr0;
        acc[3] += vr1;
    } else {
        const double d0 = (vl0 - vr0) - m0, d1 = (vl1 - vr1) - m1;
        acc[0] += d0 * d0;
        acc[1] += d1 * d1;
    }
}

// grid: chunks x gene tiles.  PASS 1: out_a[ch][g], out_b[ch][g] the chunk's two sums; PASS 2: out_a[ch][g] its sum of
// centred squares, mdelta [steps][G] the steps' mean deltas.  The pair records are read through uniform addresses.
template <int VEC, int PASS>
__global__ __launch_bounds__(TPB) void pair_pass_kernel(const PairRef* __restrict__ pairs, const ChunkRef* __restrict__ chunks,
                                                        int G, const double* __restrict__ mdelta,
                                                        double* __restrict__ out_a, double* __restrict__ out_b) {
    const int ch = blockIdx.x;
    const int t0 = blockIdx.y * GT;
    const int g0 = VEC == 2 ? t0 + 2 * (int)threadIdx.x : t0 + (int)threadIdx.x;
    if (g0 >= G) return;  // (VEC 2: G is even, so g0 + 1 is a gene too)
    const int g1 = VEC == 2 ? g0 + 1 : g0 + TPB;
    const bool has1 = g1 < G;
    const int g1c = has1 ? g1 : G - 1;  // a lane without a second gene reads the last one and drops it
    const ChunkRef c = chunks[ch];
    const PairRef* __restrict__ q = pairs + c.begin;
    double m0 = 0.0, m1 = 0.0;
    if (PASS == 2) {
        m0 = mdelta[(int64_t)c.step * G + g0];
        m1 = mdelta[(int64_t)c.step * G + g1c];
    }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const double* kept = nullptr;  // the column k0 / k1 hold
    double k0 = 0.0, k1 = 0.0;
    int i = 0;
    for (; i + 4 <= c.len; i += 4) {
        const PairRef p0 = q[i], p1 = q[i + 1], p2 = q[i + 2], p3 = q[i + 3];
        double r00, r01, r10, r11, r20, r21, r30, r31;
        // (each branch issues all its loads in one go: a load ahead of the branch would be waited for at the branch)
        if (p0.l == p1.l && p1.l == p2.l && p2.l == p3.l) {  // (uniform) one left cell: read once, or not at all
            if (p0.l != kept) {
                load2<VEC>(p0.l, g0, g1c, k0, k1);
                kept = p0.l;
            }
            load2<VEC>(p0.r, g0, g1c, r00, r01);
            load2<VEC>(p1.r, g0, g1c, r10, r11);
            load2<VEC>(p2.r, g0, g1c, r20, r21);
            load2<VEC>(p3.r, g0, g1c, r30, r31);
            add_pair<PASS>(p0, k0, k1, r00, r01, m0, m1, acc);
            add_pair<PASS>(p1, k0, k1, r10, r11, m0, m1, acc);
            add_pair<PASS>(p2, k0, k1, r20, r21, m0, m1, acc);
            add_pair<PASS>(p3, k0, k1, r30, r31, m0, m1, acc);
        } else {
            double l00, l01, l10, l11, l20, l21;
            load2<VEC>(p0.r, g0, g1c, r00, r01);
            load2<VEC>(p1.r, g0, g1c, r10, r11);
            load2<VEC>(p2.r, g0, g1c, r20, r21);
            load2<VEC>(p3.r, g0, g1c, r30, r31);
            load2<VEC>(p0.l, g0, g1c, l00, l01);
            load2<VEC>(p1.l, g0, g1c, l10, l11);
            load2<VEC>(p2.l, g0, g1c, l20, l21);
            load2<VEC>(p3.l, g0, g1c, k0, k1);
            kept = p3.l;
            add_pair<PASS>(p0, l00, l01, r00, r01, m0, m1, acc);
            add_pair<PASS>(p1, l10, l11, r10, r11, m0, m1, acc);
            add_pair<PASS>(p2, l20, l21, r20, r21, m0, m1, acc);
            add_pair<PASS>(p3, k0, k1, r30, r31, m0, m1, acc);
        }
    }
    for (; i < c.len; ++i) {
        const PairRef p = q[i];
        double r0, r1;
        load2<VEC>(p.r, g0, g1c, r0, r1);
        if (p.l != kept) {
            load2<VEC>(p.l, g0, g1c, k0, k1);
            kept = p.l;
        }
        add_pair<PASS>(p, k0, k1, r0, r1, m0, m1, acc);
    }
    const int64_t row = (int64_t)ch * G;
    if (PASS == 1) {
        out_a[row + g0] = acc[0];
        out_b[row + g0] = acc[2];
        if (has1) {
            out_a[row + g1] = acc[1];
            out_b[row + g1] = acc[3];
        }
    } else {
        out_a[row + g0] = acc[0];
        if (has1) out_a[row + g1] = acc[1];
    }
}

// step s, gene g: the chunk sums of the step in ascending order; mean = (mean left + mean right) / 2 (:197), mdelta = mean
// left - mean right.  chunk0 [steps + 1], npairs [steps].
__global__ __launch_bounds__(256) void mean_reduce_kernel(const double* __restrict__ part_l, const double* __restrict__ part_r,
                                                          int G, const int32_t* __restrict__ chunk0,
                                                          const int64_t* __restrict__ npairs, double* __restrict__ mean,
                                                          double* __restrict__ mdelta) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int s = blockIdx.y;
    if (g >= G) return;
    const double2 lr = fold_ascending<8>(make_double2(0.0, 0.0), chunk0[s], chunk0[s + 1], [&](int ch) {
        return make_double2(part_l[(int64_t)ch * G + g], part_r[(int64_t)ch * G + g]);
    });
    const double P = (double)npairs[s];
    const double ml = lr.x / P, mr = lr.y / P;  // (no pairs: NaN, as rowMeans of no columns)
    mean[(int64_t)s * G + g] = (ml + mr) / 2.0;
    mdelta[(int64_t)s * G + g] = ml - mr;
}

// total = (sum of the chunks' centred squares, ascending) / (P - 1); NaN below two pairs
__global__ __launch_bounds__(256) void total_reduce_kernel(const double* __restrict__ part, int G,
                                                           const int32_t* __restrict__ chunk0,
                                                           const int64_t* __restrict__ npairs, double* __restrict__ total) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int s = blockIdx.y;
    if (g >= G) return;
    const double v = fold_ascending<8>(0.0, chunk0[s], chunk0[s + 1], [&](int ch) { return part[(int64_t)ch * G + g]; });
    const int64_t P = npairs[s];
    total[(int64_t)s * G + g] = P >= 2 ? v / (double)(P - 1) : __longlong_as_double(0x7ff8000000000000ll);
}

// ---- batches kept as CSC: per batch indptr [n + 1] absolute positions into idx / val.  indptr has been checked on the
// host (non-decreasing, within the arrays), idx and val are checked by sp_check_kernel.
constexpr int ST = DELTA_SPARSE_GENE_TILE;
enum { SP_F_VALUE = CSC_F_WORDS, SP_F_WORDS };  // behind the pattern pair: a value that is not finite

struct CscRef {
    const int64_t* indptr;
    const int32_t* idx;
    const double* val;
};
struct SparsePairRef {
    const int32_t* li;  // the left cell's rows and values, and how many it stores
    const double* lv;
    int64_t ln;
    const int32_t* ri;
    const double* rv;
    int64_t rn;
    double sl, sr;  // the two scales (1 without cos.norm)
};

// The entries of the cells [c0, c0 + m), one wave a cell: the pattern flags (csc_entry_flags) and the values.
__global__ __launch_bounds__(256) void sp_check_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                       const double* __restrict__ val, int G, int64_t c0, int64_t m,
                                                       int32_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int64_t c = c0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= c0 + m) return;  // (a whole wave leaves)
    const int64_t kb = indptr[c], ke = indptr[c + 1];
    int bad = 0, bad_row = 0, bad_order = 0;
    for (int64_t k = kb + lane; k < ke; k += 64) {
        bad |= !(fabs(val[k]) <= std::numeric_limits<double>::max());
        (void)csc_entry_flags(idx, k, kb, idx[k], G, bad_row, bad_order);
    }
    if (bad_row) flags[CSC_F_ROW] = 1;
    if (bad_order) flags[CSC_F_ORDER] = 1;
    if (bad) flags[SP_F_VALUE] = 1;
}

// l2[c] of the cells [0, n) of a batch, one wave a cell: lane l adds the squares of the column's entries l, l + 64, ...,
// then the lanes are added in a fixed order.  mult (nullable) [G]: how often a gene is in the list of the norm genes.
__global__ __launch_bounds__(256) void sp_l2_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                    const double* __restrict__ val, int G, int64_t n,
                                                    const int32_t* __restrict__ mult, double* __restrict__ l2) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= n) return;  // (a whole wave leaves)
    const int64_t kb = indptr[c], ke = indptr[c + 1];
    double s = 0.0;
    for (int64_t k = kb + lane; k < ke; k += 64) {
        const int32_t r = idx[k];
        if (r < 0 || r >= G) continue;
        const double v = val[k];
        if (!mult) s += v * v;
        else if (mult[r] > 0) s += (double)mult[r] * (v * v);
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) l2[c] = sqrt(s);
}

// pair_prep_kernel for CSC batches: base [B] the batches' three arrays
__global__ __launch_bounds__(256) void sp_pair_prep_kernel(const int32_t* __restrict__ left, const int32_t* __restrict__ right,
                                                           int64_t P, const int64_t* __restrict__ off, int B,
                                                           const CscRef* __restrict__ base, const double* __restrict__ scale,
                                                           SparsePairRef* __restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    auto column = [&](int64_t c, const int32_t*& idx, const double*& val, int64_t& n) {
        int lo = 0, hi = B - 1;  // the last batch that starts at or before c
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (off[mid] <= c) lo = mid; else hi = mid - 1;
        }
        const CscRef b = base[lo];
        const int64_t kb = b.indptr[c - off[lo]], ke = b.indptr[c - off[lo] + 1];
        idx = b.idx + kb;
        val = b.val + kb;
        n = ke - kb;
    };
    const int64_t cl = (int64_t)left[p] - 1, cr = (int64_t)right[p] - 1;
    SparsePairRef q;
    column(cl, q.li, q.lv, q.ln);
    column(cr, q.ri, q.rv, q.rn);
    q.sl = scale ? scale[cl] : 1.0;
    q.sr = scale ? scale[cr] : 1.0;
    out[p] = q;
}

// grid: chunks x gene tiles of ST genes, a workgroup of ONE wave (every barrier below is then a wait for the wave's own
// LDS queue).  Lane l first finds the tile's entries in the columns of the chunk's pairs l and l + 64; then the pairs are
// taken in order.  A column that is canonical -- every column is: a run refuses the others before this kernel starts --
// has at most ST entries in the tile and no row twice, so no two lanes meet at a gene within a column.
//   PASS 1: a / b = the tile's sums of s_l x_left and s_r x_right; out_a[ch][g], out_b[ch][g].
//   PASS 2: b takes the left column's values (stamp: by which pair of the chunk), the right column's are taken off them
//           or, where the left cell stores nothing, squared at once; then the left lanes read the deltas back.  a = the sum
//           of (delta - mean delta)^2 over the pairs that store the gene, touched = how many those are;
//           out_a[ch][g] = a + ((pairs - touched) * mdelta) * mdelta.
template <int PASS>
__global__ __launch_bounds__(64) void sp_pair_pass_kernel(const SparsePairRef* __restrict__ pairs,
                                                          const ChunkRef* __restrict__ chunks, int G,
                                                          const double* __restrict__ mdelta, double* __restrict__ out_a,
                                                          double* __restrict__ out_b) {
    constexpr int SECOND = PASS == 2 ? ST : 1;
    __shared__ double a[ST], b[ST];
    __shared__ double md[SECOND];
    __shared__ int32_t stamp[SECOND], touched[SECOND];
    __shared__ int32_t lo_l[PC], n_l[PC], lo_r[PC], n_r[PC];
    const int lane = threadIdx.x;
    const int ch = blockIdx.x;
    const int g0 = blockIdx.y * ST, g1 = min(G, g0 + ST);
    const ChunkRef c = chunks[ch];
    const SparsePairRef* __restrict__ q = pairs + c.begin;
    for (int i = lane; i < g1 - g0; i += 64) {
        a[i] = 0.0;
        b[i] = 0.0;
        if (PASS == 2) {
            md[i] = mdelta[(int64_t)c.step * G + g0 + i];
            stamp[i] = 0;
            touched[i] = 0;
        }
    }
    for (int j = lane; j < c.len; j += 64) {
        const SparsePairRef p = q[j];
        const int64_t fl = first_row_at_least(p.li, 0, p.ln, g0), fr = first_row_at_least(p.ri, 0, p.rn, g0);
        lo_l[j] = (int32_t)fl;
        n_l[j] = (int32_t)(first_row_at_least(p.li, fl, p.ln, g1) - fl);
        lo_r[j] = (int32_t)fr;
        n_r[j] = (int32_t)(first_row_at_least(p.ri, fr, p.rn, g1) - fr);
    }
    __syncthreads();
    for (int j = 0; j < c.len; ++j) {
        const SparsePairRef p = q[j];  // (a uniform address)
        const int nl = n_l[j], nr = n_r[j];
        const csc_rows_ptr li = (csc_rows_ptr)(p.li + lo_l[j]), ri = (csc_rows_ptr)(p.ri + lo_r[j]);
        const csc_vals_ptr lv = (csc_vals_ptr)(p.lv + lo_l[j]), rv = (csc_vals_ptr)(p.rv + lo_r[j]);
        int rl = -1, rr = -1;  // this lane's first entry of either column: four loads in flight
        double vl = 0.0, vr = 0.0;
        if (lane < nl) {
            rl = li[lane];
            vl = lv[lane];
        }
        if (lane < nr) {
            rr = ri[lane];
            vr = rv[lane];
        }
        if (PASS == 1) {
            csc_wave_walk(li, lv, nl, lane, g0, g1, rl, vl, [&](int i, double v) { a[i] += p.sl * v; });
            csc_wave_walk(ri, rv, nr, lane, g0, g1, rr, vr, [&](int i, double v) { b[i] += p.sr * v; });
            __syncthreads();
        } else {
            const int32_t tag = j + 1;
            csc_wave_walk(li, lv, nl, lane, g0, g1, rl, vl, [&](int i, double v) {
                b[i] = p.sl * v;
                stamp[i] = tag;
            });
            __syncthreads();
            csc_wave_walk(ri, rv, nr, lane, g0, g1, rr, vr, [&](int i, double v) {
                const double x = p.sr * v;
                if (stamp[i] == tag) {
                    b[i] = b[i] - x;
                } else {  // the left cell stores no entry of this gene: s_l * 0 - s_r x_right
                    const double d = (0.0 - x) - md[i];
                    a[i] += d * d;
                    touched[i] += 1;
                }
            });
            __syncthreads();
            csc_wave_walk(li, lv, nl, lane, g0, g1, rl, vl, [&](int i, double) {
                const double d = b[i] - md[i];
                a[i] += d * d;
                touched[i] += 1;
            });
            __syncthreads();
        }
    }
    const int64_t row = (int64_t)ch * G + g0;
    for (int i = lane; i < g1 - g0; i += 64) {
        if (PASS == 1) {
            out_a[row + i] = a[i];
            out_b[row + i] = b[i];
        } else {
            const double m = md[i];
            out_a[row + i] = a[i] + ((double)(c.len - touched[i]) * m) * m;
        }
    }
}

}  // namespace

// what Delta::run takes
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

inline DeltaRun delta_run_args(int cos_norm, const int32_t* norm_genes0, int n_norm_genes, int nsteps,
                               const int32_t* const* left, const int32_t* const* right, const int64_t* npairs, double* mean,
                               double* total) {
    DeltaRun a;
    a.cos_norm = cos_norm;
    a.norm_genes0 = norm_genes0;
    a.n_norm_genes = n_norm_genes;
    a.nsteps = nsteps;
    a.left = left;
    a.right = right;
    a.npairs = npairs;
    a.mean = mean;
    a.total = total;
    return a;
}

// argument checks of Delta::begin_batch / run without a device (throw Error): G genes, N cells uploaded so far
void delta_check_batch(int64_t n, int64_t cells_before) {
    check_cell_count(n);
    if (cells_before + n > 0x7fffffffll) throw Error(BMX_ERR_ARG, "the batches hold at most 2^31 - 1 cells together");
}

void delta_check_run(int G, int64_t N, const DeltaRun& a) {
    if (a.nsteps < 1) throw Error(BMX_ERR_ARG, "'pairs' must hold at least one merge step");
    if (!a.left || !a.right || !a.npairs) throw Error(BMX_ERR_ARG, "the pair lists are missing");
    if (!a.mean || !a.total) throw Error(BMX_ERR_ARG, "an output matrix is missing");
    if (a.n_norm_genes < 0 || (a.norm_genes0 && a.n_norm_genes < 1) || (!a.norm_genes0 && a.n_norm_genes > 0))
        throw Error(BMX_ERR_ARG, "invalid gene list for the cosine norms");
    for (int i = 0; i < a.n_norm_genes; ++i)
        if (a.norm_genes0[i] < 0 || a.norm_genes0[i] >= G) throw Error(BMX_ERR_SUBSET, "subset indices out of range");
    int64_t chunks = 0;
    for (int s = 0; s < a.nsteps; ++s) {
        const int64_t P = a.npairs[s];
        if (P < 0) throw Error(BMX_ERR_ARG, "a merge step has a negative number of pairs");
        if (P > 0 && (!a.left[s] || !a.right[s])) throw Error(BMX_ERR_ARG, "a merge step's pair list is missing");
        for (int64_t p = 0; p < P; ++p)
            if (a.left[s][p] < 1 || a.left[s][p] > N || a.right[s][p] < 1 || a.right[s][p] > N)
                throw Error(BMX_ERR_ARG, "'pairs' indices out of range");
        chunks += (P + PC - 1) / PC;
    }
    if (chunks > 0x7fffffffll) throw Error(BMX_ERR_ARG, "too many pairs");
}

// What the dense and the CSC handle share: the batches stay resident, and the per-gene mean and variance of the MNN-pair
// deltas of every merge step come out of one run.  The handle says how its batches give the cell norms, a pair's record
// and the two pair passes; the chunks, the reductions over them and the download are here.
template <class Batch>
class DeltaBase : protected ResidentBatches<Batch> {
  protected:
    using Store = ResidentBatches<Batch>;
    using Store::batches_;
    using Store::cache_;
    using Store::device_;
    using Store::G_;
    using Store::ms_;
    using Store::stream_;
    using Store::timer_;
    using Store::Store;
    ~DeltaBase() = default;  // (the handle's own destructor calls retire(): resident_batches.hpp)

    // the words of 8 bytes of a pair's record
    virtual size_t pair_record_words() const = 0;
    // on stream_, before run() waits for it: the tables of the batches' addresses, and with norm_genes0 the norm genes
    virtual void stage_tables(const DeltaRun& a) = 0;
    // after that wait: what the device has found wrong with the batches (throw Error)
    virtual void check_batches() {}
    // l2[off[b] + c] = the l2 of cell c of batch b over the norm genes staged
    virtual void launch_l2(const DeltaRun& a, const std::vector<int64_t>& off, double* l2) = 0;
    // records [Ptot] from the 1-based columns left / right; d_off [B + 1] the batches' first columns, scale nullable
    virtual void launch_prep(const int32_t* d_left, const int32_t* d_right, int64_t Ptot, const int64_t* d_off,
                             const double* d_scale, void* records) = 0;
    // pass 1: part / part_r [chunks][G] the chunks' two sums; pass 2: part the chunks' sums of centred squares
    virtual void launch_pass(int pass, int nch, const void* records, const ChunkRef* d_chunks, const double* d_mdelta,
                             double* part, double* part_r) = 0;

    // free HBM holds `need` bytes more (parked blocks of earlier handles count as free memory), or Error; what is free
    size_t check_room(size_t need) {
        size_t free_b = 0, total_b = 0;
        BMX_HIP(hipMemGetInfo(&free_b, &total_b));
        if (need > free_b) {
            DevBlockCache::release_global();
            BMX_HIP(hipMemGetInfo(&free_b, &total_b));
        }
        if (need > free_b) throw Error(BMX_ERR_HIP, no_room(need, free_b));
        return free_b;
    }
    // begin(): a failed allocation is reported as check_room reports it
    template <class F>
    void begin_with_room(size_t need, size_t free_b, F&& begin) {
        try {
            begin();
        } catch (const Error& e) {
            if (std::string(e.what()).find("hipMalloc failed") == std::string::npos) throw;
            throw Error(BMX_ERR_HIP, no_room(need, free_b));
        }
    }

  public:
    void run(const DeltaRun& a) {
        if (batches_.empty()) throw Error(BMX_ERR_ARG, "no batch has been added");
        for (auto& b : batches_)
            if (!b->complete()) throw Error(BMX_ERR_ARG, "a batch has not received all its cells");
        const int64_t N = cells();
        delta_check_run(G_, N, a);
        const double t0 = now_ms();
        CacheScope scope(&cache_);
        BMX_HIP(hipSetDevice(device_));
        const int G = G_, B = (int)batches_.size(), S = a.nsteps;

        // the steps' lists side by side, cut into chunks at fixed positions of each list
        std::vector<int64_t> npairs(a.npairs, a.npairs + S), off((size_t)B + 1, 0);
        std::vector<int32_t> chunk0((size_t)S + 1, 0);
        std::vector<ChunkRef> chunks;
        int64_t Ptot = 0;
        for (int s = 0; s < S; ++s) {
            for (int64_t b = 0; b < npairs[(size_t)s]; b += PC)
                chunks.push_back({Ptot + b, (int32_t)std::min<int64_t>(PC, npairs[(size_t)s] - b), s});
            Ptot += npairs[(size_t)s];
            chunk0[(size_t)s + 1] = (int32_t)chunks.size();
        }
        const int nch = (int)chunks.size();
        for (int b = 0; b < B; ++b) off[(size_t)b + 1] = off[(size_t)b] + batches_[(size_t)b]->n;

        int32_t* d_left = left_.reserve((size_t)std::max<int64_t>(Ptot, 1));
        int32_t* d_right = right_.reserve((size_t)std::max<int64_t>(Ptot, 1));
        void* d_pairs = pairs_.reserve((size_t)std::max<int64_t>(Ptot, 1) * pair_record_words());
        ChunkRef* d_chunks = reinterpret_cast<ChunkRef*>(chunks_.reserve((size_t)std::max(nch, 1) * (sizeof(ChunkRef) / 8)));
        int64_t* d_off = off_.reserve((size_t)B + 1 + (size_t)S);  // off [B + 1], npairs [S]
        int64_t* d_np = d_off + B + 1;
        int32_t* d_chunk0 = chunk0_.reserve((size_t)S + 1);
        double* part = part_.reserve((size_t)std::max(nch, 1) * G * 2);  // [2][chunks][G]
        double* part_r = part + (size_t)std::max(nch, 1) * G;
        double* stats = stats_.reserve((size_t)S * G * 3);  // mean [S][G], total [S][G], mean delta [S][G]
        double* d_mean = stats;
        double* d_total = stats + (size_t)S * G;
        double* d_mdelta = d_total + (size_t)S * G;

        int64_t at = 0;
        for (int s = 0; s < S; ++s) {
            const size_t bytes = (size_t)npairs[(size_t)s] * sizeof(int32_t);
            if (bytes) {
                upload_small(d_left + at, a.left[s], bytes);
                upload_small(d_right + at, a.right[s], bytes);
            }
            at += npairs[(size_t)s];
        }
        if (nch) upload_small(d_chunks, chunks.data(), (size_t)nch * sizeof(ChunkRef));
        upload_small(d_off, off.data(), ((size_t)B + 1) * sizeof(int64_t));
        upload_small(d_np, npairs.data(), (size_t)S * sizeof(int64_t));
        upload_small(d_chunk0, chunk0.data(), ((size_t)S + 1) * sizeof(int32_t));
        stage_tables(a);
        BMX_HIP(hipStreamSynchronize(stream_));  // (the host vectors may go; the caller's lists have been read)
        check_batches();

        const double* d_scale = nullptr;
        if (a.cos_norm) {
            double* l2 = l2_.reserve((size_t)N * 2 + (size_t)B);  // l2 [N], scale [N], bmean [B]
            double* scale = l2 + N;
            double* bmean = scale + N;
            const int e0 = timer_.mark(stream_);
            launch_l2(a, off, l2);
            hipLaunchKernelGGL(l2_mean_kernel, dim3((unsigned)B), dim3(256), 0, stream_, (const double*)l2,
                               (const int64_t*)d_off, bmean);
            BMX_LAUNCH_CHECK();
            hipLaunchKernelGGL(scale_kernel, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, stream_, (const double*)l2, N,
                               (const double*)bmean, B, scale);
            BMX_LAUNCH_CHECK();
            timer_.span(1, e0, timer_.mark(stream_));
            d_scale = scale;
        }

        const dim3 rgrid((unsigned)cdiv(G, 256), (unsigned)S);
        const int e1 = timer_.mark(stream_);
        if (Ptot > 0) {
            launch_prep(d_left, d_right, Ptot, d_off, d_scale, d_pairs);
            BMX_LAUNCH_CHECK();
        }
        const int e2 = timer_.mark(stream_);
        timer_.span(3, e1, e2);
        if (nch > 0) {
            launch_pass(1, nch, d_pairs, d_chunks, nullptr, part, part_r);
            BMX_LAUNCH_CHECK();
        }
        const int e3 = timer_.mark(stream_);
        timer_.span(2, e2, e3);
        hipLaunchKernelGGL(mean_reduce_kernel, rgrid, dim3(256), 0, stream_, (const double*)part, (const double*)part_r, G,
                           (const int32_t*)d_chunk0, (const int64_t*)d_np, d_mean, d_mdelta);
        BMX_LAUNCH_CHECK();
        const int e4 = timer_.mark(stream_);
        timer_.span(3, e3, e4);
        if (nch > 0) {
            launch_pass(2, nch, d_pairs, d_chunks, d_mdelta, part, nullptr);
            BMX_LAUNCH_CHECK();
        }
        const int e5 = timer_.mark(stream_);
        timer_.span(2, e4, e5);
        hipLaunchKernelGGL(total_reduce_kernel, rgrid, dim3(256), 0, stream_, (const double*)part, G,
                           (const int32_t*)d_chunk0, (const int64_t*)d_np, d_total);
        BMX_LAUNCH_CHECK();
        timer_.span(3, e5, timer_.mark(stream_));

        // the statistics of all steps in one download
        host_.resize((size_t)S * G * 2);
        BMX_HIP(hipMemcpyAsync(host_.data(), stats, host_.size() * sizeof(double), hipMemcpyDeviceToHost, stream_));
        BMX_HIP(hipStreamSynchronize(stream_));
        std::memcpy(a.mean, host_.data(), (size_t)S * G * sizeof(double));
        std::memcpy(a.total, host_.data() + (size_t)S * G, (size_t)S * G * sizeof(double));
        timer_.collect(ms_);
        ms_[4] += now_ms() - t0;
    }

    // milliseconds since the handle was made: upload (host wall time), HIP-event time of the cell norms, of the two pair
    // passes, of the pair preparation and the reductions over chunks, and the host wall time of the runs
    using Store::stage_ms;

  protected:
    int64_t cells() const {
        int64_t N = 0;
        for (auto& b : batches_) N += b->n;
        return N;
    }
    static std::string no_room(size_t need, size_t free_b) {
        return "the batches do not fit in free HBM (this batch needs " + std::to_string(need >> 20) + " MiB, " +
               std::to_string(free_b >> 20) + " MiB are free): use 'subset_row' to restrict the genes";
    }
    void upload_small(void* dev, const void* host, size_t bytes) {
        if (bytes >= ((size_t)1 << 20))
            upload_pageable(dev, host, bytes, stream_);
        else
            BMX_HIP(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, stream_));
    }

    DevBuf<int32_t> left_, right_, chunk0_;
    DevBuf<int64_t> off_;
    DevBuf<double> pairs_, chunks_, part_, stats_, l2_;  // (pairs_, chunks_: records of 8-byte words)
    std::vector<double> host_;
};

struct DeltaBatch : ResidentBatch {};

// genes x cells FP64 matrices, column-major
class Delta : public DeltaBase<DeltaBatch> {
  public:
    Delta(int device, int G) : DeltaBase(device, G, "bmx_delta_begin_batch") {}
    ~Delta() { retire(); }

    void begin_batch(int64_t n) {
        delta_check_batch(n, cells());
        check_begin(batches_.empty() ? nullptr : batches_.back().get());
        BMX_HIP(hipSetDevice(device_));
        const size_t elems = (size_t)n * G_;
        const size_t need = (elems + elems / 8 + 64) * sizeof(double);  // what DevBuf::reserve asks for
        const size_t free_b = check_room(need);
        begin_with_room(need, free_b, [&] { begin(n, [](DeltaBatch&) {}); });
    }

    void add_block(const double* x_block, int64_t m) {
        const double t0 = now_ms();
        add(x_block, m, [&](DeltaBatch& b, double*) {
            if (b.complete()) BMX_HIP(hipStreamSynchronize(stream_));
        });
        ms_[0] += now_ms() - t0;
    }

  private:
    size_t pair_record_words() const override { return sizeof(PairRef) / 8; }
    void stage_tables(const DeltaRun& a) override {
        const size_t B = batches_.size();
        hbase_.resize(B);  // (a member: it is read until run() has waited for the stream)
        for (size_t b = 0; b < B; ++b) hbase_[b] = batches_[b]->x.p;
        upload_small(base_.reserve(B), hbase_.data(), B * sizeof(double*));
        if (a.cos_norm && a.norm_genes0)
            upload_small(genes_.reserve((size_t)a.n_norm_genes), a.norm_genes0, (size_t)a.n_norm_genes * sizeof(int32_t));
    }
    void launch_l2(const DeltaRun& a, const std::vector<int64_t>& off, double* l2) override {
        for (size_t b = 0; b < batches_.size(); ++b)
            cell_l2_device(stream_, batches_[b]->x.p, G_, batches_[b]->n, a.norm_genes0 ? genes_.p : nullptr, a.n_norm_genes,
                           false, l2 + off[b]);
    }
    void launch_prep(const int32_t* d_left, const int32_t* d_right, int64_t Ptot, const int64_t* d_off, const double* d_scale,
                     void* records) override {
        hipLaunchKernelGGL(pair_prep_kernel, dim3((unsigned)cdiv(Ptot, 256)), dim3(256), 0, stream_, d_left, d_right, Ptot,
                           d_off, (int)batches_.size(), reinterpret_cast<const double* const*>(base_.p), G_, d_scale,
                           static_cast<PairRef*>(records));
    }
    void launch_pass(int pass, int nch, const void* records, const ChunkRef* d_chunks, const double* d_mdelta, double* part,
                     double* part_r) override {
        const dim3 pgrid((unsigned)nch, (unsigned)cdiv(G_, GT));
        const PairRef* d_pairs = static_cast<const PairRef*>(records);
        auto kernel = G_ % 2 == 0 ? (pass == 1 ? pair_pass_kernel<2, 1> : pair_pass_kernel<2, 2>)
                                  : (pass == 1 ? pair_pass_kernel<1, 1> : pair_pass_kernel<1, 2>);
        hipLaunchKernelGGL(kernel, pgrid, dim3(TPB), 0, stream_, d_pairs, d_chunks, G_, d_mdelta, part, part_r);
    }

    DevBuf<int32_t> genes_;
    DevBuf<double> base_;  // (the batches' addresses)
    std::vector<const double*> hbase_;
};

// ---- the same over batches kept as CSC (indptr int64, 0-based int32 rows, FP64 values), whose cells arrive in column
// blocks; every stored entry is checked behind its upload, and a run refuses what the check has found
struct DeltaCscBatch : CscBatch {};

class DeltaSparse : public DeltaBase<DeltaCscBatch> {
  public:
    DeltaSparse(int device, int G) : DeltaBase(device, G, "bmx_delta_sparse_begin_batch") {
        CacheScope scope(&cache_);
        BMX_HIP(hipMemsetAsync(flags_.reserve(SP_F_WORDS), 0, SP_F_WORDS * sizeof(int32_t), stream_));
        BMX_HIP(hipStreamSynchronize(stream_));
    }
    ~DeltaSparse() { retire(); }

    // a batch of n cells with nnz stored entries in all
    void begin_batch(int64_t n, int64_t nnz) {
        delta_check_batch(n, cells());
        check_csc_begin(nnz);
        check_begin(batches_.empty() ? nullptr : batches_.back().get());
        BMX_HIP(hipSetDevice(device_));
        const size_t ne = (size_t)std::max<int64_t>(nnz, 1);  // what the three DevBuf::reserve ask for
        const size_t need = ((size_t)n + 1 + ((size_t)n + 1) / 8 + 64) * sizeof(int64_t) +
                            (ne + ne / 8 + 64) * (sizeof(int32_t) + sizeof(double));
        const size_t free_b = check_room(need);
        begin_with_room(need, free_b, [&] { begin_csc(n, nnz, [](DeltaCscBatch&) {}); });
    }

    // the next m cells of the batch begun last: indptr [m + 1] relative to the block, its nnz entries (pageable)
    void add_block(int64_t m, const int64_t* indptr, const int32_t* indices, const double* data, int64_t nnz) {
        const double t0 = now_ms();
        DeltaCscBatch* open = batches_.empty() ? nullptr : batches_.back().get();
        check_block(open, indptr, m, begin_entry_);  // (add_csc's checks, here ahead of its first device call)
        check_csc_block(open->n, open->filled, m, indptr, indices, data, nnz);
        check_csc_entries(*open, m, nnz);
        add_csc(m, indptr, indices, data, nnz, [&](DeltaCscBatch& b, int64_t c0) {
            hipLaunchKernelGGL(sp_check_kernel, dim3((unsigned)cdiv(m, 4)), dim3(256), 0, stream_, (const int64_t*)b.indptr.p,
                               (const int32_t*)b.indices.p, (const double*)b.data.p, G_, c0, m, flags_.p);
            BMX_LAUNCH_CHECK();
            if (b.complete()) BMX_HIP(hipStreamSynchronize(stream_));
        });
        ms_[0] += now_ms() - t0;
    }

  private:
    size_t pair_record_words() const override { return sizeof(SparsePairRef) / 8; }
    void stage_tables(const DeltaRun& a) override {
        const size_t B = batches_.size();
        hbase_.resize(B);  // (members: they are read until run() has waited for the stream)
        for (size_t b = 0; b < B; ++b) hbase_[b] = {batches_[b]->indptr.p, batches_[b]->indices.p, batches_[b]->data.p};
        upload_small(base_.reserve(B * (sizeof(CscRef) / 8)), hbase_.data(), B * sizeof(CscRef));
        if (a.cos_norm && a.norm_genes0) {  // how often each gene is in the list
            hmult_.assign((size_t)G_, 0);
            for (int i = 0; i < a.n_norm_genes; ++i) hmult_[(size_t)a.norm_genes0[i]] += 1;
            upload_small(mult_.reserve((size_t)G_), hmult_.data(), (size_t)G_ * sizeof(int32_t));
        }
        BMX_HIP(hipMemcpyAsync(found_, flags_.p, sizeof(found_), hipMemcpyDeviceToHost, stream_));
    }
    void check_batches() override {
        throw_if_bad_pattern(found_);
        if (found_[SP_F_VALUE]) throw Error(BMX_ERR_ARG, "values should be finite");
    }
    void launch_l2(const DeltaRun& a, const std::vector<int64_t>& off, double* l2) override {
        for (size_t b = 0; b < batches_.size(); ++b) {
            const DeltaCscBatch& bt = *batches_[b];
            hipLaunchKernelGGL(sp_l2_kernel, dim3((unsigned)cdiv(bt.n, 4)), dim3(256), 0, stream_, (const int64_t*)bt.indptr.p,
                               (const int32_t*)bt.indices.p, (const double*)bt.data.p, G_, bt.n,
                               (const int32_t*)(a.norm_genes0 ? mult_.p : nullptr), l2 + off[b]);
            BMX_LAUNCH_CHECK();
        }
    }
    void launch_prep(const int32_t* d_left, const int32_t* d_right, int64_t Ptot, const int64_t* d_off, const double* d_scale,
                     void* records) override {
        hipLaunchKernelGGL(sp_pair_prep_kernel, dim3((unsigned)cdiv(Ptot, 256)), dim3(256), 0, stream_, d_left, d_right, Ptot,
                           d_off, (int)batches_.size(), reinterpret_cast<const CscRef*>(base_.p), d_scale,
                           static_cast<SparsePairRef*>(records));
    }
    void launch_pass(int pass, int nch, const void* records, const ChunkRef* d_chunks, const double* d_mdelta, double* part,
                     double* part_r) override {
        const dim3 pgrid((unsigned)nch, (unsigned)cdiv(G_, ST));
        const SparsePairRef* d_pairs = static_cast<const SparsePairRef*>(records);
        hipLaunchKernelGGL(pass == 1 ? sp_pair_pass_kernel<1> : sp_pair_pass_kernel<2>, pgrid, dim3(64), 0, stream_, d_pairs,
                           d_chunks, G_, d_mdelta, part, part_r);
    }

    DevBuf<int32_t> flags_, mult_;
    DevBuf<double> base_;  // (the batches' CscRef)
    std::vector<CscRef> hbase_;
    std::vector<int32_t> hmult_;
    int32_t found_[SP_F_WORDS] = {0, 0, 0};  // flags_ as the last run read it
};

}  // namespace bmx

/* ---------------------------------------------------------------- bmx_delta_*, bmx_delta_sparse_* --------------- */
struct bmx_delta final : bmx::Delta {
    using Delta::Delta;
};
struct bmx_delta_sparse final : bmx::DeltaSparse {
    using DeltaSparse::DeltaSparse;
};

extern "C" {

int32_t bmx_delta_create(int32_t device, int32_t G, bmx_delta_t** out) {
    return bmx::guarded([&] {
        if (!out) throw bmx::Error(BMX_ERR_ARG, "null output pointer");
        if (G < 1) throw bmx::Error(BMX_ERR_ARG, "mnnDeltaVariance needs at least one gene");
        *out = new bmx_delta(device, G);
    });
}

void bmx_delta_destroy(bmx_delta_t* h) { delete h; }

int32_t bmx_delta_begin_batch(bmx_delta_t* h, int64_t n) {
    return bmx::guarded([&] { bmx::live(h).begin_batch(n); });
}

int32_t bmx_delta_add_block(bmx_delta_t* h, const double* x_block, int64_t n_block) {
    return bmx::guarded([&] { bmx::live(h).add_block(x_block, n_block); });
}

int32_t bmx_delta_run(bmx_delta_t* h, int32_t cos_norm, const int32_t* norm_genes0, int32_t n_norm_genes, int32_t nsteps,
                      const int32_t* const* left, const int32_t* const* right, const int64_t* npairs, double* mean,
                      double* total) {
    return bmx::guarded([&] {
        // (delta_check_run comes before any device work)
        bmx::live(h).run(bmx::delta_run_args(cos_norm, norm_genes0, n_norm_genes, nsteps, left, right, npairs, mean, total));
    });
}

int32_t bmx_delta_stage_ms(const bmx_delta_t* h, double* out5) {
    return bmx::guarded([&] {
        if (!h || !out5) throw bmx::Error(BMX_ERR_ARG, "null argument");
        h->stage_ms(out5);
    });
}

int32_t bmx_delta_sparse_create(int32_t device, int32_t G, bmx_delta_sparse_t** out) {
    return bmx::guarded([&] {
        if (!out) throw bmx::Error(BMX_ERR_ARG, "null output pointer");
        if (G < 1) throw bmx::Error(BMX_ERR_ARG, "mnnDeltaVariance needs at least one gene");
        *out = new bmx_delta_sparse(device, G);
    });
}

void bmx_delta_sparse_destroy(bmx_delta_sparse_t* h) { delete h; }

int32_t bmx_delta_sparse_begin_batch(bmx_delta_sparse_t* h, int64_t n, int64_t nnz) {
    return bmx::guarded([&] { bmx::live(h).begin_batch(n, nnz); });
}

int32_t bmx_delta_sparse_add_block(bmx_delta_sparse_t* h, int64_t n_block, const int64_t* indptr, const int32_t* indices,
                                   const double* data, int64_t nnz) {
    return bmx::guarded([&] { bmx::live(h).add_block(n_block, indptr, indices, data, nnz); });
}

int32_t bmx_delta_sparse_run(bmx_delta_sparse_t* h, int32_t cos_norm, const int32_t* norm_genes0, int32_t n_norm_genes,
                             int32_t nsteps, const int32_t* const* left, const int32_t* const* right, const int64_t* npairs,
                             double* mean, double* total) {
    return bmx::guarded([&] {
        bmx::live(h).run(bmx::delta_run_args(cos_norm, norm_genes0, n_norm_genes, nsteps, left, right, npairs, mean, total));
    });
}

int32_t bmx_delta_sparse_stage_ms(const bmx_delta_sparse_t* h, double* out5) {
    return bmx::guarded([&] {
        if (!h || !out5) throw bmx::Error(BMX_ERR_ARG, "null argument");
        h->stage_ms(out5);
    });
}

}  // extern "C"
