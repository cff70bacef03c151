/*
 * batchelor_mi355x.h -- C ABI of the MI355X-native fastMNN / reducedMNN hot path (libbatchelor_mi355x.so).
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ / torch / R types.  Each entry point names the
 * reference interface it replaces (paths relative to the batchelor source tree).  Matrices crossing the boundary
 * use R's memory layout: column-major double, int32 indices, 1-based cell / batch ids unless stated otherwise.
 * All pointers are HOST pointers unless the name says `_dev`.  Calls return BMX_OK or a negative code; the message
 * (identical to the R / Rcpp error text where the reference has one) is read with bmx_last_error() so that the
 * R shim can hand it to Rf_error() verbatim (src/RcppExports.cpp:11,21 BEGIN_RCPP/END_RCPP).
 */
#ifndef BATCHELOR_MI355X_H
#define BATCHELOR_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BMX_OK 0
#define BMX_ERR_HIP (-1)        /* HIP runtime failure (no GPU, out of memory, launch error) */
#define BMX_ERR_DIM_GENES (-2)  /* "number of genes do not match up between matrices"  src/adjust_shift_variance.cpp:35 */
#define BMX_ERR_DIM_CELLS (-3)  /* "number of cells do not match up between matrices"  src/adjust_shift_variance.cpp:40 */
#define BMX_ERR_SUBSET (-4)     /* "subset indices out of range"                        src/utils.cpp:9 */
#define BMX_ERR_INDEX_LEN (-5)  /* "'index' must have length equal to number of rows in 'averaged'" src/smooth_gaussian_kernel.cpp:19 */
#define BMX_ERR_ARG (-6)        /* invalid argument (message says which) */
#define BMX_ERR_TREE (-7)       /* "invalid leaf nodes specified in 'merge.order'" R/MNN_tree.R:104 and friends */
#define BMX_ERR_NO_PAIRS (-8)   /* no MNN pairs in a merge (R raises an error there: R/fastMNN.R:588-589 on NaN) */
#define BMX_ERR_EXCHANGE (-9)   /* the multi-GPU exchange callback failed */

/* Message of the last failing call on this thread. */
const char* bmx_last_error(void);
/* Number of visible HIP devices (0 when there is no GPU); never throws. */
int32_t bmx_device_count(void);
/* Frees arrays returned through `int32_t**` / `double**` out-parameters. */
void bmx_free(void* p);
/* The one-shot entry points (bmx_fast_mnn, the single primitives) run on the calling thread's CURRENT HIP device; a host
 * without HIP bindings of its own picks it here (hipSetDevice). */
int32_t bmx_set_device(int32_t device);
/* Engines park their device blocks in a process-wide pool when they go (at most 16 GB / 256 blocks: a host that calls
 * fastMNN() again and again then pays its hipMallocs once); an allocation that fails inside the library empties the pool
 * by itself, other allocators of the process (torch, RCCL, the host's own hipMalloc) call this when they need the memory.
 * The (at most 8 per device) streams parked by engines that are gone are destroyed too. */
void bmx_trim_caches(void);

/* ------------------------------------------------------------------------------------------------------------------
 * Legacy .Call kernels (R_CallMethodDef table, src/RcppExports.cpp:48-58)
 * ---------------------------------------------------------------------------------------------------------------- */

/* Replaces _batchelor_find_mutual_nns (src/find_mutual_nns.cpp:8-41; R stub R/RcppExports.R:8-10).
 * left [nL x k2], right [nR x k1]: column-major, 1-based.  Pairs come out for left cell ascending and, within a
 * left cell, in the order of its row of `left`.  *out_left / *out_right are malloc'ed (bmx_free). */
int32_t bmx_find_mutual_nns(const int32_t* left, int32_t nL, int32_t k2, const int32_t* right, int32_t nR, int32_t k1,
                            int32_t** out_left, int32_t** out_right, int64_t* npairs);

/* Replaces _batchelor_smooth_gaussian_kernel (src/smooth_gaussian_kernel.cpp:11-118; caller R/mnnCorrect.R:458).
 * averaged [g x U], index [index_len] 0-based columns of mat, mat [gd x n], out [g x n] caller-allocated. */
int32_t bmx_smooth_gaussian_kernel(const double* averaged, int32_t g, int32_t U, const int32_t* index,
                                   int32_t index_len, const double* mat, int32_t gd, int32_t n, double sigma2,
                                   double* out);

/* Replaces _batchelor_adjust_shift_variance (src/adjust_shift_variance.cpp:30-164; caller R/mnnCorrect.R:477).
 * data1 [g1 x n1], data2 [g2 x n2], vect [vrow x vcol] (= n2 x g), restrict1/2 0-based, out [n2]. */
int32_t bmx_adjust_shift_variance(const double* data1, int32_t g1, int32_t n1, const double* data2, int32_t g2,
                                  int32_t n2, const double* vect, int32_t vrow, int32_t vcol, double sigma2,
                                  const int32_t* restrict1, int32_t nr1, const int32_t* restrict2, int32_t nr2,
                                  double* out);

/* The same native with strict mode.  Form 2 below (the tiled form, taken beyond 4e7 pairs) settles a cell one of three ways:
 * the histogram quantile (a well-conditioned cell: the reference's value to 1e-8), a re-run in the reference's own order of
 * operations (a cell flagged as ill-conditioned: bit-equal), or -- a flagged cell with more significant pairs than the re-run
 * holds -- the histogram quantile again, which may then land on ANOTHER quantile.  strict != 0: the call records the way of
 * every cell, and the cells of that third kind are recomputed in the reference's order of operations (the literal wide
 * form, form 3): every flagged cell then has the reference's bits, every other one stays within 1e-8.  The cost grows with
 * the number of such cells (sequential chains over all restricted cells, each), and the host waits once per call for that
 * number.  Where the call takes form 1 or 3 anyway strict changes nothing.  With strict == 0 and counts == NULL this IS
 * bmx_adjust_shift_variance.
 * counts (nullable): {cells the tiled form handled, re-run literally, flagged beyond the re-run, recomputed by the strict
 * pass}, from this call's own buffers; each -1 where the tiled form did not run or strict is off. */
int32_t bmx_adjust_shift_variance_ex(const double* data1, int32_t g1, int32_t n1, const double* data2, int32_t g2,
                                     int32_t n2, const double* vect, int32_t vrow, int32_t vcol, double sigma2,
                                     const int32_t* restrict1, int32_t nr1, const int32_t* restrict2, int32_t nr2,
                                     double* out, int32_t strict, int64_t* counts);

/* Which form of adjust_shift_variance a call of these sizes takes (a pure function of the sizes): 1 = the reference's order
 * of operations literally (bit-equal to the CPU restatement, every cell; up to 4e7 (cell, restricted cell) pairs), 2 =
 * 16-cell tiles on the FP64 matrix cores with a histogram quantile (beyond that: a cell whose quantile walk is decided on
 * the last bits may land on the neighbouring quantile), 3 = the literal wide form (bit-equal to form 1; taken instead of
 * form 2 above 256 genes, whatever the size, and at any size under the testing hook "asv_wide" -- this query knows no
 * gene count, so it reports 3 only under the hook).  The engine's var_adj merges go through the same switch. */
int32_t bmx_adjust_shift_variance_form(int32_t n2, int32_t nr1, int32_t nr2);

/* ------------------------------------------------------------------------------------------------------------------
 * Third-party contract on the path: BiocNeighbors::queryKNN / findMutualNN (re-export R/findMutualNN.R:1-3; call
 * sites R/MNN_tree.R:129, R/fastMNN.R:605), and queryKNN's sibling findKNN for what workflows do next with the corrected
 * coordinates.  Exact Euclidean search, ascending distance, ties by lowest index.
 * ---------------------------------------------------------------------------------------------------------------- */

/* queryKNN(X, query, k): X [nx x d], query [nq x d] column-major; index [nq x k] 1-based, distance [nq x k]
 * (either output may be NULL).  k is clamped to nx by the caller (safe.k, R/fastMNN.R:604). */
int32_t bmx_query_knn(const double* X, int32_t nx, const double* query, int32_t nq, int32_t d, int32_t k,
                      int32_t* index, double* distance);

/* findKNN(X, k, subset): for each row of X (or each row named in `subset`, 1-based, any order, repeats allowed; NULL = all)
 * its k nearest OTHER rows of X: index 1-based [nq x k] column-major, distance Euclidean, ascending, ties to the lower
 * row; the row itself is never in its own list, rows that coincide with it are.  0 <= k <= n - 1.  X as in bmx_query_knn.
 * nq = n_subset with a subset (n_subset is ignored without one), else n; either output may be NULL; k = 0 or no query
 * row writes nothing.  X goes to the device once and is searched against itself at k + 1 by the search of bmx_query_knn;
 * on the device each list then loses the row's own entry, or its last entry where k + 1 lower-numbered copies of the row
 * fill the list.  Searching at k + 1 means that k = 36 on rows of at most 61 columns and k = 20 on longer rows leave the
 * candidate tiers' lists for the partitioned search: exact as everything here, slower. */
int32_t bmx_find_knn(const double* X, int32_t n, int32_t d, int32_t k, const int32_t* subset, int32_t n_subset,
                     int32_t* index, double* distance);

/* makeSNNGraph from an index: the shared-nearest-neighbour graph of index [n x k] (column-major, 1-based: each row's k nearest
 * OTHER rows, distinct, never the row itself -- what bmx_find_knn returns).  With L(c) = (c, index[c,1..k]) at ranks 0..k, cells
 * a > b share an edge exactly when L(a) and L(b) have a cell in common (S = their common cells).  type 0 "rank": weight
 * max(k - r / 2, 1e-6), r = the smallest rank_a(s) + rank_b(s) over S; 1 "number": |S|; 2 "jaccard": |S| / (2 (k + 1) - |S|).
 * *first > *second (1-based), ascending first then second, *weight, *m edges; the arrays are malloc'ed (bmx_free).  The same
 * input gives the same bytes.  1 <= k <= min(n - 1, 128), n * k < 2^31; n = 0 or 1: no edge (k is not looked at).  BMX_ERR_ARG
 * with a message for those, for an entry outside 1..n, a row that lists itself and a row that lists a row twice (found on
 * the device). */
int32_t bmx_snn_graph(const int32_t* index, int32_t n, int32_t k, int32_t type, int32_t** first, int32_t** second,
                      double** weight, int64_t* m);
/* makeSNNGraph(X, k): X as in bmx_find_knn goes to the device once, bmx_find_knn's search finds every row's k nearest other
 * rows, and the graph of bmx_snn_graph is built from the lists where they lie in device memory. */
int32_t bmx_make_snn_graph(const double* X, int32_t n, int32_t d, int32_t k, int32_t type, int32_t** first, int32_t** second,
                           double** weight, int64_t* m);

/* findMutualNN(data1, data2, k1, k2) -> first / second, 1-based, malloc'ed (bmx_free). */
int32_t bmx_find_mutual_nn(const double* data1, int32_t n1, const double* data2, int32_t n2, int32_t d, int32_t k1,
                           int32_t k2, int32_t** first, int32_t** second, int64_t* npairs);

/* Diagnostics of the last kNN call on this thread: queries that needed the exact FP64 re-scan. */
int64_t bmx_last_knn_exact_fallbacks(void);
/* Testing hook: non-zero routes every kNN query through the exact FP64 re-scan. */
void bmx_set_force_exact_knn(int32_t on);
/* Testing hooks, process-wide, set by an explicit call only: NOTHING in the environment of the host process changes what
 * the library computes, which tier of the search or which form of adjust_shift_variance runs (the library reads two
 * environment variables: BMX_DEBUG=1 prints the shape decisions of every search to stderr, BMX_HOST_THREADS=n sizes the
 * pool of host threads behind the pinned staging ring).  Knobs: "knn_tier" (1 / 2: that candidate tier only, 3: the exact
 * FP64 scan only), "sample" (rows of a candidate pass's threshold sample, -1 = automatic), "split_c" / "force_c"
 * (reference ranges of the tail / of every query block), "no_margin" (fp16 tier: lists cut at their KS-th best only),
 * "asv_fast" (the tiled form of adjust_shift_variance at any size), "exchange_always" (a single rank goes through its
 * exchange transport too), "refine_wave" (the exact re-rank spends a whole wave on every query), "asv_cap" (tiled
 * adjust_shift_variance: addends a chain of the literal re-run of an ill-conditioned cell may keep; -1 = default, 0 = no
 * re-run), "asv_modes" (n: the tiled form records which way each of the first n cells of a call went, see
 * bmx_dev_get_bytes), "asv_sync" (0: the tiled form's workgroups do not wait for each other at the start of a round of
 * tiles -- the default; 1 = they do, measured slower), "sample_split" (ranges the threshold sample of a search with few
 * query blocks is split into; -1 = automatic, the default; 0 = never), "lk_seed" (searches with k beyond the tiers' lists: 1 = the
 * reference's partitions after the first are searched within the first's 36th distance, the default; 0 = all plainly), "tau_replay" (developer experiment: 1 = every search of
 * a run records its queries' final thresholds, 2 = the same sequence of searches starts its full passes from them),
 * "asv_strict" (-1 = every adjust_shift_variance call is strict where its caller says so, the default; 1 = every call is
 * strict: times strict mode on a workload whose driver has no switch for it), "mfma_shape" (fp16 tier: the MFMA shape of the
 * candidate sweep, 0 = 32x32x16, 1 = 16x16x32 where the row width has it; -1 = the library's table, the default),
 * "ref_order" (fp16 tier: the reference image of a search in ascending order of the rows' squared distance from the centre of
 * the queries, so that the rows nearest the queries are swept first; -1 = where the search has a threshold sample, the default;
 * 0 = never; 1 = wherever the tier runs; results do not depend on it),
 * "snn_lds_candidates" (SNN graph: candidates of a cell that one LDS window holds; 0 = 2048, the default; at least k + 1 and at
 * most 4096 are used; cells with more take several windows and give the same edges),
 * "reset" (all back to their defaults).
 * Unknown name: BMX_ERR_ARG. */
int32_t bmx_dev_set(const char* name, int32_t value);
/* Counters for tests and bench.py, current device: "asv_tiled_cells" (cells the tiled form of adjust_shift_variance has
 * handled), "asv_literal_cells" (of those, re-run in the reference's order of operations: bit-equal to the exact form),
 * "asv_fallback_cells" (ill-conditioned cells with too many significant pairs for the re-run: histogram quantile, may pick a
 * neighbouring quantile), "asv_tally_reset" (zeroes them and the ticks); 100 MHz device ticks of the tiled form added up over its
 * workgroups: "asv_ticks_stream", "asv_ticks_wait", "asv_ticks_cells" (the stream, the testing hook's round barrier, the per-cell
 * phase), "asv_ticks_literal" / "asv_ticks_chains" (the re-run cells' selection + re-evaluation + sort, their chains and walks),
 * "asv_literal_addends" (addends the re-run cells kept), "asv_chain_tiles" (tiles with a re-run cell).  Waits for the device.
 * Constants, no device needed: "delta_gene_tile" / "delta_pair_chunk" (genes a workgroup of bmx_delta_run's pair passes
 * owns, pairs of a step it walks), "delta_sparse_gene_tile" (genes a workgroup of bmx_delta_sparse_run's owns), "genevar_chunk" / "genevar_gene_tile" (cells of a chunk of the gene-variance handles,
 * genes a workgroup of the sparse one owns), "cluster_sparse_gene_tile" (genes a workgroup of bmx_cluster_sparse_centroids
 * keeps in the LDS).  Of the searches of this thread's single-primitive entry points (bmx_query_knn, bmx_find_knn, bmx_find_mutual_nn ...),
 * added up since the thread's first: "knn_exact_fallbacks" (queries finished by the FP64 paths) and "knn_tier2_queries" (queries
 * the first candidate tier handed to the second) -- what bmx_engine_profile_detail reports of an engine; "knn_mfma_shape"
 * (the MFMA shape the last fp16 candidate pass of those searches ran with: 0 = 32x32x16, 1 = 16x16x32, -1 = none yet).
 * Of the whole process, engines and single primitives alike: "knn_ordered_searches" / "knn_unordered_searches" (candidate passes
 * that ran with the reference image in key order / without).
 * Of this thread's last bmx_snn_graph / bmx_make_snn_graph: "snn_spilled_cells" (cells whose candidates took more than one LDS
 * window), "snn_graph_us" (microseconds between HIP events around the graph's kernels, the search excluded). */
int32_t bmx_dev_get(const char* name, int64_t* value);
/* "asv_modes" (after bmx_dev_set "asv_modes" = n): which way each of the first n cells of the LAST tiled adjust_shift_variance
 * call went -- 0 the histogram quantile (a well-conditioned cell), 1 re-run in the reference's order of operations, 2
 * ill-conditioned with more significant pairs than the re-run holds; 255 beyond what was recorded. */
int32_t bmx_dev_get_bytes(const char* name, void* dst, int64_t n);
/* HIP-event milliseconds of the device kernels of this thread's last bmx_smooth_gaussian_kernel / bmx_adjust_shift_variance
 * call (the host transfers of the call excluded): what bench.py's roofline of the two legacy natives is taken over. */
double bmx_last_native_kernel_ms(void);
/* Testing hook, needs no GPU: dst[0, bytes) = src[0, bytes) by the pool of host threads that moves the boundary's
 * matrices between the caller's memory and the pinned staging buffers (csrc/host_xfer.hpp) -- lets a CPU test hammer that
 * pool from several threads at once. */
int32_t bmx_dev_host_copy(void* dst, const void* src, int64_t bytes);

/* ------------------------------------------------------------------------------------------------------------------
 * The merge engine: replaces .fast_mnn / .fast_mnn_core (R/fastMNN.R:398-562) and everything they call
 * (R/MNN_tree.R, R/utils_tricube.R, R/utils_reorder.R) with one device-resident run.  The natural cut is the call
 * `.fast_mnn(batches, k, prop.k, restrict, ndist, merge.order, auto.merge, min.batch.skip)` made from
 * R/fastMNN.R:356,380 and R/reducedMNN.R:83,89.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct bmx_engine bmx_engine_t;

typedef struct {
    int32_t struct_size;   /* sizeof(bmx_params_t) as the CALLER's header has it: the library reads that many bytes and
                              gives the fields a later header appends their defaults (var_adj = 0, sigma = 0.1), so a
                              caller built against any header that HAS this field keeps working (the layout before it
                              -- round 2's, without struct_size -- is not readable and is refused for k < 36; fields
                              are only ever appended from here on); smaller than the fields up to auto_merge, or
                              larger than the library's own struct with non-zero bytes beyond: BMX_ERR_ARG */
    int32_t k;             /* k = 20 */
    double prop_k;         /* NaN = NULL (R/MNN_tree.R:140-146) */
    double ndist;          /* ndist = 3 */
    double min_batch_skip; /* NaN = NA_real_: batch.size not computed, nothing skipped (R/fastMNN.R:484) */
    int32_t auto_merge;    /* non-zero: R/MNN_tree.R:154-226 instead of the predefined tree */
    int32_t var_adj;       /* non-zero: rescale every cell's correction vector as mnnCorrect(var.adj=TRUE) does --
                              pmax(adjust_shift_variance(left, right, correction, sigma), 1) * correction
                              (R/mnnCorrect.R:331-342,462-481).  fastMNN() has no such switch: 0 is its behaviour */
    double sigma;          /* bandwidth handed to adjust_shift_variance as `sigma2` (R/mnnCorrect.R:477), 0.1 */
    int32_t var_adj_strict; /* non-zero (needs var_adj, else BMX_ERR_ARG): every adjust_shift_variance call of the run in
                              strict mode (bmx_adjust_shift_variance_ex); 0 for a caller whose header ends at sigma */
} bmx_params_t;

/* Multi-GPU exchange: called by the engine when `buf` (a DEVICE buffer of world * bytes_per_rank bytes whose slice
 * [rank * bytes_per_rank, +bytes_per_rank) this rank has filled) must become identical on all ranks (an in-place
 * all-gather; RCCL over xGMI in production).  The engine's stream is idle when it is called.  Return 0 on success. */
typedef int32_t (*bmx_allgather_fn)(void* ctx, void* buf, int64_t bytes_per_rank);

/* Creates an engine on HIP device `device` (its workspaces persist across runs). */
int32_t bmx_engine_create(int32_t device, bmx_engine_t** out);
void bmx_engine_destroy(bmx_engine_t* e);
/* Every kNN search is split by query rows over `world` ranks and completed with `fn`; all ranks hold all batches. */
int32_t bmx_engine_set_shard(bmx_engine_t* e, int32_t rank, int32_t world, bmx_allgather_fn fn, void* ctx);
/* Production exchange: RCCL called from inside the engine, in place on the engine's stream (no host round trip, no
 * staging copy).  bmx_rccl_load resolves the RCCL entry points from `librccl_path` (the RCCL the process already
 * uses -- one RCCL per process; NULL searches the global scope); rank 0 makes the 128-byte id with
 * bmx_rccl_unique_id and the host side hands it to every rank (MPI, torch.distributed, a file: not this library's
 * business); bmx_engine_init_rccl is collective over the ranks and replaces any callback set with set_shard. */
int32_t bmx_rccl_load(const char* librccl_path);
int32_t bmx_rccl_unique_id(void* id_out, int32_t bytes);
int32_t bmx_engine_init_rccl(bmx_engine_t* e, int32_t rank, int32_t world, const void* unique_id, int32_t bytes);
/* All-gathers issued and bytes received by this rank since the last bmx_engine_run started. */
int32_t bmx_engine_exchange_stats(bmx_engine_t* e, int64_t* calls, int64_t* bytes);
/* Copies the batches to HBM.  data[b]: nrows[b] x d column-major; restrict_idx[b]: 1-based, any order, a cell may be named
 * more than once (any R subsetting vector, R/checkInputs.R:96-120: the search then sees it as that many points), 
 * n_restrict[b] entries, or NULL / n_restrict[b] < 0 for "all cells". */
int32_t bmx_engine_upload(bmx_engine_t* e, int32_t nbatches, int32_t d, const double* const* data,
                          const int32_t* nrows, const int32_t* const* restrict_idx, const int32_t* n_restrict);
/* Runs all merges on the resident inputs (asynchronous launches; returns after the final stream synchronisation).
 * tree: the binary merge tree in post-order, leaf = 1-based batch id, 0 = "merge the two nodes on top of the stack,
 * deeper one is the left/reference child" -- e.g. list(list(1,2),3) is {1,2,0,3,0}.  Ignored when auto_merge. */
int32_t bmx_engine_run(bmx_engine_t* e, const bmx_params_t* params, const int32_t* tree, int32_t tree_len);
/* Results of the last run.  corrected: N x d column-major, rows in input batch order (R/fastMNN.R:541-547);
 * batch: N batch ids (1-based); merge_left / merge_right: (B-1) x B row-major, batch ids of each merge's left and
 * right sets padded with 0; batch_size, skipped: B-1; lost_var: (B-1) x B column-major.  Any pointer may be NULL. */
int32_t bmx_engine_download(bmx_engine_t* e, double* corrected, int32_t* batch, int32_t* merge_left,
                            int32_t* merge_right, double* batch_size, int32_t* skipped, double* lost_var);
/* MNN pairs of merge `merge` (0-based), 1-based OUTPUT-row indices (R/fastMNN.R:533-547); malloc'ed (bmx_free). */
int32_t bmx_engine_pairs(bmx_engine_t* e, int32_t merge, int32_t** left, int32_t** right, int64_t* npairs);
/* The same into arrays the caller owns (an R shim allocates its INTSXPs first and saves a copy): *npairs receives the
 * number of pairs; with left == right == NULL nothing else happens (size query), else capacity must be >= *npairs. */
int32_t bmx_engine_pairs_into(bmx_engine_t* e, int32_t merge, int32_t* left, int32_t* right, int64_t capacity,
                              int64_t* npairs);
/* Every merge's pairs in one call (what the shim does after a run: merge.info's `pairs` list, R/fastMNN.R:550-561):
 * left[m] / right[m] receive merge m's pairs, capacity[m] >= its pair count (bmx_engine_pairs_into's size query);
 * nmerges must be the number of merges of the last run.  One pass of the host threads over all lists instead of one
 * per list. */
int32_t bmx_engine_pairs_all_into(bmx_engine_t* e, int32_t nmerges, int32_t* const* left, int32_t* const* right,
                                  const int64_t* capacity);
/* Sizes of merge `merge`: out[0..5] = {cells searched on the left, on the right, MNN-involved right cells U,
 * pairs P, all left cells, all right cells} -- the inputs of the algorithmic flop / byte counts. */
int32_t bmx_engine_merge_stats(bmx_engine_t* e, int32_t merge, int64_t* out6);
/* Hang safety.  The candidate kernels synchronise their waves through LDS words in unbounded poll loops, so the HOST
 * never waits without a deadline: every wait of a run polls the engine's stream against base_ms plus a term scaled from
 * the work queued (about 1e4 times its expected duration).  When a deadline passes the call returns BMX_ERR_HIP with a
 * message starting "watchdog:", and the engine is dead: every later call on it fails at once and bmx_engine_destroy
 * abandons its stream and device memory instead of waiting for them -- only a fresh process gets the GPU back.
 * Default base 60 000 ms; base_ms <= 0 switches the watchdog off (plain hipStreamSynchronize). */
int32_t bmx_engine_set_watchdog(bmx_engine_t* e, double base_ms);
/* Testing hook of the watchdog: queues a kernel that keeps the engine's stream busy for `ms` milliseconds and then ends
 * by itself (the GPU stays healthy). */
int32_t bmx_engine_debug_stall(bmx_engine_t* e, int32_t ms);
/* With profiling on, every launch of a candidate-pass kernel (knn_topk_f16 / knn_topk_bf16, bmx_engine_knn_kernel names
 * the last one) is bracketed by HIP events on the engine's stream; after a run: total milliseconds, number of launches, and queries that needed the exact re-scan. */
int32_t bmx_engine_set_profiling(bmx_engine_t* e, int32_t on);
int32_t bmx_engine_profile(bmx_engine_t* e, double* topk_ms, int64_t* topk_launches, int64_t* exact_fallbacks);
/* Diagnostics for full-size parity checks: the next runs keep a device copy of the two matrices that merge `merge`
 * (0-based; -1 = off) hands to findMutualNN -- the left and right node after orthogonalisation
 * (R/fastMNN.R:473-477).  bmx_engine_snapshot copies them out ROW-major ([n x d], cells in node order); pass NULL
 * matrices to read the sizes first. */
int32_t bmx_engine_set_snapshot(bmx_engine_t* e, int32_t merge);
int32_t bmx_engine_snapshot(bmx_engine_t* e, double* left_rm, double* right_rm, int64_t* n_left, int64_t* n_right);
/* With params.var_adj, the snapshot merge also keeps what its adjust_shift_variance call (R/mnnCorrect.R:462-481) was handed
 * and what it returned: the centred left and right nodes and the right cells' correction vectors (ROW-major [n x d]), the
 * scalings [n_right] before pmax(., 1), the two restrict vectors (0-based rows of the nodes).  sizes4 = {n_left, n_right,
 * length(restrict1), length(restrict2)}; NULL pointers are skipped.  Lets a test hold one merge of a large tree against
 * src/adjust_shift_variance.cpp on the same inputs, a sample of cells at a time. */
int32_t bmx_engine_snapshot_var_adj(bmx_engine_t* e, double* left_rm, double* right_rm, double* corr_rm, double* scaling,
                                    int32_t* restrict1, int32_t* restrict2, int64_t* sizes4);
/* Testing hooks of var_adj runs made with bmx_dev_set("asv_modes", n > 0) (they wait for the device after every merge):
 * out3 = cells merge `merge`'s tiled adjust_shift_variance call re-ran in the reference's order of operations / flagged as
 * ill-conditioned but beyond the re-run / handled in all (-1: not recorded, e.g. the exact form ran); and the way every right
 * cell of the SNAPSHOT merge went (dst[0, n): 0 histogram quantile, 1 re-run, 2 flagged beyond it; 255 not recorded). */
int32_t bmx_engine_var_adj_tally(bmx_engine_t* e, int32_t merge, int64_t* out3);
int32_t bmx_engine_snapshot_var_adj_modes(bmx_engine_t* e, uint8_t* dst, int64_t n);
/* params.var_adj_strict: cells merge `merge`'s strict pass recomputed on this rank, from the call's own buffers (no testing
 * hook needed); -1: strict was off or the call did not take the tiled form. */
int32_t bmx_engine_var_adj_strict_cells(bmx_engine_t* e, int32_t merge, int64_t* cells);
/* Per kernel class (profiling on, since the last run started): out[0], out[1] = milliseconds and launches of the fp16
 * full pass, out[2], out[3] of the split-bf16 full pass, out[4], out[5] of the sample passes, out[6] = milliseconds of
 * the merges' streaming sections (everything that is not a kNN search), out[7] = queries that took the exact FP64
 * path, out[8] = queries the first tier handed to the second, out[9] = runs of this engine that were repeated with
 * host-checked searches (a run first leaves the counts of its uncertified queries on the device; when a search cannot be
 * completed that way -- hundreds of uncertified queries, lists overflowing with ties -- it starts over; the ranks of a
 * sharded run agree on that through a flag that travels with every search's lists, and start over together). */
int32_t bmx_engine_profile_detail(bmx_engine_t* e, double* out10);
/* The last profiled run's adjust_shift_variance calls (params.var_adj): out[0] = milliseconds (HIP events on the engine's
 * stream around each call), out[1] = calls, out[2] = (cell, restricted cell) pairs this rank evaluated. */
int32_t bmx_engine_profile_var_adj(bmx_engine_t* e, double* out3);
/* Measurement hook: ONE rank's share of an N-rank run on one GPU.  mode 1: the next run (a single rank) records what every
 * exchange of the run would have gathered; mode 2: the following runs are rank `rank` of `world` -- each search covers that
 * rank's slice of the query rows (bmx_shard_range), every replicated kernel runs in full, and an exchange fills the other
 * ranks' slices from the recording by a device copy (the collective itself is not timed: bmx_engine_exchange_stats gives its
 * calls and bytes); results are those of the recorded run; mode 0: back to normal.  Predefined merge trees only (auto-merge
 * deals whole searches over the ranks); the engine must have no transport (bmx_engine_init_rccl / _set_shard). */
int32_t bmx_engine_emulate(bmx_engine_t* e, int32_t mode, int32_t rank, int32_t world);
/* Name of the full-pass candidate kernel the engine launched last, as rocprofv3 prints it (template arguments
 * included): lets a benchmark check that a stored counter measurement belongs to the kernel it has just timed. */
int32_t bmx_engine_knn_kernel(bmx_engine_t* e, char* buf, int32_t n);
/* Candidate-pass kernel used by the engine's last MFMA-path search: 2 = knn_topk_bf16 (split-bf16 MFMA, LDS ring),
 * 3 = knn_topk_f16 (single fp16 product, LDS ring), -1 = none yet (bmx_dev_set "knn_tier" restricts the search to one
 * tier for A/B runs). */
int32_t bmx_engine_knn_variant(bmx_engine_t* e);

/* One-shot convenience (what the R shim calls): create + upload + run + download + pairs stay queryable on *out_engine
 * until bmx_engine_destroy. */
int32_t bmx_fast_mnn(int32_t nbatches, int32_t d, const double* const* data, const int32_t* nrows,
                     const int32_t* const* restrict_idx, const int32_t* n_restrict, const bmx_params_t* params,
                     const int32_t* tree, int32_t tree_len, double* corrected, int32_t* batch, int32_t* merge_left,
                     int32_t* merge_right, double* batch_size, int32_t* skipped, double* lost_var,
                     bmx_engine_t** out_engine);

/* ------------------------------------------------------------------------------------------------------------------
 * mnnCorrect() in gene space (R/mnnCorrect.R:125-393): the classic method end to end on the device, in place of the R
 * shim's .mnn_correct.  Batches are R matrices: genes x cells, column-major; restrict and subset.row are 1-based.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t struct_size;      /* sizeof(bmx_mnn_params_t) as the caller's header has it (fields are only ever appended) */
    int32_t k;                /* k = 20 */
    double prop_k;            /* NaN = NULL */
    double sigma;             /* sigma = 0.1 (handed to smooth_gaussian_kernel and adjust_shift_variance as is) */
    int32_t cos_norm_in;      /* cos.norm.in = TRUE */
    int32_t cos_norm_out;     /* cos.norm.out = TRUE */
    int32_t var_adj;          /* var.adj = TRUE */
    int32_t correct_all;      /* correct.all = FALSE */
    int32_t svd_dim;          /* must be 0: svd.dim > 0 is refused (BMX_ERR_ARG) */
    int32_t auto_merge;       /* must be 0: auto.merge = TRUE is refused (BMX_ERR_ARG) */
    const int32_t* subset_row;  /* 1-based genes, or NULL */
    int32_t n_subset_row;
    const int32_t* tree;      /* the binarised merge tree in post-order: leaf = batch id, 0 = merge (as bmx_fast_mnn) */
    int32_t tree_len;
    int32_t reserved;         /* the four bytes that were padding behind tree_len in the header before var_adj_strict: never
                                 read, whatever they hold (a caller built against that header leaves them unspecified) */
    int32_t var_adj_strict;   /* non-zero (needs var_adj, else BMX_ERR_ARG): both adjust_shift_variance calls of every merge
                                 in strict mode (bmx_adjust_shift_variance_ex).  Behind the earlier header's 80 bytes, so it
                                 is read only where struct_size covers it: a caller with that header gets 0 */
} bmx_mnn_params_t;
typedef struct bmx_mnn_result bmx_mnn_result_t;
/* Runs mnnCorrect on the calling thread's current device; every argument is checked before any device work.  *out holds
 * the result until bmx_mnn_result_free. */
int32_t bmx_mnn_correct(int32_t nbatches, int32_t n_genes, const double* const* data, const int32_t* ncells,
                        const int32_t* const* restrict_idx, const int32_t* n_restrict, const bmx_mnn_params_t* params,
                        bmx_mnn_result_t** out);
/* The same for batches given as CSC (genes x cells, a column per cell): indptr[b] is [ncells[b] + 1], from 0 to the
 * batch's number of stored entries and never decreasing; indices[b] the 0-based rows, strictly ascending within a column;
 * data[b] the stored values (indices[b] and data[b] may be NULL only where the batch has no stored entry).  indptr is
 * checked before any device work; a row outside [0, n_genes) or rows that do not ascend are seen on the device, where
 * such an entry is left out, and end the call with BMX_ERR_ARG.  A batch's CSC goes up whole and is expanded there into
 * the rows the correction needs: with subset.row and without correct.all no all-genes matrix exists on either side.
 * The result is bmx_mnn_correct's over the same matrices, bit for bit; a stored value v counts as 0.0 + v, so a stored
 * -0.0 is the +0.0 it becomes when a sparse matrix is made dense by adding its entries into zeros. */
int32_t bmx_mnn_correct_sparse(int32_t nbatches, int32_t n_genes, const int64_t* const* indptr,
                               const int32_t* const* indices, const double* const* data, const int32_t* ncells,
                               const int32_t* const* restrict_idx, const int32_t* n_restrict,
                               const bmx_mnn_params_t* params, bmx_mnn_result_t** out);
/* Sizes: genes of the corrected matrix (all genes with correct.all and a subset, else the subset's), cells, and the
 * pairs of every merge (npairs [nbatches - 1], NULL to skip). */
int32_t bmx_mnn_result_sizes(const bmx_mnn_result_t* r, int32_t* n_genes_out, int64_t* ncells, int64_t* npairs);
/* Caller-allocated: corrected [n_genes_out x ncells] column-major, cells in input order; batch [ncells] 1-based;
 * merge_left / merge_right [(nbatches - 1) x nbatches] row-major, batch ids zero-padded; pairs_left[m] / pairs_right[m]
 * npairs[m] 1-based columns of `corrected` each (any pointer may be NULL to skip that output). */
int32_t bmx_mnn_result_into(const bmx_mnn_result_t* r, double* corrected, int32_t* batch, int32_t* merge_left,
                            int32_t* merge_right, int32_t* const* pairs_left, int32_t* const* pairs_right);
/* Diagnostics: device time (HIP events, ms) over all merges of the stages search + pairs, averaging, smoothing,
 * adjust_shift_variance (both calls), apply. */
int32_t bmx_mnn_result_stage_ms(const bmx_mnn_result_t* r, double* out5);
/* params.var_adj_strict: out [(nbatches - 1) x 2] row-major, per merge the cells the strict pass recomputed in its
 * adjust_shift_variance call on the input genes and in the one on the output genes (-1: strict off, no such call, or the
 * call did not take the tiled form). */
int32_t bmx_mnn_result_strict_cells(const bmx_mnn_result_t* r, int64_t* out);
void bmx_mnn_result_free(bmx_mnn_result_t* r);

/* Row range [begin, end) of `n` query rows owned by `rank` of `world` (pure host arithmetic, no GPU). */
void bmx_shard_range(int64_t n, int32_t rank, int32_t world, int64_t* begin, int64_t* end);
/* Bytes each rank contributes to the in-place all-gather of a list with bytes_per_row bytes per query row (the slices
 * are padded to equal length: the gathered buffer holds world * this many bytes).  The engine sizes its exchanges with
 * the same function. */
int64_t bmx_shard_gather_bytes(int64_t n, int32_t world, int64_t bytes_per_row);

/* ------------------------------------------------------------------------------------------------------------------
 * Single primitives of the merge step, host in / host out, for parity tests that read like the reference's own
 * (tests/testthat/test-fast-mnn.R:7-92).  Same kernels as the engine.
 * ---------------------------------------------------------------------------------------------------------------- */
/* .center_along_batch_vector (R/fastMNN.R:626-640): mat [n x d] column-major in/out; restrict 1-based or NULL. */
int32_t bmx_center_along_batch_vector(double* mat, int32_t n, int32_t d, const double* batch_vec,
                                      const int32_t* restrict_idx, int32_t n_restrict);
/* .tricube_weighted_correction (R/fastMNN.R:599-608): curdata [n x d] in/out, correction [U x d], in_mnn [U] 1-based. */
int32_t bmx_tricube_weighted_correction(double* curdata, int32_t n, int32_t d, const double* correction,
                                        const int32_t* in_mnn, int32_t U, int32_t k, double ndist);
/* .average_correction (R/fastMNN.R:567-580) fed by findMutualNN on the same data: averaged [U x d] and second [U]
 * are malloc'ed; also returns the pairs. */
int32_t bmx_mnn_average_correction(const double* refdata, int32_t n1, const double* curdata, int32_t n2, int32_t d,
                                   int32_t k1, int32_t k2, int32_t** first, int32_t** second, int64_t* npairs,
                                   double** averaged, int32_t** second_u, int32_t* U);
/* .compute_perbatch_var (R/fastMNN.R:651-658) for one batch: sum over dims of the sample variance of data [n x d]. */
int32_t bmx_total_variance(const double* data, int32_t n, int32_t d, double* out);

/* ------------------------------------------------------------------------------------------------------------------
 * Directly upstream of the engine in fastMNN() (R/fastMNN.R:348-354).  x is genes x cells, column-major.
 * ---------------------------------------------------------------------------------------------------------------- */
/* cosineNorm(x, mode=) (R/cosineNorm.R:53-82): l2 [n] and / or the normalised matrix [G x n]; either may be NULL. */
int32_t bmx_cosine_norm(const double* x, int32_t G, int32_t n, double* l2, double* normalized);
/* One pass over x: cosine normalisation (if cos_norm != 0) fused with the PCA projection of R/multiBatchPCA.R:236-239,
 * out [n x d] = crossprod(cosineNorm(x) - centers, rotation); rotation [G x d] column-major, centers [G]. */
int32_t bmx_cosnorm_project(const double* x, int32_t G, int32_t n, const double* rotation, int32_t d,
                            const double* centers, int32_t cos_norm, double* out);

/* ------------------------------------------------------------------------------------------------------------------
 * multiBatchPCA on the device (R/multiBatchPCA.R:211-322; called from fastMNN() at R/fastMNN.R:353-354).  The batches
 * (genes x cells, column-major, as the reference has them) are uploaded once and stay in HBM; neither the scaled
 * genes x N matrix nor the genes x genes Gram matrix is formed: the top subspace is found by blocked subspace
 * iteration on the FP64 matrix cores with the centring and the cosine normalisation folded in.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct bmx_pca bmx_pca_t;
int32_t bmx_pca_create(int32_t device, int32_t n_genes, bmx_pca_t** out);
void bmx_pca_destroy(bmx_pca_t* p);
/* x: n_genes x n column-major (host).  weight: the batch's weight w_b (1 = R's default: every batch counts the same
 * whatever its size, R/multiBatchPCA.R:299-334).  cos_norm != 0: cosineNorm(x) (R/cosineNorm.R:63-82) on the fly. */
int32_t bmx_pca_add_batch(bmx_pca_t* p, const double* x, int64_t n, double weight, int32_t cos_norm);
/* The same batch handed over in column blocks, so that a 32 GB batch (200 000 cells x 20 000 genes, BASELINE.json
 * configs[3]) never has to exist in host memory at once: announce the batch, then its cells in order.  x_block is
 * n_genes x n_block column-major host memory, pageable or pinned; it has been read completely when the call returns
 * (it goes through a pinned double-buffered staging ring: host copy and DMA overlap). */
int32_t bmx_pca_begin_batch(bmx_pca_t* p, int64_t n, double weight, int32_t cos_norm);
int32_t bmx_pca_add_block(bmx_pca_t* p, const double* x_block, int64_t n_block);
/* multiBatchPCA's SVD (R/multiBatchPCA.R:386-393; the reference's irlba stops at tol = 1e-5) by Chebyshev-filtered
 * subspace iteration on a block of 64 vectors (d <= 56) or 128 (d <= 120): iterates until the Ritz residuals
 * max_j |M x_j - theta_j x_j| / theta_1 of the d wanted pairs are <= tol; at most max_iters applications of the operator
 * (one pass over every batch each), then BMX_ERR_ARG with the residual reached in the message.  iters_used / residual
 * (nullable) are written in both cases.  centers [n_genes], rotation [n_genes x d] column-major (columns defined up to
 * sign, as any SVD's), sdev [d] singular values of the scaled matrix; any may be NULL.  Needs n_genes and the total
 * number of cells above the block width.  A run that ends without reaching tol has written its results and leaves the
 * handle fitted; a fit that fails for any other reason leaves it unfitted (bmx_pca_project then refuses), whatever an
 * earlier fit had left. */
int32_t bmx_pca_fit_tol(bmx_pca_t* p, int32_t d, double tol, int32_t max_iters, double* centers, double* rotation,
                        double* sdev, int32_t* iters_used, double* residual);
/* Fixed-count form: exactly `iters` plain subspace iterations, no convergence test (kept for callers of round 2). */
int32_t bmx_pca_fit(bmx_pca_t* p, int32_t d, int32_t iters, double* centers, double* rotation, double* sdev);
/* crossprod(cosineNorm(x_b) - centers, rotation) (R/multiBatchPCA.R:236-239): out [n_b x d] column-major. */
int32_t bmx_pca_project(bmx_pca_t* p, int32_t batch, double* out);

/* multiBatchPCA(subset.row=, get.all.genes=TRUE, get.variance=TRUE) (R/multiBatchPCA.R:401-432).  The bmx_pca_t holds
 * the subset.row rows only (the caller gathers them; cos_norm then norms over exactly those rows, R/fastMNN.R:348-351) and
 * is fitted as above.  A bmx_pca_genes_t borrows the fitted handle and streams the n_genes_left rows OUTSIDE the subset
 * through the device once, in column blocks that are not kept (two in HBM at a time: the upload of a block overlaps the
 * kernels of the one before): per block the cells' projections are recomputed from the resident subset rows, and one
 * read of the block on the FP64 matrix cores accumulates  sum_b (w_b / n_b) sum_c scale_c x_gc pcs_b[c][j]  and the gene
 * sums.  bmx_pca_genes_finish then gives the leftover genes' grand centres (formed as the subset's) and rotation rows
 *     ( that sum  -  center[g] * sum_b (w_b / n_b) sum_c pcs_b[c][j] ) / sdev[j]^2
 * = left.scaled %*% v swept by d.  The fitted handle must outlive this one; after a bmx_pca_begin_batch / add_batch / fit
 * on it every call here is BMX_ERR_ARG.  No floating-point atomics: the same calls give the same bits.
 * n_genes_left may be 0 (bmx_pca_genes_total_variance alone). */
typedef struct bmx_pca_genes bmx_pca_genes_t;
int32_t bmx_pca_genes_create(int32_t n_genes_left, bmx_pca_t* fitted, bmx_pca_genes_t** out);
void bmx_pca_genes_destroy(bmx_pca_genes_t* h);
/* The leftover rows of batch `batch` (0-based) follow; batches come 0, 1, ... in the order they were added. */
int32_t bmx_pca_genes_begin_batch(bmx_pca_genes_t* h, int32_t batch);
/* The next n_block cells of that batch, in order: x_left_block is n_genes_left x n_block column-major host memory,
 * pageable or pinned, read completely when the call returns (the staging ring of bmx_pca_add_block). */
int32_t bmx_pca_genes_add_block(bmx_pca_genes_t* h, const double* x_left_block, int64_t n_block);
/* Once every batch has all its cells: centers_left [n_genes_left], rotation_left [n_genes_left x d] column-major; either
 * may be NULL. */
int32_t bmx_pca_genes_finish(bmx_pca_genes_t* h, double* centers_left, double* rotation_left);
/* *var_total = sum_b (w_b / n_b) |x_b diag(scale_b) - centers 1^T|_F^2 over the resident (subset) rows, summed in the
 * centred form in a fixed order; var.total of R/multiBatchPCA.R:428-431 is this over the number of batches. */
int32_t bmx_pca_genes_total_variance(bmx_pca_genes_t* h, double* var_total);

/* multiBatchPCA over batches kept in HBM as CSC -- per batch indptr [n + 1] (int64), 0-based int32 row indices and FP64
 * values, the rows of a column strictly ascending (explicit zeros are values like any other) -- as bmx_norm_sparse_t keeps
 * its counts.  Row layout: the handle holds all n_rows rows of every batch; the first n_rows_pca are the rows the PCA
 * runs on (x[subset.row] in the caller's order, duplicates included), the others are the genes outside the subset,
 * ascending (n_rows_pca == n_rows: no subset, or no get.all.genes).  Rows ascend within a column, so the PCA rows of a
 * cell are a prefix of its column; the cut is found once per column at upload, and cos_norm norms over that prefix only.
 * After a batch's last block the device builds a row-major companion (rows of cos-scaled values with their cells,
 * ascending) by a counting sort without atomics.  The operator  M Q = sum_b (w_b / n_b) C_b C_b^T Q  is two gathers on the
 * FP64 vector ALUs, 64 subspace columns at a time with a lane per column: by cell from the CSC (Z = C_b^T Q) and by gene
 * from the companion (rows cut into segments of bmx_dev_get "pca_sparse_row_segment" entries, a row's segments added in
 * ascending order by a second kernel).  The iteration around it -- Chebyshev filter, Cholesky QR 2, Rayleigh-Ritz,
 * residual, starting block -- is the one bmx_pca_t runs, on the dense n_rows_pca x 64 blocks.  No floating-point
 * atomics: the same calls give the same bits, however the batches were cut into blocks.
 * What only the device sees of the pattern is flagged at upload and reported by the fit: "a row index is outside [0,
 * number of genes)", "the row indices of a column should be strictly ascending".  Such entries are skipped by every
 * kernel, never used as an address.  A batch holds at most 2^31 - 1 cells and any number of stored entries. */
typedef struct bmx_pca_sparse bmx_pca_sparse_t;
int32_t bmx_pca_sparse_create(int32_t device, int32_t n_rows, int32_t n_rows_pca, bmx_pca_sparse_t** out);
void bmx_pca_sparse_destroy(bmx_pca_sparse_t* h);
/* The checks of a block on their own (no device), as bmx_norm_check_sparse_block: a block of n_block cells for a batch
 * of n cells of which `filled` have arrived; indptr [n_block + 1] relative to the block starts at 0, never decreases and
 * ends at nnz; indices and data [nnz] may be NULL only when nnz is 0. */
int32_t bmx_pca_sparse_check_block(int64_t n, int64_t filled, int64_t n_block, const int64_t* indptr,
                                   const int32_t* indices, const double* data, int64_t nnz);
/* A batch of n cells with nnz stored entries in all (reserved once); weight and cos_norm as for bmx_pca_add_batch.  Its
 * cells follow in one or more blocks, in order (host memory, read completely when the call returns). */
int32_t bmx_pca_sparse_begin_batch(bmx_pca_sparse_t* h, int64_t n, double weight, int32_t cos_norm, int64_t nnz);
int32_t bmx_pca_sparse_add_block(bmx_pca_sparse_t* h, int64_t n_block, const int64_t* indptr, const int32_t* indices,
                                 const double* data, int64_t nnz);
/* As bmx_pca_fit_tol / bmx_pca_fit over the first n_rows_pca rows: the same meaning, limits (d <= 120, a block of 64 or
 * 128 vectors, "rank below the subspace width"), messages and fitted state after a failure; centers [n_rows_pca],
 * rotation [n_rows_pca x d] column-major, sdev [d]. */
int32_t bmx_pca_sparse_fit_tol(bmx_pca_sparse_t* h, int32_t d, double tol, int32_t max_iters, double* centers,
                               double* rotation, double* sdev, int32_t* iters_used, double* residual);
int32_t bmx_pca_sparse_fit(bmx_pca_sparse_t* h, int32_t d, int32_t iters, double* centers, double* rotation,
                           double* sdev);
/* crossprod(cosineNorm(x_b) - centers, rotation) over the PCA rows: out [n_b x d] column-major. */
int32_t bmx_pca_sparse_project(bmx_pca_sparse_t* h, int32_t batch, double* out);
/* Once fitted, the rows outside the subset (resident: nothing is streamed): centers_left [n_rows - n_rows_pca] and
 * rotation_left [(n_rows - n_rows_pca) x d] column-major by the formula of bmx_pca_genes_finish; either may be NULL. */
int32_t bmx_pca_sparse_genes(bmx_pca_sparse_t* h, double* centers_left, double* rotation_left);
/* *var_total as bmx_pca_genes_total_variance, over the PCA rows, in the centred form per gene:
 * sum over the stored entries of (scale_c x_gc - center[g])^2  +  (n_b - stored entries of g) * center[g]^2. */
int32_t bmx_pca_sparse_total_variance(bmx_pca_sparse_t* h, double* var_total);

/* ------------------------------------------------------------------------------------------------------------------
 * clusterMNN() (R/clusterMNN.R:101-312): the two per-cell stages around the centroid-level merge.  The batches (genes x
 * cells, column-major) are uploaded once, whole or in column blocks through the pinned staging ring, and stay in HBM
 * between the centroid pass and the propagation; a batch that does not fit fails with the allocation error.  The
 * full-rank PCA of the centroids (.full_rank_pca, :171-181) and the merge itself (reducedMNN(k = 1): bmx_fast_mnn) stay
 * with the caller.  Every argument is checked before any device work.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct bmx_cluster bmx_cluster_t;
/* subset_row: 1-based genes (subset.row) the cosine norms and the projection are taken over (R/clusterMNN.R:140,274), or
 * NULL / 0 for all genes.  The centroids always cover all n_genes (correct.all needs them). */
int32_t bmx_cluster_create(int32_t device, int32_t n_genes, const int32_t* subset_row, int32_t n_subset_row,
                           bmx_cluster_t** out);
void bmx_cluster_destroy(bmx_cluster_t* h);
/* x: n_genes x n column-major (host).  clusters0 [n]: 0-based cluster id of every cell, below n_clusters.  restrict_idx:
 * 1-based cells, n_restrict of them (a cell named twice counts twice, as R's subsetting would), or NULL / n_restrict < 0
 * for "all cells".  cos_norm != 0: columns over pmax(1e-8, l2) (R/cosineNorm.R:63-82).  A cluster without a restricted
 * cell is BMX_ERR_ARG. */
int32_t bmx_cluster_add_batch(bmx_cluster_t* h, const double* x, int64_t n, const int32_t* clusters0, int32_t n_clusters,
                              const int32_t* restrict_idx, int64_t n_restrict, int32_t cos_norm);
/* The same batch in column blocks (as bmx_pca_begin_batch / bmx_pca_add_block): announce it, then its cells in order. */
int32_t bmx_cluster_begin_batch(bmx_cluster_t* h, int64_t n, const int32_t* clusters0, int32_t n_clusters,
                                const int32_t* restrict_idx, int64_t n_restrict, int32_t cos_norm);
int32_t bmx_cluster_add_block(bmx_cluster_t* h, const double* x_block, int64_t n_block);
/* .compute_centroids (R/clusterMNN.R:231-244) of batch `batch` (0-based): out [n_genes x n_clusters] column-major, the
 * mean of every cluster's restricted cells.  Bitwise the same from run to run (no floating-point atomics). */
int32_t bmx_cluster_centroids(bmx_cluster_t* h, int32_t batch, double* out);
/* .propagate_to_cells + .smooth_gaussian_from_centroids (R/clusterMNN.R:262-312) for one batch.  rotation [rows x d]
 * column-major and centers [rows], rows = n_subset_row (in subset_row's order) or n_genes; centroid_pcs / corrected_pcs
 * [n_clusters x d] column-major: the batch's centroids before and after the merge; 1 <= d <= 256.  out [n x d]
 * column-major; *sigma_out (nullable) = the median distance of the restricted cells to their nearest centroid, equal to
 * numpy.median of those distances bit for bit.  A sigma of 0 is not special-cased (NaN, as in the reference). */
int32_t bmx_cluster_propagate(bmx_cluster_t* h, int32_t batch, const double* rotation, int32_t d, const double* centers,
                              const double* centroid_pcs, const double* corrected_pcs, double* out, double* sigma_out);
/* Diagnostics, milliseconds since the handle was made: out[0] = upload (host wall time of the staged copies), then HIP-event
 * time of the centroid pass, the projection, nearest centroid + median, the smoothing. */
int32_t bmx_cluster_stage_ms(const bmx_cluster_t* h, double* out5);

/* The same over batches kept in HBM as CSC -- per batch indptr [n + 1] (int64), 0-based int32 row indices strictly
 * ascending within a column and FP64 values (explicit zeros are values like any other; implicit entries are zeros).  A
 * batch is announced with its cells and its stored entries and filled in column blocks (per block: indptr [n_block + 1]
 * relative to the block -- starts at 0, never decreases, ends at nnz; indices and data may be NULL only when nnz is 0;
 * host memory, read completely when the call returns).  Only the two streaming reads differ from bmx_cluster_t:
 *   - the centroid pass takes a chunk's cells in list order and adds every stored entry to its gene's accumulator, which
 *     a workgroup keeps in the LDS for bmx_dev_get "cluster_sparse_gene_tile" genes: the dense handle's sums with their
 *     terms of +0 left out, so without cos_norm the centroids equal the dense handle's bit for bit;
 *   - the projection gathers the rotation's rows of a cell's stored entries, one wave a cell, 64 columns at a time.
 * Under cos_norm a cell's l2 is taken over its stored entries in the subset_row rows, behind the block's upload.  The
 * reduction over chunks, the centring, the nearest centroid, the median and the smoothing are bmx_cluster_t's kernels,
 * and so are the arguments' meanings, limits and messages and the five stage times.  No floating-point atomics: the same
 * calls give the same bits, however the batch was cut into blocks.
 * What only the device sees of the pattern is flagged behind the upload, and bmx_cluster_sparse_centroids /
 * bmx_cluster_sparse_propagate refuse with BMX_ERR_ARG before they start: "a row index is outside [0, number of genes)",
 * "the row indices of a column should be strictly ascending".  Such entries are skipped by every kernel, never used as an
 * address.  A batch holds at most 2^31 - 1 cells and any number of stored entries. */
typedef struct bmx_cluster_sparse bmx_cluster_sparse_t;
/* subset_row / n_subset_row: as for bmx_cluster_create. */
int32_t bmx_cluster_sparse_create(int32_t device, int32_t n_genes, const int32_t* subset_row, int32_t n_subset_row,
                                  bmx_cluster_sparse_t** out);
void bmx_cluster_sparse_destroy(bmx_cluster_sparse_t* h);
/* A batch of n cells with nnz stored entries in all (reserved once); the other arguments as for bmx_cluster_begin_batch.
 * Its cells follow in one or more blocks, in order; a block's checks and norms run behind the upload of the next. */
int32_t bmx_cluster_sparse_begin_batch(bmx_cluster_sparse_t* h, int64_t n, int64_t nnz, const int32_t* clusters0,
                                       int32_t n_clusters, const int32_t* restrict_idx, int64_t n_restrict, int32_t cos_norm);
int32_t bmx_cluster_sparse_add_block(bmx_cluster_sparse_t* h, int64_t n_block, const int64_t* indptr, const int32_t* indices,
                                     const double* data, int64_t nnz);
/* As bmx_cluster_centroids: out [n_genes x n_clusters] column-major (dense). */
int32_t bmx_cluster_sparse_centroids(bmx_cluster_sparse_t* h, int32_t batch, double* out);
/* As bmx_cluster_propagate: out [n x d] column-major (dense). */
int32_t bmx_cluster_sparse_propagate(bmx_cluster_sparse_t* h, int32_t batch, const double* rotation, int32_t d,
                                     const double* centers, const double* centroid_pcs, const double* corrected_pcs,
                                     double* out, double* sigma_out);
/* As bmx_cluster_stage_ms; the upload includes the wait for the last block's checks and norms. */
int32_t bmx_cluster_sparse_stage_ms(const bmx_cluster_sparse_t* h, double* out5);

/* ------------------------------------------------------------------------------------------------------------------
 * kmeans(): R's kmeans(x, centers = <matrix>, algorithm = "Lloyd") (what bluster::KmeansParam stands for in
 * clusterMNN(clusters = <BlusterParam>), R/clusterMNN.R:199-221).  The observations (n x d, the d values of an observation
 * contiguous: d x n column-major) are uploaded once, whole or in blocks of observations through the pinned staging ring,
 * and stay in HBM for every run (start) and every iteration.  The assignment takes the products x . c on the FP64 matrix
 * cores and compares |c|^2 - 2 x.c, the lowest index winning on equal values; the centre update adds every cluster's
 * members in ascending order without floating-point atomics: the same calls give the same bits.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct bmx_kmeans bmx_kmeans_t;
#define BMX_KMEANS_MAX_CENTERS 1024
int32_t bmx_kmeans_create(int32_t device, int32_t n_dims, bmx_kmeans_t** out);
void bmx_kmeans_destroy(bmx_kmeans_t* h);
/* Announce the n >= 1 observations (once per handle), then hand them over in order: x_block [n_block][n_dims]. */
int32_t bmx_kmeans_begin(bmx_kmeans_t* h, int64_t n);
int32_t bmx_kmeans_add_block(bmx_kmeans_t* h, const double* x_block, int64_t n_block);
/* Lloyd from centers [n_centers][n_dims] (every centre contiguous), 1 <= n_centers <= min(n, 1024), iter_max >= 1.  Labels
 * start as "none"; every iteration assigns each observation to its nearest centre; no label changed: the run ends with
 * *converged_out = 1; otherwise every centre becomes the mean of its members, *iter_out counts the assignments, and after
 * iter_max of them the run ends behind the update with *converged_out = 0.  cluster_out [n]: 1-based labels; centers_out
 * [n_centers][n_dims]: the means of those labels; size_out [n_centers]; withinss_out [n_centers] = sum (x - c)^2 taken
 * directly; *tot_withinss_out their sum in ascending order.  BMX_ERR_ARG: "initial centers are not distinct" (two equal
 * rows of `centers`), "empty cluster: try a better set of initial centers" (an update met a cluster without members; the
 * outputs are then undefined).  The handle stays usable after either. */
int32_t bmx_kmeans_run(bmx_kmeans_t* h, const double* centers, int32_t n_centers, int32_t iter_max, int32_t* cluster_out,
                       double* centers_out, int32_t* size_out, double* withinss_out, double* tot_withinss_out,
                       int32_t* iter_out, int32_t* converged_out);
/* Diagnostics, milliseconds since the handle was made: out[0] = upload (host wall time of the staged copies), then HIP-event
 * time of the assignments, the centre updates and withinss, out[4] = host wall time of the downloads. */
int32_t bmx_kmeans_stage_ms(const bmx_kmeans_t* h, double* out5);

/* ------------------------------------------------------------------------------------------------------------------
 * rescaleBatches() (R/rescaleBatches.R:103-150) and regressBatches() (R/regressBatches.R:93-158): the linear
 * corrections.  The batches (genes x cells, column-major) are uploaded once, whole or in column blocks through the
 * pinned staging ring, and stay in HBM between the per-gene statistics and the pass that writes the result; results
 * come back genes x cells, column-major, cells in input order.  subset.row is applied by the caller: it uploads the rows
 * it wants corrected, n_genes of them.  Per-gene sums are taken over fixed chunks of a batch's restricted cells in a
 * fixed order without floating-point atomics: the same input gives the same bits on every run and for every blocking of
 * the upload.  Every argument is checked before any device work.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct bmx_linear bmx_linear_t;
#define BMX_LINEAR_MAX_DESIGN_COLUMNS 64
int32_t bmx_linear_create(int32_t device, int32_t n_genes, bmx_linear_t** out);
void bmx_linear_destroy(bmx_linear_t* h);
/* Optional, before the first batch: what is going to be asked for, so that the per-gene sums of a column block run
 * behind the upload of the next block.  kind 0: nothing (the sums run inside bmx_linear_rescale / _regress); 1: plain sums
 * (bmx_linear_regress without a design); 2: sums of log_base^x - pseudo_count (bmx_linear_rescale with these values).
 * keep_unlogged != 0 (kind 2, batches without restriction): the unlogged values are kept in HBM and read by the second
 * pass instead of being recomputed.  The results do not depend on this call. */
int32_t bmx_linear_expect(bmx_linear_t* h, int32_t kind, double log_base, double pseudo_count, int32_t keep_unlogged);
/* A batch of n cells.  restrict_idx: 1-based cells the statistics are taken over, n_restrict of them (a cell named twice
 * counts twice, as R's subsetting would), or NULL / n_restrict < 0 for "all cells".  Its cells follow in one or more
 * blocks (x_block: n_genes x n_block column-major, host), in order. */
int32_t bmx_linear_begin_batch(bmx_linear_t* h, int64_t n, const int32_t* restrict_idx, int64_t n_restrict);
int32_t bmx_linear_add_block(bmx_linear_t* h, const double* x_block, int64_t n_block);
/* .rescale_batches (R/rescaleBatches.R:103-150).  outs[b]: n_genes x n_b column-major (caller-allocated), every cell of
 * batch b.  avg_out [n_genes x n_batches] column-major (the mean of log_base^x - pseudo_count over each batch's
 * restricted cells) and ref_out [n_genes] (their minimum over the batches) are nullable.  log(x, log_base) is log2 for 2,
 * log10 for 10 and log(x) / log(log_base) otherwise, as in R.  At least two batches. */
int32_t bmx_linear_rescale(bmx_linear_t* h, double log_base, double pseudo_count, double* const* outs, double* avg_out,
                           double* ref_out);
/* regressBatches(): residuals of a per-gene least-squares fit on the restricted cells, for every cell.
 * design == NULL: one indicator column per batch; outs[b] = x - (mean over batch b's restricted cells);
 * coef_out [n_genes x n_batches] (nullable) holds the means; p, w, keep are ignored (n_keep must be 0).
 * Otherwise design [N x p] column-major, N = all cells in upload order, 1 <= p <= 64, and w [R x p] column-major =
 * the transposed pseudo-inverse of design's restricted rows (R rows: the restricted cells batch by batch, ascending
 * within a batch), so that coef = X[, restricted] %*% w; the caller factors the design and refuses a rank-deficient
 * one.  keep: 1-based columns of the design that are NOT regressed out (n_keep of them, may be 0).
 * outs[b] = x - coef[, dropped] %*% t(design[cells of b, dropped]); coef_out [n_genes x p] (nullable). */
int32_t bmx_linear_regress(bmx_linear_t* h, const double* design, int32_t p, const double* w, const int32_t* keep,
                           int32_t n_keep, double* const* outs, double* coef_out);
/* The checks of bmx_residual_pca_create / _fit's PCA arguments on their own (no device), as bmx_norm_check_*. */
int32_t bmx_linear_check_pca(int32_t n_genes, int32_t n_pca_rows, int32_t d, double tol, int32_t max_applies,
                             const double* weights, int32_t n_batches);
/* The batches as they were uploaded, back into outs[b] (n_genes x n_b) through the download ring with no kernel in
 * between: the least that moving a call's bytes in and out costs (scripts/linear_correct_probe.py measures against it). */
int32_t bmx_linear_fetch(bmx_linear_t* h, double* const* outs);
/* Diagnostics, milliseconds since the handle was made: out[0] = upload (host wall time of the staged copies), HIP-event
 * time of out[1] the first pass (chunk sums / the product with w), out[2] the statistics kernels, out[3] the second pass's
 * kernels; out[4] = host wall time of the second pass with its downloads. */
int32_t bmx_linear_stage_ms(const bmx_linear_t* h, double* out5);

/* ------------------------------------------------------------------------------------------------------------------
 * regressBatches(d=, deferred=TRUE) (R/regressBatches.R:148-155): the PCA of the residuals, which are never formed.
 * The handle borrows a bmx_linear_t whose batches have all arrived, as bmx_pca_genes_t borrows a fitted bmx_pca_t: the
 * PCA runs over the first n_pca_rows rows of its resident batches, which are the PCA's batches.  The bmx_linear_t must
 * outlive this handle; a batch begun on it since makes every later call here an error.
 * bmx_residual_pca_fit fits the coefficients exactly as bmx_linear_regress fits them (design, p, w, keep, n_keep and
 * coef_out as there; the same bits), then runs multiBatchPCA (R/multiBatchPCA.R:211-322) on the residuals: weights
 * [n_batches] (NULL: equal weights), the grand centre the weighted mean of every batch's mean residual over ALL its cells.
 * The residual of a batch is its data minus a term of rank <= 65, so the subspace iteration of bmx_pca_fit_tol applies
 * its two products to the resident data and corrects the two skinny results.  1 <= d <= 120; tol > 0: until the relative
 * Ritz residual is <= tol, at most max_applies applications of the operator (an error when they do not reach it, after
 * the results have been written); tol <= 0: exactly max_applies plain steps.  centers_out [n_pca_rows], rotation_out
 * [n_pca_rows x d] column-major, sdev_out [d], iters_used, residual_out: nullable.  bmx_linear_rescale / _regress on the
 * bmx_linear_t work as before, whether or not a PCA was fitted.  The same input gives the same bits on every run and for
 * every blocking of the upload (fixed-order sums, no floating-point atomics).
 * bmx_residual_pca_project: crossprod(residuals of batch `batch` (0-based) - centers, rotation) of the fit: out [n_b x d]
 * column-major.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct bmx_residual_pca bmx_residual_pca_t;
int32_t bmx_residual_pca_create(int32_t n_pca_rows, bmx_linear_t* loaded, bmx_residual_pca_t** out);
void bmx_residual_pca_destroy(bmx_residual_pca_t* h);
int32_t bmx_residual_pca_fit(bmx_residual_pca_t* h, const double* design, int32_t p, const double* w, const int32_t* keep,
                             int32_t n_keep, const double* weights, int32_t d, double tol, int32_t max_applies,
                             double* coef_out, double* centers_out, double* rotation_out, double* sdev_out,
                             int32_t* iters_used, double* residual_out);
int32_t bmx_residual_pca_project(bmx_residual_pca_t* h, int32_t batch, double* out);

/* ------------------------------------------------------------------------------------------------------------------
 * multiBatchNorm() (R/multiBatchNorm.R:100-280): size factors rescaled between batches, then log-normalized values.
 * The batches (genes x cells counts, FP64, column-major, finite and >= 0) are uploaded once, whole or in column blocks
 * through the pinned staging ring, and stay in HBM.  With S the statistic rows:
 *   size factors  sf = given / mean(given), or lib / mean(lib) with lib[c] = sum over S of x[g, c]; every one must be
 *                 finite and > 0 ("size factors should be positive")
 *   averages      ave[g] = (1 / n) * sum over c of x[g, c] / sf[c], g in S
 *   ratios        for every pair first < second, over the genes with
 *                 (ave_f / sum(ave_f) + ave_s / sum(ave_s)) / 2 * (sum(ave_f) + sum(ave_s)) / 2 >= min_mean:
 *                 ratios[first][second] = median(ave_s / ave_f), ratios[second][first] = median(ave_f / ave_s) (the middle
 *                 order statistic, or the mean of the two middle ones; 0 / x = 0 and x / 0 = inf are ordered with the
 *                 rest); no kept gene, a NaN ratio or a median that is 0 or not finite is an error ("median ratio of
 *                 averages between batches is not finite").  The diagonal is 1; the reference batch is the first column
 *                 whose minimum is the smallest; rescaling[b] = ratios[b][reference].
 *   values        log2(x / (sf / rescaling[b]) + pseudo_count), or x / (sf / rescaling[b]), for every uploaded row.
 * Library sizes and per-gene sums are taken in a fixed order over fixed chunks of cells without floating-point atomics:
 * the same input gives the same bits on every run and for every blocking of the upload.  Arguments are checked before
 * any device work; what only the data can show (a bad count, a cell without counts, a pair without a median) is raised
 * as device flags and reported by bmx_norm_run when its kernels have finished.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct bmx_norm bmx_norm_t;
/* stat_rows: 1-based rows of S in the order the averages are reported (a row named twice counts twice), n_stat of them;
 * NULL / n_stat < 0: all rows.  (A caller that wants values for the rows of S only uploads just those rows.) */
int32_t bmx_norm_create(int32_t device, int32_t n_genes, const int32_t* stat_rows, int64_t n_stat, bmx_norm_t** out);
void bmx_norm_destroy(bmx_norm_t* h);
/* The argument checks of bmx_norm_create / _begin_batch / _run on their own: they need no device. */
int32_t bmx_norm_check_create(int32_t n_genes, const int32_t* stat_rows, int64_t n_stat);
int32_t bmx_norm_check_batch(int64_t n, const double* size_factors);
int32_t bmx_norm_check_run(double min_mean, int32_t log, double pseudo_count);
/* A batch of n cells.  size_factors [n] (any scale, finite and > 0) or NULL for library sizes.  Its cells follow in one
 * or more blocks (x_block: n_genes x n_block column-major, host), in order; the library sizes and per-gene sums of a
 * block run behind the upload of the next. */
int32_t bmx_norm_begin_batch(bmx_norm_t* h, int64_t n, const double* size_factors);
int32_t bmx_norm_add_block(bmx_norm_t* h, const double* x_block, int64_t n_block);
/* outs[b]: n_genes x n_b column-major (caller-allocated).  Nullable: sf_out [cells of all batches, upload order] the
 * size factors the values were divided by (never re-centred); ave_out [n_stat x n_batches] column-major; ratios_out
 * [n_batches x n_batches] ROW-major (ratios_out[i * n_batches + j] = ratios[i][j]); smallest_out the 1-based reference
 * batch.  log: 1 for log2(. + pseudo_count), 0 for the normalized counts. */
int32_t bmx_norm_run(bmx_norm_t* h, double min_mean, int32_t log, double pseudo_count, double* const* outs, double* sf_out,
                     double* ave_out, double* ratios_out, int32_t* smallest_out);
/* Diagnostics, milliseconds since the handle was made: out[0] = upload (host wall time of the staged copies), HIP-event
 * time of out[1] the statistics passes (column sums, per-gene sums, size factors, averages), out[2] the ratio stage,
 * out[3] the output kernels; out[4] = host wall time of the output pass with its downloads. */
int32_t bmx_norm_stage_ms(const bmx_norm_t* h, double* out5);

/* Sparse counts: the same function over batches kept in HBM as CSC -- per batch indptr [n + 1] (int64), 0-based int32 row
 * indices and FP64 values, the rows of a column strictly ascending (no duplicates; explicit zeros are values like any
 * other).  A batch is announced with its cells and its stored entries and filled in column blocks.  Statistics, ratios
 * and flags are those of bmx_norm_t, and the per-gene sums take their terms in the same order with the zeros left out,
 * which changes no bit of a sum of non-negative terms: with the same size factors the results equal the dense handle's
 * bit for bit.  Values are written for the stored entries only; zero_out tells what every other entry would be.  What
 * only the device sees of the pattern is flagged like a bad count and reported by bmx_norm_sparse_run: "a row index is
 * outside [0, number of genes)", "the row indices of a column should be strictly ascending".  Such entries are skipped
 * by every kernel, never used as an address. */
typedef struct bmx_norm_sparse bmx_norm_sparse_t;
/* stat_rows / n_stat: as for bmx_norm_create. */
int32_t bmx_norm_sparse_create(int32_t device, int32_t n_genes, const int32_t* stat_rows, int64_t n_stat,
                               bmx_norm_sparse_t** out);
void bmx_norm_sparse_destroy(bmx_norm_sparse_t* h);
/* The checks of a block on their own (no device): a block of n_block cells for a batch of n cells of which `filled` have
 * arrived.  indptr [n_block + 1] is relative to the block: it starts at 0, never decreases and ends at nnz; indices and
 * data [nnz] may be NULL only when nnz is 0. */
int32_t bmx_norm_check_sparse_block(int64_t n, int64_t filled, int64_t n_block, const int64_t* indptr,
                                    const int32_t* indices, const double* data, int64_t nnz);
/* A batch of n cells with nnz stored entries in all (reserved once).  size_factors: as for bmx_norm_begin_batch.  Its cells
 * follow in one or more blocks, in order; a block's reductions run behind the upload of the next. */
int32_t bmx_norm_sparse_begin_batch(bmx_norm_sparse_t* h, int64_t n, const double* size_factors, int64_t nnz);
int32_t bmx_norm_sparse_add_block(bmx_norm_sparse_t* h, int64_t n_block, const int64_t* indptr, const int32_t* indices,
                                  const double* data, int64_t nnz);
/* outs[b]: [nnz_b] the values of batch b's stored entries in their order (may be NULL for a batch without entries).
 * zero_out (nullable): log2(pseudo_count) by the device's log2 -- what the dense handle writes for a zero -- or 0 without
 * the log.  The other arguments as for bmx_norm_run. */
int32_t bmx_norm_sparse_run(bmx_norm_sparse_t* h, double min_mean, int32_t log, double pseudo_count, double* const* outs,
                            double* sf_out, double* ave_out, double* ratios_out, int32_t* smallest_out, double* zero_out);
/* As bmx_norm_stage_ms. */
int32_t bmx_norm_sparse_stage_ms(const bmx_norm_sparse_t* h, double* out5);

/* ------------------------------------------------------------------------------------------------------------------
 * mnnDeltaVariance() (R/mnnDeltaVariance.R:95-201): per gene and merge step, the mean of the MNN-paired cells and the
 * variance of their deltas.  The batches (genes x cells, column-major) are uploaded once, whole or in column blocks
 * through the pinned staging ring, and stay in HBM; a batch that does not fit in free HBM fails with a message that
 * names subset_row (the caller uploads the rows it wants, n_genes of them; streaming by gene block is not offered).
 * The trend fit and the combination over steps stay with the caller.  Every sum has one fixed order and no
 * floating-point atomics are used: the same input gives the same bits on every run.  Every argument is checked before
 * any device work.  The kernels' gene-tile width and pair-chunk length are bmx_dev_get "delta_gene_tile" /
 * "delta_pair_chunk" (no device needed).
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct bmx_delta bmx_delta_t;
int32_t bmx_delta_create(int32_t device, int32_t n_genes, bmx_delta_t** out);
void bmx_delta_destroy(bmx_delta_t* h);
/* A batch of n cells; its cells follow in one or more blocks (x_block: n_genes x n_block column-major, host), in order. */
int32_t bmx_delta_begin_batch(bmx_delta_t* h, int64_t n);
int32_t bmx_delta_add_block(bmx_delta_t* h, const double* x_block, int64_t n_block);
/* One call for all merge steps.  cos_norm != 0 (:121-126): every cell of every batch is divided by
 * pmax(1e-8, l2 / ml2), l2 its norm over norm_genes0 (0-based genes, n_norm_genes of them; NULL / 0: all genes), ml2 the
 * mean over the batches of each batch's mean l2.  left[s] / right[s]: the npairs[s] pairs of step s as 1-based columns
 * of the batches side by side in upload order (what merge_info.pairs holds).  mean and total are [n_genes x nsteps]
 * column-major: mean = (rowMeans(left) + rowMeans(right)) / 2, total = the sample variance of left - right, taken as
 * rowVars takes it (the mean first, then the centred squares); NaN where a step has fewer than two pairs (mean: none). */
int32_t bmx_delta_run(bmx_delta_t* h, int32_t cos_norm, const int32_t* norm_genes0, int32_t n_norm_genes, int32_t nsteps,
                      const int32_t* const* left, const int32_t* const* right, const int64_t* npairs, double* mean,
                      double* total);
/* Diagnostics, milliseconds since the handle was made: out[0] = upload (host wall time of the staged copies), HIP-event
 * time of out[1] the cell norms, out[2] the two pair passes (the gather), out[3] the pair preparation and the reductions
 * over chunks; out[4] = host wall time of bmx_delta_run. */
int32_t bmx_delta_stage_ms(const bmx_delta_t* h, double* out5);

/* The same over batches kept in HBM as CSC, what R/mnnDeltaVariance.R:185-201 does over SVT_SparseMatrix blocks: per batch
 * indptr [n + 1] (int64), 0-based int32 row indices strictly ascending within a column and FP64 values (explicit zeros
 * are values like any other).  A batch is announced with its cells and its stored entries and filled in column blocks
 * (per block: indptr [n_block + 1] relative to the block -- starts at 0, never decreases, ends at nnz; indices and data
 * may be NULL only when nnz is 0).  Pairs, chunks, outputs and stage times are those of bmx_delta_t.  The sums of a chunk
 * take the stored entries in pair order -- the dense handle's sums with their terms of +0 left out -- so without
 * cos_norm `mean` equals the dense handle's bit for bit; a pair's two entries of a gene are combined before they are
 * squared, and the pairs of a chunk where neither cell stores the gene enter `total` as (pairs - touched) * m * m, m the
 * step's mean delta.  The same input gives the same bits on every run, for every block width, and for a step alone or
 * among others.  Every stored entry is checked on the device behind its upload, and bmx_delta_sparse_run refuses with
 * BMX_ERR_ARG before its pair passes start: "a row index is outside [0, number of genes)", "the row indices of a column
 * should be strictly ascending", "values should be finite".  The genes are tiled by bmx_dev_get "delta_sparse_gene_tile"
 * (no device needed).  A batch that does not fit in free HBM is refused as by bmx_delta_begin_batch. */
typedef struct bmx_delta_sparse bmx_delta_sparse_t;
int32_t bmx_delta_sparse_create(int32_t device, int32_t n_genes, bmx_delta_sparse_t** out);
void bmx_delta_sparse_destroy(bmx_delta_sparse_t* h);
int32_t bmx_delta_sparse_begin_batch(bmx_delta_sparse_t* h, int64_t n, int64_t nnz);
int32_t bmx_delta_sparse_add_block(bmx_delta_sparse_t* h, int64_t n_block, const int64_t* indptr, const int32_t* indices,
                                   const double* data, int64_t nnz);
int32_t bmx_delta_sparse_run(bmx_delta_sparse_t* h, int32_t cos_norm, const int32_t* norm_genes0, int32_t n_norm_genes,
                             int32_t nsteps, const int32_t* const* left, const int32_t* const* right, const int64_t* npairs,
                             double* mean, double* total);
int32_t bmx_delta_sparse_stage_ms(const bmx_delta_sparse_t* h, double* out5);

/* ------------------------------------------------------------------------------------------------------------------
 * Per-batch, per-gene mean and variance: what scran::modelGeneVar() takes from its input before any trend, and what
 * quickCorrect() (R/quickCorrect.R:66-120) ranks its genes by.  For every batch b and gene g over the batch's n_b cells:
 *   mean[g, b]  = (1 / n_b) * sum over c of x[g, c]
 *   total[g, b] = (1 / (n_b - 1)) * sum over c of (x[g, c] - mean[g, b])^2      (NaN for a batch of one cell)
 * Values are FP64, genes x cells column-major, and must be finite.  A batch STREAMS through two block buffers: it is
 * announced with its cells and sent in column blocks, each reduced behind the copy of the next, so a batch need not
 * fit in HBM.  The cells of a batch are cut into chunks of 256 at fixed positions WITHIN THE BATCH (bmx_dev_get
 * "genevar_chunk"); a block that does not end its batch must hold whole chunks.  Per chunk and gene the kernels take
 * the sum in cell order, the chunk mean, then the sum of squared deviations from it in cell order (two sweeps, never
 * E[x^2] - E[x]^2); the chunks are merged in ascending order by the pairwise update of Chan, Golub and LeVeque,
 *   delta = mB - mA;  n = nA + nB;  m = mA + (delta * nB) / n;  M2 = (M2A + M2B) + (((delta * delta) * nA) * nB) / n.
 * No floating-point atomics, contraction off: the results are the same bits on every run, for every block width, and
 * whichever batches were sent before.  Arguments are checked before any device work; what only the data can show is
 * raised as device flags and reported by bmx_genevar_run with BMX_ERR_ARG: "values should be finite".
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct bmx_genevar bmx_genevar_t;
int32_t bmx_genevar_create(int32_t device, int32_t n_genes, bmx_genevar_t** out);
void bmx_genevar_destroy(bmx_genevar_t* h);
/* The argument checks of bmx_genevar_create / _add_block / bmx_genevar_sparse_add_block on their own: they need no
 * device.  A block of n_block cells for a batch of n cells of which `filled` have arrived; for the sparse block see
 * bmx_genevar_sparse_add_block. */
int32_t bmx_genevar_check_create(int32_t n_genes);
int32_t bmx_genevar_check_block(int64_t n, int64_t filled, int64_t n_block);
int32_t bmx_genevar_check_sparse_block(int64_t n, int64_t filled, int64_t n_block, const int64_t* indptr,
                                       const int32_t* indices, const double* data, int64_t nnz);
/* A batch of n cells (1 <= n < 2^31).  Its cells follow in one or more blocks (x_block: n_genes x n_block column-major,
 * host, pageable is fine), in order; n_block is a multiple of 256 unless the block ends the batch. */
int32_t bmx_genevar_begin_batch(bmx_genevar_t* h, int64_t n);
int32_t bmx_genevar_add_block(bmx_genevar_t* h, const double* x_block, int64_t n_block);
/* mean_out, total_out: n_genes x n_batches column-major (caller-allocated), batches in upload order. */
int32_t bmx_genevar_run(bmx_genevar_t* h, double* mean_out, double* total_out);
/* Diagnostics, milliseconds since the handle was made: out[0] = upload (host wall time of the staged copies), out[1] =
 * HIP-event time of the kernels, out[2] = host wall time of bmx_genevar_run. */
int32_t bmx_genevar_stage_ms(const bmx_genevar_t* h, double* out3);

/* The same over batches given as canonical CSC: per block indptr [n_block + 1] (int64, relative to the block: starts at
 * 0, never decreases, ends at nnz), 0-based int32 row indices strictly ascending within a column and FP64 values
 * (explicit zeros are values like any other).  Only two blocks are on the device at a time.  A gene's sum takes the
 * stored entries in cell order -- the dense handle's sum with its terms of +0 left out, so `mean` equals the dense
 * handle's bit for bit but for the sign of a zero; the implicit zeros of a chunk enter M2 as (cells - stored) * m * m.
 * What only the device sees of the pattern is flagged and reported by bmx_genevar_sparse_run: "a row index is outside
 * [0, number of genes)", "the row indices of a column should be strictly ascending".  Such entries are skipped by every
 * kernel, never used as an address.  The genes are tiled by bmx_dev_get "genevar_gene_tile". */
typedef struct bmx_genevar_sparse bmx_genevar_sparse_t;
int32_t bmx_genevar_sparse_create(int32_t device, int32_t n_genes, bmx_genevar_sparse_t** out);
void bmx_genevar_sparse_destroy(bmx_genevar_sparse_t* h);
/* A batch of n cells with nnz stored entries in all; its blocks follow in order (n_block as for bmx_genevar_add_block;
 * indices and data may be NULL only when the block's nnz is 0). */
int32_t bmx_genevar_sparse_begin_batch(bmx_genevar_sparse_t* h, int64_t n, int64_t nnz);
int32_t bmx_genevar_sparse_add_block(bmx_genevar_sparse_t* h, int64_t n_block, const int64_t* indptr,
                                     const int32_t* indices, const double* data, int64_t nnz);
/* As bmx_genevar_run / bmx_genevar_stage_ms. */
int32_t bmx_genevar_sparse_run(bmx_genevar_sparse_t* h, double* mean_out, double* total_out);
int32_t bmx_genevar_sparse_stage_ms(const bmx_genevar_sparse_t* h, double* out3);

#ifdef __cplusplus
}
#endif
#endif /* BATCHELOR_MI355X_H */
