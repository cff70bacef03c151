// clusterMNN() on the device (cluster_mnn.hip): the batches stay resident between the centroid pass and the propagation
// of the centroids' corrections to the cells.  Host-side interface behind the bmx_cluster_* entry points.
#pragma once
#include <cstdint>

namespace bmx {

class Cluster;
// subset: 1-based genes (subset.row) the cosine norms and the projection are taken over, or null / nsubset = 0 for all
Cluster* cluster_create(int device, int G, const int32_t* subset, int nsubset);
void cluster_destroy(Cluster* c);
// argument checks of cluster_begin_batch, without a device (throws bmx::Error(BMX_ERR_ARG))
void cluster_check_batch(int64_t n, const int32_t* clusters0, int C, const int32_t* restrict_idx, int64_t n_restrict);
// a batch of n cells: clusters0 [n] 0-based cluster ids below C, restrict_idx 1-based cells (null / n_restrict < 0: all);
// its columns follow in one or more blocks, in order
void cluster_begin_batch(Cluster* c, int64_t n, const int32_t* clusters0, int C, const int32_t* restrict_idx,
                         int64_t n_restrict, int cos_norm);
void cluster_add_block(Cluster* c, const double* x_block_host, int64_t m);
// .compute_centroids (R/clusterMNN.R:231-244): out [G x C_b] column-major host memory
void cluster_centroids(Cluster* c, int batch, double* out);
// .propagate_to_cells for one batch (R/clusterMNN.R:262-282): rotation [rows x d] column-major and centers [rows] over the
// handle's genes (the subset's, in its order), centroid_pcs / corrected_pcs [C_b x d] column-major, out [n_b x d]
void cluster_propagate(Cluster* c, int batch, const double* rotation, int d, const double* centers,
                       const double* centroid_pcs, const double* corrected_pcs, double* out, double* sigma_out);
// milliseconds since the handle was made: upload (host wall time of the staged copies), then HIP-event time of the
// centroid pass, the projection, nearest centroid + median, the smoothing
void cluster_stage_ms(const Cluster* c, double* out5);

}  // namespace bmx
