"""batchelor_amd: MI355X-native fastMNN / reducedMNN hot path behind batchelor's interface.

Host side mirrors the reference's R functions (same names, arguments, 1-based conventions and error text); the
arithmetic runs in hand-written HIP kernels for gfx950 behind the C ABI of include/batchelor_mi355x.h.
"""
from ._lib import BatchelorMI355XError, device_count  # noqa: F401
from .neighbors import SnnGraph, find_knn, make_snn_graph, neighbors_to_snn_graph, query_knn  # noqa: F401
from .reduced_mnn import MnnEngine, MnnResult, divideIntoBatches, reducedMNN  # noqa: F401
from .natives import (adjust_shift_variance, find_mutual_nn, find_mutual_nns, smooth_gaussian_kernel)  # noqa: F401
from .multi_batch_pca import (DevicePCA, DevicePCAGenes, DeviceSparsePCA, cosineNorm, multiBatchPCA,  # noqa: F401
                              multiBatchPCA_host, project, sparse_row_segment)
from .fast_mnn import fastMNN  # noqa: F401
from .mnn_correct import mnnCorrect  # noqa: F401
from .kmeans import KmeansParam, KmeansResult, kmeans  # noqa: F401
from .cluster_mnn import ClusterMnnResult, clusterMNN  # noqa: F401
from .linear_correct import LinearCorrectResult, regressBatches, rescaleBatches  # noqa: F401
from .delta_variance import MnnDeltaVarianceResult, mnnDeltaVariance  # noqa: F401
from .multi_batch_norm import MultiBatchNormResult, multiBatchNorm  # noqa: F401
from .model_gene_var import GeneVarTable, combineVar, getTopHVGs, modelGeneVar  # noqa: F401
from .batch_correct import (ClassicMnnParam, FastMnnParam, NoCorrectParam, NoCorrectResult, QuickCorrectResult,  # noqa: F401
                            RegressParam, RescaleParam, batchCorrect, intersectRows, noCorrect, quickCorrect)
