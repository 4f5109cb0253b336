"""dynaalign_amd -- MI355X-native all-pairs similarity hot path of DynaAlign.

Drop-in for the reference's ``similarityMH()`` / ``similarityNW()`` (reference
R/RcppExports.R:15-17, :34-36).  The compute lives in hand-written HIP kernels
for gfx950 behind a C ABI (include/dynaalign.h, libdynaalign_hip.so); this
package is the thin host side: argument marshalling (`similarity`), torch-tensor
plumbing for device-resident use (`device`), row-sharding over GPUs
(`sharding`) and synthetic inputs (`synth`).  There is no CPU implementation of
the hot path in the package: without the HIP library and a GPU every compute
call raises.
"""
from ._capi import DynaAlignError, load as load_library  # noqa: F401
from .clusterbreak import (  # noqa: F401
    clusterbreak, clusterconsensus, clusterconsensus_device, louvain, louvain_csr, louvain_device, louvain_sync_dense, netcluster,
    components, components_dense, components_device,
)
from .similarity import (  # noqa: F401
    SimilarityMatrix, get_option, hash_family_seeds, mh_counts, minhash_signatures, nw_pairs,
    pack_sequences, quantile_type7, set_option, similarityMH, similarityMH_cross, similarityMH_edges, similarityNW, similarityNW_cross, similarityNW_edges,
    nw_code_ranks, similarityMH_cross_topk, similarityNW_cross_topk, similarityMH_cross_edges, similarityNW_cross_edges,
    NWAlignment, nw_align, nw_align_long, nw_align_strings,
    nw_value_ranks, similarityNW_edges_long, similarityNW_cross_edges_long,
    SimilarityStats, compute_similarity_stats, stats_from_histogram, similarityMH_stats, similarityNW_stats, similarityNW_stats_long,
    similarityMH_knn, similarityNW_knn, knn_dense, knn_graph, similarityMH_knn_edges, similarityNW_knn_edges,
    similarityNW_knn_long, similarityNW_knn_edges_long, similarityNW_cross_topk_long,
    jaccard_dense, jaccard_counts, similarityJaccard, similarityJaccard_cross, similarityJaccard_cross_topk, similarityJaccard_knn,
    similarityJaccard_knn_edges, similarityJaccard_edges,
    similarityJaccard_long, similarityJaccard_cross_long, similarityJaccard_cross_topk_long, similarityJaccard_knn_long,
    similarityJaccard_knn_edges_long, similarityJaccard_edges_long, similarityJaccard_cross_edges_long, similarityJaccard_stats_long,
    lev_dense, lev_counts, similarityLev, similarityLev_cross, similarityLev_cross_topk, similarityLev_knn, similarityLev_knn_edges,
    similarityLev_edges, similarityLev_cross_edges,
    similarityMH_lsh_edges, lsh_edges_dense, lsh_collision_probability, similarityMH_lsh_knn, similarityMH_lsh_knn_edges, lsh_knn_dense,
    similarityMH_lsh_cross_edges, similarityMH_lsh_cross_topk, lsh_cross_edges_dense, lsh_cross_topk_dense,
    similarityMH_lsh_components, lsh_components_dense,
    similarityNW_lsh_edges, similarityNW_lsh_cross_edges, nw_lsh_edges_dense, nw_lsh_cross_edges_dense, nw_lsh_last_route,
    similarityNW_lsh_knn, similarityNW_lsh_knn_edges, similarityNW_lsh_cross_topk, nw_lsh_knn_dense, nw_lsh_cross_topk_dense,
)

__all__ = [
    "clusterbreak", "clusterconsensus", "clusterconsensus_device", "netcluster", "louvain", "louvain_csr", "louvain_sync_dense", "louvain_device", "nw_align", "nw_align_long", "nw_align_strings", "NWAlignment",
    "similarityMH", "similarityNW", "similarityMH_cross", "similarityNW_cross", "similarityMH_cross_topk", "similarityNW_cross_topk", "similarityMH_cross_edges", "similarityNW_cross_edges", "nw_code_ranks", "similarityMH_edges", "similarityNW_edges", "similarityNW_edges_long", "similarityNW_cross_edges_long", "nw_value_ranks", "quantile_type7", "minhash_signatures", "mh_counts", "nw_pairs", "hash_family_seeds",
    "SimilarityStats", "compute_similarity_stats", "stats_from_histogram", "similarityMH_stats", "similarityNW_stats", "similarityNW_stats_long",
    "similarityMH_knn", "similarityNW_knn", "knn_dense", "knn_graph", "similarityMH_knn_edges", "similarityNW_knn_edges",
    "similarityNW_knn_long", "similarityNW_knn_edges_long", "similarityNW_cross_topk_long",
    "jaccard_dense", "jaccard_counts", "similarityJaccard", "similarityJaccard_cross", "similarityJaccard_cross_topk", "similarityJaccard_knn",
    "similarityJaccard_knn_edges", "similarityJaccard_edges",
    "similarityJaccard_long", "similarityJaccard_cross_long", "similarityJaccard_cross_topk_long", "similarityJaccard_knn_long",
    "similarityJaccard_knn_edges_long", "similarityJaccard_edges_long", "similarityJaccard_cross_edges_long", "similarityJaccard_stats_long",
    "lev_dense", "lev_counts", "similarityLev", "similarityLev_cross", "similarityLev_cross_topk", "similarityLev_knn", "similarityLev_knn_edges",
    "similarityLev_edges", "similarityLev_cross_edges",
    "similarityMH_lsh_edges", "lsh_edges_dense", "lsh_collision_probability", "similarityMH_lsh_knn", "similarityMH_lsh_knn_edges", "lsh_knn_dense",
    "similarityMH_lsh_cross_edges", "similarityMH_lsh_cross_topk", "lsh_cross_edges_dense", "lsh_cross_topk_dense",
    "components", "components_dense", "components_device", "similarityMH_lsh_components", "lsh_components_dense",
    "similarityNW_lsh_edges", "similarityNW_lsh_cross_edges", "nw_lsh_edges_dense", "nw_lsh_cross_edges_dense", "nw_lsh_last_route",
    "similarityNW_lsh_knn", "similarityNW_lsh_knn_edges", "similarityNW_lsh_cross_topk", "nw_lsh_knn_dense", "nw_lsh_cross_topk_dense",
    "pack_sequences", "set_option", "get_option", "SimilarityMatrix", "DynaAlignError", "load_library",
]
