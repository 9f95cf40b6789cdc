"""gcn_amd — MI355X-native GCN aggregation (CSR SpMM) behind the pygcn op surface.

    import gcn_amd
    gcn_amd.install()                 # torch.spmm / torch.sparse.mm → HIP kernel (gcn1–5)
    adj = gcn_amd.CsrAdjacency.from_scipy(A_hat)   # explicit handle
    C = gcn_amd.spmm(adj, X)

Drop-in shared objects for gcn6.py live in gcn_amd/dropin/ (see INTEGRATION.md).
"""
from ._lib import GcnAmdError, LIB_PATH, DROPIN_DIR, load as load_library  # noqa: F401
from .spmm import CsrAdjacency, spmm, gather_rows, dropout_rows, install, uninstall  # noqa: F401
from .attention import edge_softmax, gat_edge_softmax, gatv2_scores, sddmm_heads, segment_sum, spmm_heads  # noqa: F401
from .aggregate import aggregate  # noqa: F401
from .edgefeat import edge_aggregate  # noqa: F401
from .sampling import Block, NeighborLoader, sample_blocks, sample_neighbors  # noqa: F401
from .subgraph import ClusterLoader, RandomWalkLoader, Subgraph, induced_subgraph, random_walk  # noqa: F401
from .construct import bucket_by_key, csr_from_edges, transpose_csr  # noqa: F401
from .coalesce import coalesce_csr, gcn_adjacency, normalize_csr, symmetrize  # noqa: F401
from .linkpred import LinkNeighborLoader, edge_subgraph, find_edges, negative_sample, pair_scores, reverse_entries, split_edges  # noqa: F401
from .spgemm import HypergraphLaplacian, SparseProduct, hypergraph_laplacian, sampled_dot, spgemm  # noqa: F401
from .knn import KNN_K_MAX, knn, knn_graph, knn_hypergraph  # noqa: F401
from . import reorder, dropin  # noqa: F401
from .layers import GCN, GINConv, GINEConv, HGNN, GraphAttention, GraphAttentionV2, GraphConvolution, GraphConvolution2, GraphSAGE, HGNNConv, SAGEConv  # noqa: F401

__version__ = "0.4.0"
