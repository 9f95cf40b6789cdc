"""Vertex-induced subgraphs and random walks on the device, and the subgraph mini-batches GCN layers train on (Cluster-GCN,
Chiang et al. 2019; GraphSAINT's random-walk sampler, Zeng et al. 2020; PyG's ``ClusterLoader`` /
``GraphSAINTRandomWalkSampler``).

    sub = gcn_amd.induced_subgraph(adj, nodes, values="gcn")       # Subgraph(adj, eid, node_ids)
    walks = gcn_amd.random_walk(adj, starts, length=4, seed=0, offset=0)
    for sub in gcn_amd.ClusterLoader(adj, parts, clusters_per_batch=8):
        logits = model(x[sub.node_ids], sub.adj)           # model: GraphConvolution layers, a GCN

A sampled ``Block`` (sampling.py) is bipartite and keeps the parent's values; a GCN layer needs a square, symmetric,
normalised adjacency over one vertex set, and that is the induced subgraph.  Both primitives are exact contracts written
out in include/gcn_spmm.h (``gcn_induced_subgraph_count_csr`` / ``_fill_csr``, ``gcn_random_walk_csr``) and run on
gcn_amd/csrc/subgraph.hip; tests/subgraph_ref.py is their numpy twin.  There is no CPU path: CPU tensors raise.
"""
from collections import namedtuple

import torch

from . import _lib
from ._lib import call
from .sampling import _check_stream, _vertex_map
from .spmm import CsrAdjacency

Subgraph = namedtuple("Subgraph", ["adj", "eid", "node_ids"])
Subgraph.__doc__ = """The subgraph a vertex set induces, a square graph over ``node_ids``.

adj: CsrAdjacency [len(node_ids) x len(node_ids)]; row i holds the entries of vertex node_ids[i] whose column is in the set,
in the parent's entry order, columns are positions in node_ids; symmetric iff the parent is; values as asked for
("parent": parent.val[eid]; "gcn": 1/sqrt(len_i * len_j) from the subgraph's own row lengths; "pattern": ones).
eid: int32, the parent's entry index of each entry.  node_ids: int64 vertex ids of the parent, in the caller's order."""

VALUES = ("parent", "gcn", "pattern")
assert _lib.SUBGRAPH_WS_BYTES <= _lib.SAMPLE_WS_BYTES      # (the adjacency's "sample" scratch serves both units)


def _check_ids(ids, name, what):
    if not isinstance(ids, torch.Tensor) or ids.dim() != 1 or ids.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: {name} must be a 1-D int32 or int64 tensor of vertex ids")
    if not ids.is_cuda:
        raise _lib.GcnAmdError(f"{what}: {name} must be a CUDA/HIP tensor (no CPU path in gcn_amd)")


def _check_square(adj, what):
    if not isinstance(adj, CsrAdjacency):
        raise TypeError(f"{what}: adj must be a CsrAdjacency")
    if adj.m != adj.n:
        raise ValueError(f"{what}: the adjacency must be square, not {adj.m}x{adj.n}")


def _check_count(v, name, what, least):
    if isinstance(v, bool) or not isinstance(v, int) or v < least:
        raise ValueError(f"{what}: {name} must be an int >= {least}, not {v!r}")


def _check_values(values, what):
    if values not in VALUES:
        raise ValueError(f"{what}: values must be one of {VALUES}, not {values!r}")


def random_walk(adj, starts, length, seed=0, offset=0):
    """``length`` steps of a uniform random walk from every vertex of ``starts``.

    adj: a square CsrAdjacency (its values are not used).  starts: 1-D int32 or int64 device tensor of vertex ids in
    [0, adj.m), repeats allowed.  length: an int >= 0.  seed, offset: the Philox key and stream position; walk i is a pure
    function of (i, starts[i], length, seed, offset) and does not depend on the other walks of the call.
    Returns an int32 tensor [len(starts), length + 1]: row i is walk i, column 0 its start.  It is the transposed view of
    the step-major buffer the kernel writes (the lanes of a wave store consecutive ints), so it is NON-CONTIGUOUS: call
    ``.contiguous()`` if a row-major copy is needed.  At a vertex without entries the walk stays where it is; each step
    picks an entry of the row uniformly (bias below d / 2^32), so a repeated entry is picked in proportion.
    One host synchronisation (the range of the starts): not capturable.  ``length == 0`` returns the starts.
    TypeError for a non-CsrAdjacency, ValueError for a non-square adjacency, a bad length, seed, offset, dtype or shape
    or a start out of range, GcnAmdError for CPU tensors."""
    _check_square(adj, "random_walk")
    _check_count(length, "length", "random_walk", 0)
    _check_stream(seed, offset, "random_walk")
    _check_ids(starts, "starts", "random_walk")
    dev = starts.device
    nw = int(starts.numel())
    out = torch.empty((length + 1, nw), dtype=torch.int32, device=dev)
    if nw == 0:
        return out.t()
    if adj.m == 0:
        raise ValueError("random_walk: the adjacency has no vertices, so every start is out of range")
    lo, hi = torch.stack([starts.min(), starts.max()]).tolist()          # the one synchronisation
    if lo < 0 or hi >= adj.m:
        raise ValueError(f"random_walk: starts must lie in [0, {adj.m}), found {lo if lo < 0 else hi}")
    if nw >= 2 ** 31:
        raise ValueError("random_walk: fewer than 2^31 walks per call (split the starts)")
    s32 = starts.to(torch.int32).contiguous()
    call("gcn_random_walk_csr", adj.rowptr, adj.col, adj.m, adj.nnz, s32, nw, int(length), int(seed), int(offset), out,
         device=dev)
    return out.t()


def induced_subgraph(adj, nodes, values="parent"):
    """The subgraph of ``adj`` induced by ``nodes``: ``A[nodes][:, nodes]`` in the parent's entry order.

    adj: a square CsrAdjacency.  nodes: DISTINCT vertex ids in [0, adj.m) in any order, a 1-D int32 or int64 device
    tensor; duplicates and ids out of range raise ValueError.  values: "parent" (``adj.val[eid]``), "gcn"
    (``1 / sqrt(len_i * len_j)`` from the subgraph's own row lengths: Cluster-GCN's renormalisation, the right Â when the
    parent's pattern carries its self-loops, as a normalised adjacency's does) or "pattern" (ones).
    Returns ``Subgraph(adj, eid, node_ids)``.  The subgraph is flagged symmetric iff the parent is (a principal submatrix
    of a symmetric matrix in one vertex order is symmetric: the backward pass needs no transpose build).
    Uses the n-entry int32 vertex map kept on ``adj`` (the one ``sample_blocks`` uses; allocated once, left cleared on
    every path), so the work of a call grows with the entries of the touched rows, not with n.  Two host synchronisations:
    the range of the nodes, and the total that sizes the outputs (the duplicate check rides on it).  Not capturable.
    TypeError for a non-CsrAdjacency, ValueError for a non-square adjacency, unknown ``values``, a bad dtype or shape,
    GcnAmdError for CPU tensors."""
    _check_square(adj, "induced_subgraph")
    _check_values(values, "induced_subgraph")
    _check_ids(nodes, "nodes", "induced_subgraph")
    dev = nodes.device
    nn = int(nodes.numel())
    ids = nodes.long()
    out_rowptr = torch.zeros(nn + 1, dtype=torch.int32, device=dev)
    if nn == 0:
        empty = torch.empty(0, dtype=torch.int32, device=dev)
        sub = CsrAdjacency(out_rowptr, empty, torch.empty(0, device=dev), (0, 0), symmetric=adj.symmetric)
        return Subgraph(sub, empty.clone(), ids)
    if adj.m == 0:
        raise ValueError("induced_subgraph: the adjacency has no vertices, so every node is out of range")
    lo, hi = torch.stack([ids.min(), ids.max()]).tolist()                # the first synchronisation
    if lo < 0 or hi >= adj.m:
        raise ValueError(f"induced_subgraph: nodes must lie in [0, {adj.m}), found {lo if lo < 0 else hi}")
    n32 = nodes.to(torch.int32).contiguous()
    vmap = _vertex_map(adj)
    ws = adj._scratch.get("sample", _lib.SAMPLE_WS_BYTES, adj.device)
    place = torch.arange(nn, dtype=torch.int32, device=dev)
    try:
        vmap[ids] = place
        repeated = (vmap[ids] != place).any()              # (a vertex named twice keeps one of its two positions)
        out_len = torch.zeros(nn, dtype=torch.int32, device=dev)
        call("gcn_induced_subgraph_count_csr", adj.rowptr, adj.col, adj.m, adj.nnz, n32, nn, vmap, out_len, ws, ws.numel(),
             device=dev)
        ends = torch.cumsum(out_len.long(), 0)
        dup, total = torch.stack([repeated.long(), ends[-1]]).tolist()   # the second synchronisation
        if dup:
            raise ValueError("induced_subgraph: nodes must be distinct")
        if total >= 2 ** 31:
            raise ValueError("induced_subgraph: the subgraph must have fewer than 2^31 entries (split the nodes)")
        out_rowptr[1:] = ends
        out_col = torch.empty(total, dtype=torch.int32, device=dev)
        out_eid = torch.empty(total, dtype=torch.int32, device=dev)
        if total > 0:                                      # (an empty tensor has no address, and the call refuses a null output)
            call("gcn_induced_subgraph_fill_csr", adj.rowptr, adj.col, adj.m, adj.nnz, n32, nn, vmap, out_rowptr, out_col,
                 out_eid, ws, ws.numel(), device=dev)
    finally:
        vmap[ids] = -1                                     # back to the cleared state (stream order: after the kernels)
    if values == "parent":
        val = adj.val[out_eid.long()]
    elif values == "pattern":
        val = torch.ones(total, dtype=torch.float32, device=dev)
    else:
        lens = out_len.double().clamp(min=1.0)              # (a column's own row is empty only in an asymmetric pattern)
        rows = torch.repeat_interleave(torch.arange(nn, device=dev), out_len.long(), output_size=total)
        val = (lens[rows] * lens[out_col.long()]).rsqrt().float()
    return Subgraph(CsrAdjacency(out_rowptr, out_col, val, (nn, nn), symmetric=adj.symmetric), out_eid, ids)


class ClusterLoader:
    """Cluster-GCN mini-batches: iterating yields the ``Subgraph`` induced by the vertices of ``clusters_per_batch``
    clusters, in ascending vertex id (``induced_subgraph(adj, ids, values)``).

    parts: one integer cluster id per vertex (a partition such as the communities of ``reorder.rabbit_device``); the ids
    need not be consecutive.  The vertices are grouped by cluster once, here (a stable sort by part and the clusters'
    pointers); a batch is a concatenation of slices and one sort.  Every epoch (every ``iter()``) draws a fresh permutation
    of the clusters from one CPU ``torch.Generator`` seeded with ``seed`` (``shuffle=False``: ascending cluster id) and
    covers every vertex exactly once; ``len()`` is the number of batches, and the last may hold fewer clusters."""

    def __init__(self, adj, parts, clusters_per_batch, shuffle=True, seed=0, values="gcn"):
        _check_square(adj, "ClusterLoader")
        _check_count(clusters_per_batch, "clusters_per_batch", "ClusterLoader", 1)
        _check_stream(seed, 0, "ClusterLoader")
        _check_values(values, "ClusterLoader")
        parts = torch.as_tensor(parts)
        if parts.dim() != 1 or parts.dtype not in (torch.int32, torch.int64) or parts.numel() != adj.m:
            raise ValueError(f"ClusterLoader: parts must be a 1-D int32 or int64 tensor with one cluster id per vertex ({adj.m})")
        self.adj, self.clusters_per_batch, self.shuffle, self.seed, self.values = adj, clusters_per_batch, bool(shuffle), seed, values
        parts = parts.to(torch.int64).cpu()
        order = torch.sort(parts, stable=True).indices     # vertices by cluster, ascending vertex id inside a cluster
        counts = torch.unique_consecutive(parts[order], return_counts=True)[1]
        self._ptr = [0] + torch.cumsum(counts, 0).tolist()
        self._order = order.to(adj.device)
        self.num_clusters = len(self._ptr) - 1
        self._gen = torch.Generator(device="cpu")
        self._gen.manual_seed(seed)

    def __len__(self):
        return (self.num_clusters + self.clusters_per_batch - 1) // self.clusters_per_batch

    def __iter__(self):
        c = self.num_clusters
        perm = torch.randperm(c, generator=self._gen).tolist() if self.shuffle else list(range(c))
        for lo in range(0, c, self.clusters_per_batch):
            chosen = perm[lo:lo + self.clusters_per_batch]
            ids = torch.cat([self._order[self._ptr[k]:self._ptr[k + 1]] for k in chosen]).sort().values
            yield induced_subgraph(self.adj, ids, self.values)


class RandomWalkLoader:
    """GraphSAINT's random-walk sampler: a batch draws ``num_roots`` roots from ``node_idx`` (uniformly, with replacement,
    from one CPU ``torch.Generator`` seeded with ``seed``), walks ``walk_length`` steps from each, and yields the
    ``Subgraph`` induced by the sorted distinct vertices of the walks.

    The Philox offset of the walks advances by one per batch and runs on from epoch to epoch, so no two batches share
    one; ``last_offset`` is the offset of the most recent batch.  ``len()`` is ``batches_per_epoch``.
    OUT OF SCOPE: GraphSAINT's loss and aggregator normalisation coefficients (estimated by pre-sampling) are not computed
    here; ``values="gcn"`` renormalises each subgraph by its own row lengths, as Cluster-GCN does."""

    def __init__(self, adj, node_idx, num_roots, walk_length, batches_per_epoch, seed=0, values="gcn"):
        _check_square(adj, "RandomWalkLoader")
        _check_count(num_roots, "num_roots", "RandomWalkLoader", 1)
        _check_count(walk_length, "walk_length", "RandomWalkLoader", 0)
        _check_count(batches_per_epoch, "batches_per_epoch", "RandomWalkLoader", 1)
        _check_stream(seed, 0, "RandomWalkLoader")
        _check_values(values, "RandomWalkLoader")
        node_idx = torch.as_tensor(node_idx)
        if node_idx.dim() != 1 or node_idx.dtype not in (torch.int32, torch.int64) or node_idx.numel() == 0:
            raise ValueError("RandomWalkLoader: node_idx must be a non-empty 1-D int32 or int64 tensor of vertex ids")
        self.adj, self.num_roots, self.walk_length, self.batches_per_epoch = adj, num_roots, walk_length, batches_per_epoch
        self.seed, self.values = seed, values
        self.node_idx = node_idx.to(device=adj.device, dtype=torch.int64)
        self._gen = torch.Generator(device="cpu")
        self._gen.manual_seed(seed)
        self._offset = 0
        self.last_offset = None

    def __len__(self):
        return self.batches_per_epoch

    def __iter__(self):
        n = int(self.node_idx.numel())
        for _ in range(self.batches_per_epoch):
            roots = self.node_idx[torch.randint(n, (self.num_roots,), generator=self._gen).to(self.node_idx.device)]
            self.last_offset = self._offset
            self._offset += 1
            walks = random_walk(self.adj, roots, self.walk_length, self.seed, self.last_offset)
            yield induced_subgraph(self.adj, torch.unique(walks), self.values)
