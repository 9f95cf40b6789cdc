"""Neighbour sampling on the device and the mini-batch blocks GraphSAGE trains on (Hamilton et al. 2017; DGL's
``sample_neighbors`` / ``to_block``, PyG's ``NeighborLoader``).

    rowptr, col, eid = gcn_amd.sample_neighbors(adj, seeds, fanout=10, seed=0, offset=0)
    blocks, input_ids = gcn_amd.sample_blocks(adj, seeds, [25, 10])
    for blocks, input_ids, batch in gcn_amd.NeighborLoader(adj, train_idx, [25, 10], batch_size=1024):
        logits = model(x[input_ids], blocks)           # model = gcn_amd.GraphSAGE(...)

The sample is a pure function of (seed, offset, entry index) — the contract is written out in include/gcn_spmm.h at
``gcn_sample_neighbors_csr`` and runs on gcn_amd/csrc/sample.hip: a row of at most ``fanout`` entries is taken whole; of a
longer one the ``fanout`` entries with the smallest Philox4x32-10 keys are taken (ties: the lower entry index), and written
in the CSR's own entry order.  So the sample is uniform without replacement, reproducible bit for bit, and the neighbours
drawn for a vertex depend on (seed, offset) only — not on the batch it is in.  Two hops therefore use different offsets
(``sample_blocks`` gives hop l the offset ``offset + l``), and ``NeighborLoader`` advances the offset from batch to batch.

``sample_neighbors`` synchronises with the host once (it reads the output size and the range of the seeds), and
``sample_blocks`` again per hop for the size of the new frontier, so neither can be captured in a HIP graph.  There is no
CPU path: CPU tensors raise.
"""
from collections import namedtuple

import torch

from . import _lib
from ._lib import call
from .spmm import CsrAdjacency

Block = namedtuple("Block", ["adj", "eid", "src_ids", "num_dst"])
Block.__doc__ = """One hop of a sampled mini-batch, a bipartite graph from ``src_ids`` to its first ``num_dst`` vertices.

adj: CsrAdjacency [num_dst x len(src_ids)]; row i holds the sampled entries of vertex src_ids[i] in the parent's entry
order, columns are positions in src_ids, values are parent.val[eid].  eid: int32, the parent's entry index of each entry.
src_ids: int64 vertex ids of the parent; src_ids[:num_dst] are the rows' vertices."""


def _check_fanout(fanout, what):
    if isinstance(fanout, bool) or not isinstance(fanout, int) or (fanout < 1 and fanout != -1):
        raise ValueError(f"{what}: fanout must be an int >= 1, or -1 for every neighbour, not {fanout!r}")


def _check_seeds(seeds, what):
    if not isinstance(seeds, torch.Tensor) or seeds.dim() != 1 or seeds.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: seeds must be a 1-D int32 or int64 tensor of vertex ids")
    if not seeds.is_cuda:
        raise _lib.GcnAmdError(f"{what}: seeds must be a CUDA/HIP tensor (no CPU path in gcn_amd)")


def _check_stream(seed, offset, what):
    for name, v in (("seed", seed), ("offset", offset)):
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 2 ** 64:
            raise ValueError(f"{what}: {name} must be an int in [0, 2^64), not {v!r}")


def sample_neighbors(adj, seeds, fanout, seed=0, offset=0):
    """Up to ``fanout`` stored entries of every row ``seeds[i]`` of ``adj``, uniformly without replacement.

    adj: any CsrAdjacency (its values are not used).  seeds: 1-D int32 or int64 device tensor of row ids in [0, adj.m),
    in any order.  fanout: an int >= 1, or -1 for every entry.  seed, offset: the Philox key and stream position.
    Returns (rowptr [len(seeds) + 1], col, eid), int32 device tensors: row i holds the columns of the entries selected
    from row seeds[i] in the CSR's entry order (a column-sorted row stays sorted), and eid their entry indices into
    adj.col / adj.val.  One host synchronisation (the output size and the range of the seeds): not capturable.
    TypeError for a non-CsrAdjacency, ValueError for a bad fanout, seed dtype or shape or a seed out of range,
    GcnAmdError for CPU tensors."""
    if not isinstance(adj, CsrAdjacency):
        raise TypeError("sample_neighbors: adj must be a CsrAdjacency")
    _check_fanout(fanout, "sample_neighbors")
    _check_stream(seed, offset, "sample_neighbors")
    _check_seeds(seeds, "sample_neighbors")
    dev = seeds.device
    ns = int(seeds.numel())
    out_rowptr = torch.zeros(ns + 1, dtype=torch.int32, device=dev)
    empty = torch.empty(0, dtype=torch.int32, device=dev)
    if ns == 0:
        return out_rowptr, empty, empty.clone()
    if adj.m == 0:
        raise ValueError("sample_neighbors: the adjacency has no rows, so every seed is out of range")
    s = seeds.long()
    sc = s.clamp(0, adj.m - 1)
    lens = (adj.rowptr[sc + 1] - adj.rowptr[sc]).long()
    if fanout > 0:
        lens = lens.clamp(max=fanout)
    ends = torch.cumsum(lens, 0)
    lo, hi, total = torch.stack([s.min(), s.max(), ends[-1]]).tolist()   # the one synchronisation
    if lo < 0 or hi >= adj.m:
        raise ValueError(f"sample_neighbors: seeds must lie in [0, {adj.m}), found {lo if lo < 0 else hi}")
    if total >= 2 ** 31:
        raise ValueError("sample_neighbors: the sample must have fewer than 2^31 entries (split the seeds)")
    out_rowptr[1:] = ends
    out_col = torch.empty(total, dtype=torch.int32, device=dev)
    out_eid = torch.empty(total, dtype=torch.int32, device=dev)
    s32 = seeds.to(torch.int32).contiguous()
    ws = adj._scratch.get("sample", _lib.SAMPLE_WS_BYTES, adj.device)
    call("gcn_sample_neighbors_csr", adj.rowptr, adj.col, adj.m, adj.nnz, s32, ns, int(fanout), int(seed), int(offset),
         out_rowptr, out_col, out_eid, ws, ws.numel(), device=dev)
    return out_rowptr, out_col, out_eid


def _vertex_map(adj):
    """vertex id -> position in the current hop's src, -1 everywhere between hops: n int32, allocated and filled once and
    kept on the adjacency; a hop touches and resets only the entries of its own vertices"""
    vmap = getattr(adj, "_sample_map", None)
    if vmap is None:
        vmap = adj._sample_map = torch.full((adj.n,), -1, dtype=torch.int32, device=adj.device)
    return vmap


def sample_blocks(adj, seeds, fanouts, seed=0, offset=0):
    """The bipartite blocks of a mini-batch: hop l (l = 0 next to the seeds) samples the current frontier with
    ``fanouts[l]`` and Philox offset ``offset + l``; its src vertices are the frontier followed by the distinct sampled
    columns that are not in it, in ascending vertex id, and they are the next hop's frontier.

    adj: a square CsrAdjacency; seeds: distinct vertex ids (1-D int32 / int64 device tensor); fanouts: one per hop.
    Returns (blocks, input_ids): ``blocks`` outermost hop first — the order a forward pass consumes, ``blocks[-1]`` has the
    seeds as its rows — and ``input_ids`` = ``blocks[0].src_ids``, the vertices whose features the batch needs.  A block's
    values are the parent's (``adj.val[eid]``), not renormalised.  The work of a call grows with the number of sampled
    entries only (the n-entry vertex map on ``adj`` is allocated once).  Synchronises with the host: not capturable."""
    if not isinstance(adj, CsrAdjacency):
        raise TypeError("sample_blocks: adj must be a CsrAdjacency")
    if adj.m != adj.n:
        raise ValueError(f"sample_blocks: the adjacency must be square, not {adj.m}x{adj.n}")
    fanouts = list(fanouts)
    if not fanouts:
        raise ValueError("sample_blocks: fanouts must name at least one hop")
    for f in fanouts:
        _check_fanout(f, "sample_blocks")
    _check_stream(seed, offset, "sample_blocks")
    _check_seeds(seeds, "sample_blocks")
    vmap = _vertex_map(adj)
    dst = seeds.long()
    blocks = []
    for hop, fanout in enumerate(fanouts):
        rowptr, col, eid = sample_neighbors(adj, dst, fanout, seed, offset + hop)        # (validates the range of dst)
        num_dst = int(dst.numel())
        vmap[dst] = torch.arange(num_dst, dtype=torch.int32, device=dst.device)
        if hop == 0 and not bool((vmap[dst] == torch.arange(num_dst, dtype=torch.int32, device=dst.device)).all()):
            vmap[dst] = -1
            raise ValueError("sample_blocks: seeds must be distinct")
        c = col.long()
        new = torch.unique(c[vmap[c] < 0])                 # sorted: ascending vertex id
        vmap[new] = torch.arange(num_dst, num_dst + int(new.numel()), dtype=torch.int32, device=dst.device)
        local = vmap[c]
        src = torch.cat([dst, new])
        vmap[src] = -1                                     # back to the cleared state
        block_adj = CsrAdjacency(rowptr, local, adj.val[eid.long()], (num_dst, int(src.numel())), symmetric=False)
        blocks.append(Block(block_adj, eid, src, num_dst))
        dst = src
    blocks.reverse()
    return blocks, dst


class NeighborLoader:
    """Mini-batches of sampled blocks over ``node_idx``: iterating yields ``(blocks, input_ids, batch_seeds)`` with
    ``blocks, input_ids = sample_blocks(adj, batch_seeds, fanouts, seed, offset)``.

    Every epoch (every ``iter()``) draws a fresh permutation of ``node_idx`` from one ``torch.Generator`` seeded with
    ``seed`` (``shuffle=False``: the given order), and the Philox offset runs on from batch to batch and epoch to epoch,
    advancing by ``len(fanouts)`` per batch, so no two hops share one.  ``len()`` is the number of batches; the last may be
    short.  ``last_offset`` is the offset of the most recent batch."""

    def __init__(self, adj, node_idx, fanouts, batch_size, shuffle=True, seed=0):
        if not isinstance(adj, CsrAdjacency):
            raise TypeError("NeighborLoader: adj must be a CsrAdjacency")
        self.fanouts = list(fanouts)
        for f in self.fanouts:
            _check_fanout(f, "NeighborLoader")
        if not self.fanouts:
            raise ValueError("NeighborLoader: fanouts must name at least one hop")
        if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
            raise ValueError(f"NeighborLoader: batch_size must be an int >= 1, not {batch_size!r}")
        _check_stream(seed, 0, "NeighborLoader")
        node_idx = torch.as_tensor(node_idx)
        if node_idx.dim() != 1 or node_idx.dtype not in (torch.int32, torch.int64):
            raise ValueError("NeighborLoader: node_idx must be a 1-D int32 or int64 tensor of vertex ids")
        self.adj, self.batch_size, self.shuffle, self.seed = adj, batch_size, bool(shuffle), seed
        self.node_idx = node_idx.to(device=adj.device, dtype=torch.int64)
        self._gen = torch.Generator(device="cpu")
        self._gen.manual_seed(seed)
        self._offset = 0
        self.last_offset = None

    def __len__(self):
        return (int(self.node_idx.numel()) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        n = int(self.node_idx.numel())
        order = self.node_idx
        if self.shuffle:
            order = order[torch.randperm(n, generator=self._gen).to(order.device)]
        for lo in range(0, n, self.batch_size):
            batch = order[lo:lo + self.batch_size]
            self.last_offset = self._offset
            self._offset += len(self.fanouts)
            blocks, input_ids = sample_blocks(self.adj, batch, self.fanouts, self.seed, self.last_offset)
            yield blocks, input_ids, batch
