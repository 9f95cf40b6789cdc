"""Link prediction: edge lookup, negative sampling, edge splits, pair scores and a mini-batch loader over edges (DGL's
``has_edges_between`` / ``edge_ids``, ``GlobalUniform`` negative sampler and ``EdgeDataLoader``; PyG's ``RandomLinkSplit`` and
``LinkNeighborLoader``).

    eid = gcn_amd.find_edges(adj, rows, cols)                      # entry index of (rows[i], cols[i]), or -1
    rev = gcn_amd.reverse_entries(adj)                             # entry index of (c, r) for every entry (r, c)
    neg = gcn_amd.negative_sample(adj, rows, num_neg=2, seed=0, offset=0)
    train_adj, train_eid, val_eid, test_eid = gcn_amd.split_edges(adj, 0.05, 0.10)
    for blocks, input_ids, pr, pc, labels in gcn_amd.LinkNeighborLoader(train_adj, eids, [10, 5], batch_size=512):
        z = model(x[input_ids], blocks)                            # model = gcn_amd.GraphSAGE(...)
        loss = bce_with_logits(gcn_amd.pair_scores(z, z, pr, pc).squeeze(1), labels)

The lookup and the rejection sampler are exact contracts written out in include/gcn_spmm.h (``gcn_csr_find_entries``,
``gcn_negative_sample_csr``) and run on gcn_amd/csrc/lookup.hip; tests/linkpred_ref.py is their numpy twin.  Both need rows
whose columns ascend; the first call on an adjacency checks that once (one host synchronisation) and keeps the answer on
the adjacency, after which ``find_edges`` and ``negative_sample`` only enqueue and can be captured in a HIP graph.  A
negative is a pure function of (seed, offset, its flat slot, max_tries, its row), not of the batch it is drawn in.
Everything here except ``pair_scores`` is integer work without a gradient; ``pair_scores`` is ``sddmm_heads`` on the
pattern of the pairs.  There is no CPU path: CPU tensors raise.
"""
import torch

from . import _lib
from ._lib import call
from .attention import sddmm_heads
from .coalesce import _entry_rows
from .construct import csr_from_edges
from .sampling import _check_fanout, _check_stream, sample_blocks
from .spmm import CsrAdjacency, dropout_rows

MAX_TRIES = 64                                         # the most candidates gcn_negative_sample_csr draws for a slot


def _check_adj(adj, what):
    if not isinstance(adj, CsrAdjacency):
        raise TypeError(f"{what}: adj must be a CsrAdjacency")


def _check_ids(ids, name, what):
    if not isinstance(ids, torch.Tensor) or ids.dim() != 1 or ids.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: {name} must be a 1-D int32 or int64 tensor")


def _check_int(v, name, what, lo, hi):
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError(f"{what}: {name} must be an int in [{lo}, {hi}], not {v!r}")


def _check_sorted(adj, what):
    """ValueError unless every row of adj holds ascending columns (repeats allowed).  Computed at the first call — one
    elementwise expression over col and one host synchronisation — and kept on the adjacency, whose pattern never changes"""
    ok = getattr(adj, "_cols_ascend", None)
    if ok is None:
        if adj.nnz < 2:
            ok = True
        else:
            first = torch.zeros(adj.nnz + 1, dtype=torch.bool, device=adj.col.device)
            first[adj.rowptr.long()] = True                # the entries that begin a row
            ok = bool(((adj.col[1:] >= adj.col[:-1]) | first[1:adj.nnz]).all())
        adj._cols_ascend = ok
    if not ok:
        raise ValueError(f"{what}: the rows of the adjacency must hold ascending columns; build it with "
                         "csr_from_edges(sort_columns=True) or pass it through coalesce_csr first")


def _check_on_device(adj, tensors, what):
    if adj.device.type != "cuda" or not all(t.is_cuda for t in tensors):
        raise _lib.GcnAmdError(f"{what}: the adjacency and the queries must be CUDA/HIP tensors (no CPU path in gcn_amd)")


def find_edges(adj, rows, cols):
    """The entry index of every pair (rows[i], cols[i]) in ``adj``, or -1 when it is not stored.

    adj: a CsrAdjacency whose rows hold ascending columns (its values are not used).  rows, cols: 1-D int32 or int64 device
    tensors of equal length.  Returns int32 [len(rows)]: the LOWEST entry index e of row rows[i] with ``adj.col[e] ==
    cols[i]`` (a row may repeat a column); -1 for a pair that is not stored and for a row or column outside the matrix.
    The first call on an adjacency checks the column order (one host synchronisation); after it the call only enqueues.
    TypeError for a non-CsrAdjacency, ValueError for a bad dtype or shape, unequal lengths or rows that do not ascend,
    GcnAmdError for CPU tensors."""
    what = "find_edges"
    _check_adj(adj, what)
    _check_ids(rows, "rows", what)
    _check_ids(cols, "cols", what)
    if rows.numel() != cols.numel():
        raise ValueError(f"{what}: rows and cols must have the same length, not {rows.numel()} and {cols.numel()}")
    q = int(rows.numel())
    if q >= 2 ** 31:
        raise ValueError(f"{what}: fewer than 2^31 queries per call")
    _check_sorted(adj, what)
    _check_on_device(adj, (rows, cols), what)
    dev = rows.device
    out = torch.empty(q, dtype=torch.int32, device=dev)
    if q > 0:
        # (an int64 id beyond int32 is not a row or column of the matrix: clamped to -1, which is not found)
        r32, c32 = (t if t.dtype == torch.int32 else torch.where((t >= 0) & (t < 2 ** 31), t, -1).to(torch.int32)
                    for t in (rows, cols))
        call("gcn_csr_find_entries", adj.rowptr, adj.col, adj.m, adj.nnz, r32.contiguous(), c32.contiguous(), q, out, device=dev)
    return out


def reverse_entries(adj):
    """int32 [nnz]: for every entry (r, c) of the square ``adj`` the entry index of (c, r) — the lowest one when (c, r) is
    stored more than once — or -1 when it is not stored.  A diagonal entry is its own reverse (the lowest of its repeats).
    On a pattern without repeated entries that holds both directions of every edge this is an involution.  Built on
    ``find_edges``, under its conditions."""
    _check_adj(adj, "reverse_entries")
    if adj.m != adj.n:
        raise ValueError(f"reverse_entries: the adjacency must be square, not {adj.m}x{adj.n}")
    _check_sorted(adj, "reverse_entries")
    _check_on_device(adj, (), "reverse_entries")
    return find_edges(adj, adj.col, _entry_rows(adj))


def negative_sample(adj, rows, num_neg=1, seed=0, offset=0, max_tries=32, exclude_self=True):
    """``num_neg`` columns for every ``rows[i]`` that row rows[i] of ``adj`` does NOT store, uniform over those columns.

    adj: a CsrAdjacency whose rows hold ascending columns.  rows: a 1-D int32 or int64 device tensor of row ids, repeats
    allowed.  Returns int32 [len(rows), num_neg].  Slot (i, s) is drawn by rejection from at most ``max_tries`` (1 .. 64)
    uniform candidates in [0, adj.n) and is -1 when every one of them is stored in the row (or, with ``exclude_self``,
    is the row itself), and for a row outside [0, adj.m): a row that stores a fraction f of the columns fails with
    probability f^max_tries.  The slot is a pure function of (seed, offset, i * num_neg + s, max_tries, the row): it does
    not depend on the other queries, and successive batches must use different offsets.  The slots of one query are
    independent, so two of them may hold the same column.  The first call on an adjacency checks the column order (one
    host synchronisation); after it the call only enqueues.
    TypeError for a non-CsrAdjacency, ValueError for a bad num_neg, seed, offset, max_tries, dtype or shape, rows that do
    not ascend or 2^31 slots or more, GcnAmdError for CPU tensors."""
    what = "negative_sample"
    _check_adj(adj, what)
    _check_int(num_neg, "num_neg", what, 1, 2 ** 31 - 1)
    _check_stream(seed, offset, what)
    _check_int(max_tries, "max_tries", what, 1, MAX_TRIES)
    _check_ids(rows, "rows", what)
    q = int(rows.numel())
    if q * num_neg >= 2 ** 31:
        raise ValueError(f"{what}: fewer than 2^31 slots (rows x num_neg) per call")
    _check_sorted(adj, what)
    _check_on_device(adj, (rows,), what)
    if q > 0 and adj.n < 1:
        raise ValueError(f"{what}: the adjacency has no columns to draw from")
    dev = rows.device
    out = torch.empty((q, num_neg), dtype=torch.int32, device=dev)
    if q > 0:
        r32 = rows if rows.dtype == torch.int32 else torch.where((rows >= 0) & (rows < 2 ** 31), rows, -1).to(torch.int32)
        call("gcn_negative_sample_csr", adj.rowptr, adj.col, adj.m, adj.n, adj.nnz, r32.contiguous(), q, num_neg, max_tries,
             int(bool(exclude_self)), int(seed), int(offset), out, device=dev)
    return out


def edge_subgraph(adj, keep):
    """The entries ``e`` of ``adj`` with ``keep[e]``, as ``(CsrAdjacency [m x n], eid int32)``: the kept entries in the
    parent's entry order (a column-sorted row stays sorted) with the parent's values, ``eid`` their parent entry indices.

    keep: a bool device tensor [nnz].  torch ops only — ``rowptr' = prefix(keep)[rowptr]``, ``col[keep]`` — and one host
    synchronisation (the number of kept entries).  The values are NOT renormalised.  The result keeps the parent's
    ``symmetric`` flag only when nothing is dropped."""
    what = "edge_subgraph"
    _check_adj(adj, what)
    if not isinstance(keep, torch.Tensor) or keep.dtype != torch.bool or keep.dim() != 1 or keep.numel() != adj.nnz:
        raise ValueError(f"{what}: keep must be a bool tensor [nnz = {adj.nnz}]")
    _check_on_device(adj, (keep,), what)
    prefix = torch.zeros(adj.nnz + 1, dtype=torch.int32, device=keep.device)
    prefix[1:] = torch.cumsum(keep, 0)
    eid = torch.nonzero(keep).squeeze(1).to(torch.int32)                  # the one synchronisation
    idx = eid.long()
    sub = CsrAdjacency(prefix[adj.rowptr.long()], adj.col[idx], adj.val[idx], (adj.m, adj.n),
                       symmetric=adj.symmetric if int(eid.numel()) == adj.nnz else False)
    if getattr(adj, "_cols_ascend", None):
        sub._cols_ascend = True                            # (a subsequence of an ascending row ascends)
    return sub, eid


TRAIN, VAL, TEST = 0, 1, 2


def _check_frac(v, name, what):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= v < 1.0:
        raise ValueError(f"{what}: {name} must be a number in [0, 1), not {v!r}")


def _split_parts(adj, val_frac, test_frac, seed, undirected):
    """uint8 [nnz]: TRAIN / VAL / TEST of every entry (the rule is written out at split_edges)"""
    dev = adj.device
    ones = torch.ones(adj.nnz, dtype=torch.float32, device=dev)
    # dropout_rows keeps element e iff its Philox word is >= p * 2^32: "not kept at p" is "word below the threshold of p"
    below = lambda p: (dropout_rows(ones, p, seed, 0) == 0) if p > 0 else torch.zeros(adj.nnz, dtype=torch.bool, device=dev)
    in_val, in_held = below(val_frac), below(val_frac + test_frac)
    part = in_held.to(torch.uint8) * TEST                  # word < thr(val + test): held out ...
    part[in_val] = VAL                                     # ... and VAL when it is also < thr(val) <= thr(val + test)
    if undirected:
        rows, cols = _entry_rows(adj), adj.col
        part[rows == cols] = TRAIN
        lower = rows > cols
        rev = find_edges(adj, cols, rows).long()
        if bool(((rev < 0) & (rows != cols)).any()):
            raise ValueError("split_edges: undirected=True needs the reverse (c, r) of every entry (r, c); symmetrize the "
                             "adjacency first or pass undirected=False")
        part[lower] = part[rev[lower]]
    return part


def split_edges(adj, val_frac, test_frac, seed=0, undirected=True):
    """A random split of the stored entries into train / validation / test, and the message-passing graph without the
    held-out entries: returns ``(train_adj, train_eid, val_eid, test_eid)``, entry indices into ``adj`` as int32, ascending.

    Entry e is decided by one 32-bit Philox4x32-10 word, the dropout mask's word of element e with this ``seed`` at offset
    0: validation when it is below ``float32(val_frac) * 2^32``, else test when it is below ``float32(val_frac + test_frac)
    * 2^32``, else train.  ``undirected=True`` (a square adjacency with column-sorted rows that stores both directions):
    the decision of an entry (r, c) with r > c is the decision of its reverse entry ``reverse_entries(adj)``, so both
    directions land in the same part; diagonal entries stay in train; ``val_eid`` / ``test_eid`` list the r < c direction
    only (score the other direction by swapping the pair), while ``train_adj`` holds both directions of its edges.  On a
    pattern with repeated entries every r < c entry decides for itself and the r > c copies follow the lowest one.
    ``train_adj, train_eid = edge_subgraph(adj, train mask)``: parent values, not renormalised.
    ValueError for fractions outside [0, 1) or summing to 1 or more, a bad seed, and with ``undirected`` an adjacency that
    is not square, not column-sorted, or lacks the reverse of an entry.  Synchronises with the host: not capturable."""
    what = "split_edges"
    _check_adj(adj, what)
    _check_frac(val_frac, "val_frac", what)
    _check_frac(test_frac, "test_frac", what)
    if not val_frac + test_frac < 1.0:
        raise ValueError(f"{what}: val_frac + test_frac must be below 1, not {val_frac + test_frac!r}")
    _check_stream(seed, 0, what)
    if undirected:
        if adj.m != adj.n:
            raise ValueError(f"{what}: undirected=True needs a square adjacency, not {adj.m}x{adj.n}")
        _check_sorted(adj, what)
    _check_on_device(adj, (), what)
    part = _split_parts(adj, float(val_frac), float(test_frac), seed, bool(undirected))
    listed = (_entry_rows(adj) < adj.col) if undirected else torch.ones(adj.nnz, dtype=torch.bool, device=adj.device)
    val_eid = torch.nonzero((part == VAL) & listed).squeeze(1).to(torch.int32)
    test_eid = torch.nonzero((part == TEST) & listed).squeeze(1).to(torch.int32)
    train_adj, train_eid = edge_subgraph(adj, part == TRAIN)
    return train_adj, train_eid, val_eid, test_eid


def pair_scores(z_rows, z_cols, rows, cols, heads=1):
    """s[i, h] = the dot product of head h of ``z_rows[rows[i]]`` and ``z_cols[cols[i]]`` for arbitrary pairs, repeats
    allowed: returns fp32 [len(rows), heads].

    z_rows: [m, H*F], z_cols: [n, H*F] fp32 device tensors (the same tensor for one embedding table), head h in columns
    hF .. hF + F - 1.  rows in [0, m), cols in [0, n): 1-D int32 or int64 device tensors of equal length.  Differentiable
    in both operands.  Composed of what exists: ``csr_from_edges(rows, cols, (m, n), sort_columns=False)`` makes the pairs
    a pattern, ``sddmm_heads`` scores its entries (gradients: ``spmm_heads`` on the pattern and its transpose), and an
    ``index_select`` through the inverse of the bucketing's ``eid`` puts the scores back in pair order — no float
    intermediate of the size of the pairs beyond the scores.  One host synchronisation (csr_from_edges checks the range
    of the ids).  ValueError for bad shapes, dtypes or ids out of range, GcnAmdError for CPU tensors."""
    what = "pair_scores"
    for t, name in ((z_rows, "z_rows"), (z_cols, "z_cols")):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise ValueError(f"{what}: {name} must be a 2-D fp32 tensor [*, H*F]")
    pattern, eid = csr_from_edges(rows, cols, (int(z_rows.shape[0]), int(z_cols.shape[0])), sort_columns=False)
    s = sddmm_heads(pattern, z_rows, z_cols, heads)        # entry t of the pattern is pair eid[t]
    inv = torch.empty_like(eid, dtype=torch.int64)
    inv[eid.long()] = torch.arange(eid.numel(), dtype=torch.int64, device=eid.device)
    return s.index_select(0, inv)


class LinkNeighborLoader:
    """Mini-batches for link prediction over the entries ``eids`` of ``adj``: iterating yields ``(blocks, input_ids,
    pair_rows, pair_cols, labels)``.

    Per batch of positive entries e, at Philox offset ``o``: the positives are (row(e), col[e]) — the rows by
    ``torch.searchsorted`` on ``rowptr`` —; ``negative_sample(adj, rows, num_neg, seed, o, max_tries)`` draws the negatives
    (row(e), c'), whose -1 slots are dropped; ``nodes`` are the sorted distinct endpoints of all pairs, and ``blocks,
    input_ids = sample_blocks(adj, nodes, fanouts, seed, o + 1)``.  The pairs are the positives in batch order followed by
    the surviving negatives in slot order, as POSITIONS IN ``nodes`` — the row order of ``blocks[-1]``, so of the model's
    output — and ``labels`` is fp32, 1 for a positive and 0 for a negative.  The blocks are sampled from ``adj`` as it is:
    a batch's positive edges are not removed from it (pass the train graph of ``split_edges`` and its entries).

    Every epoch draws a fresh permutation of ``eids`` from one ``torch.Generator`` seeded with ``seed`` (``shuffle=False``:
    the given order); the offset advances by ``1 + len(fanouts)`` per batch and runs on across epochs, so no two draws
    share one.  ``len()`` is the number of batches; the last may be short.  ``last_offset`` is ``o`` of the most recent
    batch and ``last_eids`` its entries."""

    def __init__(self, adj, eids, fanouts, batch_size, num_neg=1, shuffle=True, seed=0, max_tries=32):
        what = "LinkNeighborLoader"
        _check_adj(adj, what)
        if adj.m != adj.n:
            raise ValueError(f"{what}: the adjacency must be square, not {adj.m}x{adj.n}")
        self.fanouts = list(fanouts)
        for f in self.fanouts:
            _check_fanout(f, what)
        if not self.fanouts:
            raise ValueError(f"{what}: fanouts must name at least one hop")
        _check_int(batch_size, "batch_size", what, 1, 2 ** 31 - 1)
        _check_int(num_neg, "num_neg", what, 1, 2 ** 31 - 1)
        _check_int(max_tries, "max_tries", what, 1, MAX_TRIES)
        _check_stream(seed, 0, what)
        eids = torch.as_tensor(eids)
        _check_ids(eids, "eids", what)
        _check_sorted(adj, what)
        _check_on_device(adj, (), what)
        self.adj, self.batch_size, self.num_neg, self.shuffle, self.seed = adj, batch_size, num_neg, bool(shuffle), seed
        self.max_tries = max_tries
        self.eids = eids.to(device=adj.device, dtype=torch.int64)
        if self.eids.numel() and not (0 <= int(self.eids.min()) and int(self.eids.max()) < adj.nnz):
            raise ValueError(f"{what}: eids must lie in [0, nnz = {adj.nnz})")
        self._gen = torch.Generator(device="cpu")
        self._gen.manual_seed(seed)
        self._offset = 0
        self.last_offset = self.last_eids = None

    def __len__(self):
        return (int(self.eids.numel()) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        adj, count = self.adj, int(self.eids.numel())
        order = self.eids
        if self.shuffle:
            order = order[torch.randperm(count, generator=self._gen).to(order.device)]
        rowptr = adj.rowptr.long()
        for lo in range(0, count, self.batch_size):
            e = order[lo:lo + self.batch_size]
            self.last_offset, self.last_eids = self._offset, e
            self._offset += 1 + len(self.fanouts)
            rows = torch.searchsorted(rowptr, e, right=True) - 1
            cols = adj.col[e].long()
            neg = negative_sample(adj, rows, self.num_neg, self.seed, self.last_offset, self.max_tries).reshape(-1).long()
            drawn = neg >= 0
            u = torch.cat([rows, rows.repeat_interleave(self.num_neg)[drawn]])
            v = torch.cat([cols, neg[drawn]])
            nodes = torch.unique(torch.cat([u, v]))        # sorted and distinct
            labels = torch.zeros(u.numel(), dtype=torch.float32, device=u.device)
            labels[:e.numel()] = 1.0
            blocks, input_ids = sample_blocks(adj, nodes, self.fanouts, self.seed, self.last_offset + 1)
            yield blocks, input_ids, torch.searchsorted(nodes, u), torch.searchsorted(nodes, v), labels
