"""Building and transposing CSR on the device: stable bucketing of indices by an integer key, and what hangs on it.

    offsets, perm = gcn_amd.bucket_by_key(keys, nbuckets)          # argsort(keys, stable) and the buckets' pointers
    at, eid = gcn_amd.transpose_csr(adj)                           # Âᵀ with duplicates kept apart; entry t is adj's eid[t]
    adj, eid = gcn_amd.csr_from_edges(rows, cols, (m, n), values="gcn")

The primitive is an exact contract written out in include/gcn_spmm.h (``gcn_bucket_count_i32`` / ``gcn_bucket_fill_i32``,
``gcn_csr_transpose_gather``) and runs on gcn_amd/csrc/construct.hip; tests/construct_ref.py is its numpy twin.
``CsrAdjacency.transpose()`` and the transposed pattern behind the gradient of ``aggregate`` are built here.  There is no
CPU path: CPU tensors raise.
"""
import torch

from . import _lib
from ._lib import call
from .spmm import CsrAdjacency


def _check_ids(ids, name, what):
    if not isinstance(ids, torch.Tensor) or ids.dim() != 1 or ids.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: {name} must be a 1-D int32 or int64 tensor")


def _check_size(v, name, what):
    if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 2 ** 31:
        raise ValueError(f"{what}: {name} must be an int in [0, 2^31), not {v!r}")


def _bucket(keys32, nbuckets):
    """(offsets int32 [nbuckets + 1], perm int32 [count]) for contiguous int32 device keys that are known to lie in
    [0, nbuckets): count, scan in place, fill; nothing is read back"""
    dev = keys32.device
    count = int(keys32.numel())
    offsets = torch.empty(nbuckets + 1, dtype=torch.int32, device=dev)
    perm = torch.empty(count, dtype=torch.int32, device=dev)
    call("gcn_bucket_count_i32", keys32, count, nbuckets, offsets, device=dev)
    offsets.cumsum_(0)                                     # (the total is count < 2^31: int32 holds every partial sum)
    if count > 0 and nbuckets > 0:
        ws = torch.empty(_lib.bucket_ws_bytes(count, nbuckets), dtype=torch.uint8, device=dev)
        call("gcn_bucket_fill_i32", keys32, count, nbuckets, offsets, perm, ws, ws.numel(), device=dev)
    return offsets, perm


def bucket_by_key(keys, nbuckets):
    """Stable bucketing: ``perm[offsets[b]:offsets[b + 1]]`` holds exactly the indices ``i`` with ``keys[i] == b``, in
    ascending ``i`` — ``np.argsort(keys, kind="stable")`` with the prefix sum of ``np.bincount(keys, minlength=nbuckets)``
    as the offsets, bit for bit and the same at every call.

    keys: a 1-D int32 or int64 device tensor with every key in [0, nbuckets), fewer than 2^31 of them.  nbuckets: an int in
    [0, 2^31).  Returns (offsets int32 [nbuckets + 1], perm int32 [len(keys)]).  One host synchronisation (the range of the
    keys): not capturable.  ValueError for a bad nbuckets, dtype, shape or a key out of range, GcnAmdError for CPU tensors."""
    _check_size(nbuckets, "nbuckets", "bucket_by_key")
    _check_ids(keys, "keys", "bucket_by_key")
    if not keys.is_cuda:
        raise _lib.GcnAmdError("bucket_by_key: keys must be a CUDA/HIP tensor (no CPU path in gcn_amd)")
    count = int(keys.numel())
    if count >= 2 ** 31:
        raise ValueError("bucket_by_key: fewer than 2^31 keys per call")
    if count > 0:
        lo, hi = torch.stack([keys.min(), keys.max()]).tolist()          # the one synchronisation
        if lo < 0 or hi >= nbuckets:
            raise ValueError(f"bucket_by_key: keys must lie in [0, {nbuckets}), found {lo if lo < 0 else hi}")
    return _bucket(keys.to(torch.int32).contiguous(), nbuckets)


def _transpose_arrays(adj, with_values=True):
    """(rowptr int32 [n + 1], row of each entry int32 [nnz], values fp32 [nnz] or None, eid int32 [nnz]) of Âᵀ: the
    bucketing of adj's entries by column (its columns lie in [0, n): the SpMM's own precondition) and one gather"""
    dev = adj.device
    trp, eid = _bucket(adj.col, adj.n)
    trow = torch.empty(adj.nnz, dtype=torch.int32, device=dev)
    tval = torch.empty(adj.nnz, dtype=torch.float32, device=dev) if with_values else None
    if adj.nnz > 0:
        call("gcn_csr_transpose_gather", adj.rowptr, adj.m, adj.nnz, eid, adj.val if with_values else None, trow, tval,
             device=dev)
    return trp, trow, tval, eid


def transpose_csr(adj):
    """Âᵀ of any CsrAdjacency, built on the device: returns ``(CsrAdjacency [n x m], eid int32 [nnz])``.

    Entry t of the result is entry ``eid[t]`` of ``adj`` and carries ``adj.val[eid[t]]``.  A row of the result (a column
    of ``adj``) lists its entries by ascending source row; a (row, column) pair that ``adj`` stores more than once stays
    that many separate entries, in their source order — nothing is merged, as everywhere in this library, where repeated
    entries add.  The result is flagged ``symmetric=False``.  No host synchronisation (the sizes are ``adj.nnz`` and
    ``adj.n``).  TypeError for a non-CsrAdjacency, GcnAmdError for an adjacency that is not on a device."""
    if not isinstance(adj, CsrAdjacency):
        raise TypeError("transpose_csr: adj must be a CsrAdjacency")
    if adj.device.type != "cuda":
        raise _lib.GcnAmdError("transpose_csr: the adjacency must live on a CUDA/HIP device (no CPU path in gcn_amd)")
    trp, trow, tval, eid = _transpose_arrays(adj)
    return CsrAdjacency(trp, trow, tval, (adj.n, adj.m), symmetric=False, chunk_nnz=adj.chunk_nnz), eid


def csr_from_edges(rows, cols, shape, values=None, sort_columns=True):
    """A CsrAdjacency from an edge list on the device: returns ``(CsrAdjacency [shape], eid int32 [E])``; entry t of the
    result is edge ``eid[t]`` of the input.

    rows, cols: 1-D int32 or int64 device tensors of equal length E < 2^31, rows in [0, shape[0]) and cols in [0, shape[1]).
    values: None (ones), an fp32 device tensor [E] carried along as ``values[eid]``, or "gcn": ``1 / sqrt(len_i * len_j)``
    from the result's own row lengths, the rule of ``induced_subgraph(values="gcn")``.  "gcn" needs a square shape and
    ASSUMES THE EDGE LIST CARRIES ITS SELF-LOOPS (i, i) and both directions of every edge, as a normalised adjacency's
    pattern does: none is added here.
    sort_columns=True: every row comes out ascending by column, repeated (row, column) pairs in input order — two stable
    bucketings, by column and then by row, i.e. ``np.lexsort((cols, rows))``.  False: one bucketing by row, the entries of
    a row keep their input order.
    REPEATED EDGES ARE NOT MERGED: they stay separate entries, and every kernel of this library adds them (a repeated edge
    weighs twice).  Symmetrising and inserting missing self-loops are out of scope here; both need a merge step, which
    lives in coalesce.py: ``coalesce_csr``, ``symmetrize``, and ``gcn_adjacency`` for the whole way from an edge list to Â.
    The result is flagged ``symmetric=False`` (nothing here checks symmetry; pass the arrays to ``CsrAdjacency`` with
    ``symmetric=True`` when it is known).  One host synchronisation (the range of the ids): not capturable.
    ValueError for a bad dtype, shape, length, values or an id out of range, GcnAmdError for CPU tensors."""
    what = "csr_from_edges"
    _check_ids(rows, "rows", what)
    _check_ids(cols, "cols", what)
    if rows.numel() != cols.numel():
        raise ValueError(f"{what}: rows and cols must have the same length, not {rows.numel()} and {cols.numel()}")
    if not isinstance(shape, (tuple, list, torch.Size)) or len(shape) != 2:
        raise ValueError(f"{what}: shape must be (rows, columns), not {shape!r}")
    m, n = shape
    _check_size(m, "shape[0]", what)
    _check_size(n, "shape[1]", what)
    E = int(rows.numel())
    if isinstance(values, str):
        if values != "gcn":
            raise ValueError(f"{what}: values must be None, an fp32 tensor [E] or \"gcn\", not {values!r}")
        if m != n:
            raise ValueError(f"{what}: values=\"gcn\" needs a square shape, not {m}x{n}")
    elif values is not None:
        if not isinstance(values, torch.Tensor) or values.dtype != torch.float32 or values.dim() != 1 or values.numel() != E:
            raise ValueError(f"{what}: values must be None, an fp32 tensor [E] or \"gcn\"")
    if E >= 2 ** 31:
        raise ValueError(f"{what}: fewer than 2^31 edges per call")
    if not (rows.is_cuda and cols.is_cuda and (not isinstance(values, torch.Tensor) or values.is_cuda)):
        raise _lib.GcnAmdError(f"{what}: rows, cols and values must be CUDA/HIP tensors (no CPU path in gcn_amd)")
    dev = rows.device
    if E > 0:
        rlo, rhi, clo, chi = torch.stack([rows.min(), rows.max(), cols.min(), cols.max()]).tolist()   # the one synchronisation
        if rlo < 0 or rhi >= m:
            raise ValueError(f"{what}: rows must lie in [0, {m}), found {rlo if rlo < 0 else rhi}")
        if clo < 0 or chi >= n:
            raise ValueError(f"{what}: cols must lie in [0, {n}), found {clo if clo < 0 else chi}")
    r32, c32 = rows.to(torch.int32).contiguous(), cols.to(torch.int32).contiguous()
    if sort_columns:
        _, by_col = _bucket(c32, n)                        # LSD: the minor key first
        rowptr, by_row = _bucket(r32.index_select(0, by_col), m)
        eid = by_col.index_select(0, by_row)
    else:
        rowptr, eid = _bucket(r32, m)
    col = c32.index_select(0, eid)
    if values is None:
        val = torch.ones(E, dtype=torch.float32, device=dev)
    elif isinstance(values, torch.Tensor):
        val = values.index_select(0, eid)
    else:
        lens = (rowptr[1:] - rowptr[:-1]).double().clamp(min=1.0)       # (a column's own row is empty only in an asymmetric pattern)
        val = (lens[r32.index_select(0, eid)] * lens[col]).rsqrt().float()
    return CsrAdjacency(rowptr, col, val, (m, n), symmetric=False), eid
