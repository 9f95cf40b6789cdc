"""The numpy twins of gcn_amd/construct.py (the contracts of gcn_bucket_count_i32 / gcn_bucket_fill_i32 and
gcn_csr_transpose_gather in include/gcn_spmm.h), and the torch formulations the library used before the device kernels:
the yardsticks of tests/test_construct_gpu.py and of tools/construct_bench.py."""
import numpy as np


def bucket_ref(keys, nbuckets):
    """(offsets int32 [nbuckets + 1], perm int32 [count]): a stable argsort and the prefix sum of a bincount"""
    keys = np.asarray(keys, np.int64)
    offsets = np.zeros(nbuckets + 1, np.int64)
    if len(keys):
        offsets[1:] = np.cumsum(np.bincount(keys, minlength=nbuckets))
    return offsets.astype(np.int32), np.argsort(keys, kind="stable").astype(np.int32)


def transpose_ref(rowptr, col, val, n):
    """(trowptr [n + 1], trow, tval, eid) of the transpose with repeated entries kept apart: entry t is source entry
    eid[t]; a transposed row lists its entries in ascending source entry (ascending row, repeats in source order)"""
    rowptr = np.asarray(rowptr, np.int64)
    trp, eid = bucket_ref(col, n)
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    return trp, rows[eid].astype(np.int32), np.asarray(val, np.float32)[eid], eid


def csr_from_edges_ref(rows, cols, shape, values=None, sort_columns=True):
    """(rowptr, col, val, eid): edges bucketed by row, in input order inside a row, or ascending by column with repeated
    pairs in input order (np.lexsort is stable); values None (ones), an array carried along, or "gcn" (1 / sqrt(len_i *
    len_j) from the result's own row lengths, in fp64, rounded once)"""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    m = shape[0]
    eid = np.lexsort((cols, rows)) if sort_columns else np.argsort(rows, kind="stable")
    rowptr = np.zeros(m + 1, np.int64)
    if len(rows):
        rowptr[1:] = np.cumsum(np.bincount(rows, minlength=m))
    col = cols[eid]
    if values is None:
        val = np.ones(len(rows), np.float32)
    elif isinstance(values, str):
        lens = np.maximum(np.diff(rowptr), 1).astype(np.float64)
        val = (1.0 / np.sqrt(lens[rows[eid]] * lens[col])).astype(np.float32)
    else:
        val = np.asarray(values, np.float32)[eid]
    return rowptr.astype(np.int32), col.astype(np.int32), val, eid.astype(np.int32)


def torch_transposed_pattern(adj):
    """CsrAdjacency._transposed_pattern as it was built with torch ops before the device kernels, verbatim"""
    import torch
    self = adj
    dev = self.device
    rp = self.rowptr.long()
    rows = torch.repeat_interleave(torch.arange(self.m, device=dev), rp[1:] - rp[:-1], output_size=self.nnz)
    c = self.col.long()
    perm = torch.argsort(c * max(self.m, 1) + rows, stable=True)
    trp = torch.zeros(self.n + 1, dtype=torch.int64, device=dev)
    trp[1:] = torch.cumsum(torch.bincount(c, minlength=self.n), 0)
    return trp.to(torch.int32), rows[perm].to(torch.int32), perm


def torch_coo_transpose(adj):
    """(rowptr, col, val) of CsrAdjacency.transpose() as it was built before the device kernels: CSR -> COO -> transposed
    and coalesced (repeated entries summed) -> CSR"""
    import torch
    csr = torch.sparse_csr_tensor(adj.rowptr.long(), adj.col.long(), adj.val, size=(adj.m, adj.n))
    t = csr.to_sparse_coo().t().coalesce().to_sparse_csr()
    return t.crow_indices(), t.col_indices(), t.values()
