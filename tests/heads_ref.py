"""fp64 numpy twins of the head-batched attention primitives (gcn_amd/csrc/multihead.hip): the contract of
include/gcn_spmm.h written a second time, on the host, with no regard for speed or summation order.

Layouts as in the header: per-entry arrays [nnz, H], node arrays [rows, H*F] with head h in columns hF .. hF+F-1,
per-node scalars [rows, H]."""
import numpy as np
import scipy.sparse as sp


def entry_rows(rowptr):
    rowptr = np.asarray(rowptr, np.int64)
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def _row_reduce(ufunc, x, rowptr, empty):
    """ufunc over each row's entries of x [nnz, H] -> [rows, H] (`empty` for a row without entries)"""
    rowptr = np.asarray(rowptr, np.int64)
    lens = np.diff(rowptr)
    out = np.full((len(lens), x.shape[1]), empty, np.float64)
    ne = lens > 0
    if ne.any():
        out[ne] = ufunc.reduceat(x, rowptr[:-1][ne], axis=0)
    return out


def row_sums(rowptr, x):
    return _row_reduce(np.add, np.asarray(x, np.float64), rowptr, 0.0)


def transpose_pattern(rowptr, col, n):
    """(trowptr [n + 1], trow [nnz], tperm [nnz]): entry t of the transposed pattern is entry tperm[t] of the CSR and sits
    in its row trow[t]; a column's entries keep their CSR order (a stable bucketing)"""
    col = np.asarray(col, np.int64)
    tperm = np.argsort(col, kind="stable")
    trowptr = np.zeros(n + 1, np.int64)
    trowptr[1:] = np.cumsum(np.bincount(col, minlength=n))
    return trowptr, entry_rows(rowptr)[tperm], tperm


def edge_softmax(rowptr, s):
    """per (row, head): exp(s - max) / sum; an all -inf (row, head) gives zeros; -inf beside a finite score gives 0"""
    s = np.asarray(s, np.float64)
    row = entry_rows(rowptr)
    mx = _row_reduce(np.maximum, s, rowptr, 0.0)
    mx = np.where(np.isneginf(mx), 0.0, mx)
    with np.errstate(invalid="ignore"):
        e = np.exp(s - mx[row])
    den = row_sums(rowptr, e)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(den == 0.0, 0.0, 1.0 / den)
    return e * inv[row]


def edge_softmax_backward(rowptr, p, g):
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    row = entry_rows(rowptr)
    return p * (g - row_sums(rowptr, p * g)[row])


def gat_pre(rowptr, col, a_dst, a_src):
    return np.asarray(a_dst, np.float64)[entry_rows(rowptr)] + np.asarray(a_src, np.float64)[np.asarray(col, np.int64)]


def gat_scores(rowptr, col, a_dst, a_src, slope):
    """leaky_relu of the sum of the two fp32 operands, the sum rounded to fp32 as the kernel forms it"""
    a_dst, a_src = np.asarray(a_dst, np.float32), np.asarray(a_src, np.float32)
    t = a_dst[entry_rows(rowptr)] + a_src[np.asarray(col, np.int64)]
    return np.where(t > 0, t, t * np.float32(slope)).astype(np.float32)


def gat_edge_softmax(rowptr, col, a_dst, a_src, slope):
    return edge_softmax(rowptr, gat_scores(rowptr, col, a_dst, a_src, slope))


def gat_edge_softmax_backward(rowptr, col, a_dst, a_src, slope, p, g):
    """(ds [nnz, H], grad_a_dst [m, H]); the derivative of leaky_relu at 0 is the slope"""
    a_dst, a_src = np.asarray(a_dst, np.float32), np.asarray(a_src, np.float32)
    pre = a_dst[entry_rows(rowptr)] + a_src[np.asarray(col, np.int64)]
    ds = edge_softmax_backward(rowptr, p, g) * np.where(pre > 0, 1.0, float(slope))
    return ds, row_sums(rowptr, ds)


def segment_sum(rowptr, x, perm=None):
    x = np.asarray(x, np.float64)
    return row_sums(rowptr, x if perm is None else x[np.asarray(perm, np.int64)])


def spmm_heads(rowptr, idx, perm, vals, x, heads, rows_in=None):
    """out[r, hF+j] = sum over the entries e of row r of vals[perm[e] or e, h] * x[idx[e], hF+j]"""
    rowptr, idx = np.asarray(rowptr, np.int64), np.asarray(idx, np.int64)
    vals, x = np.asarray(vals, np.float64), np.asarray(x, np.float64)
    if perm is not None:
        vals = vals[np.asarray(perm, np.int64)]
    rows, k = len(rowptr) - 1, x.shape[1]
    F = k // heads
    out = np.zeros((rows, k))
    for h in range(heads):
        A = sp.csr_matrix((vals[:, h], idx, rowptr), shape=(rows, x.shape[0] if rows_in is None else rows_in))
        out[:, h * F:(h + 1) * F] = A @ x[:, h * F:(h + 1) * F]
    return out


def sddmm_heads(rowptr, col, a, b, heads, block=1 << 16):
    """out[e, h] = sum over j < F of a[row(e), hF+j] * b[col[e], hF+j]"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    row, col = entry_rows(rowptr), np.asarray(col, np.int64)
    F = a.shape[1] // heads
    out = np.zeros((len(col), heads))
    for s in range(0, len(col), block):
        e = slice(s, s + block)
        out[e] = np.einsum("ehf,ehf->eh", a[row[e]].reshape(-1, heads, F), b[col[e]].reshape(-1, heads, F))
    return out
