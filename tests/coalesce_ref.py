"""Numpy twins of the merge contract of include/gcn_spmm.h (gcn_csr_coalesce_count / _fill, gcn_csr_degree_f64,
gcn_csr_normalize_f32) and of the Python layer on top of it (gcn_amd/coalesce.py).  The value folds are explicit
np.float32 loops, left to right in entry order: the summation order is the contract's, not numpy's."""
import numpy as np


def _fold(vals, reduce):
    acc = np.float32(vals[0])
    if reduce == "first":
        return acc
    with np.errstate(all="ignore"):
        for v in vals[1:]:
            v = np.float32(v)
            if reduce == "sum":
                acc = np.float32(acc + v)
            elif reduce == "max":
                acc = v if (v > acc or v != v) else acc
            else:
                acc = v if (v < acc or v != v) else acc
    return acc


def coalesce_ref(rowptr, col, val, n, reduce="sum", diagonal="keep", diag_value=1.0):
    """-> (out_rowptr int32 [m + 1], out_col int32, out_val fp32 or None, out_first int32, seg int32 [nnz]).  A run is a
    maximal stretch of consecutive entries of one row with the same column (sorted or not); val None: a pattern"""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    m = len(rowptr) - 1
    dv = np.float32(diag_value)
    out_len = np.zeros(m, np.int64)
    out_col, out_val, out_first = [], [], []
    seg = np.full(len(col), -1, np.int32)
    for r in range(m):
        b, e = int(rowptr[r]), int(rowptr[r + 1])
        has_diag = r < n
        c_row = col[b:e]
        head = np.ones(e - b, bool)
        head[1:] = c_row[1:] != c_row[:-1]
        starts = np.flatnonzero(head) + b
        ends = np.append(starts[1:], e)
        present = has_diag and bool(np.any(c_row == r))
        entries = []                                    # (column, value, first entry, run end)
        for h, k in zip(starts, ends):
            c = int(col[h])
            on_diag = has_diag and c == r
            if diagonal == "drop" and on_diag:
                continue                                # (seg stays -1)
            v = None
            if val is not None:
                v = _fold(val[h:k], reduce)
                if diagonal == "add" and on_diag:
                    with np.errstate(all="ignore"):
                        v = np.float32(v + dv)
            entries.append((c, v, int(h), int(k)))
        if diagonal in ("fill", "add") and has_diag and not present:
            pos = sum(1 for c, _, _, _ in entries if c < r)              # the heads left of the diagonal
            entries.insert(pos, (r, dv if val is not None else None, -1, -1))
        base = len(out_col)
        for j, (c, v, h, k) in enumerate(entries):
            out_col.append(c)
            out_val.append(v)
            out_first.append(h)
            if h >= 0:
                seg[h:k] = base + j
        out_len[r] = len(entries)
    out_rowptr = np.zeros(m + 1, np.int32)
    out_rowptr[1:] = np.cumsum(out_len)
    return (out_rowptr, np.asarray(out_col, np.int32), np.asarray(out_val, np.float32) if val is not None else None,
            np.asarray(out_first, np.int32), seg)


def sorted_csr_ref(rows, cols, m):
    """(rowptr int32 [m + 1], eid): the column-sorted CSR of an edge list, repeated pairs in input order"""
    eid = np.lexsort((cols, rows))
    rowptr = np.zeros(m + 1, np.int32)
    rowptr[1:] = np.cumsum(np.bincount(np.asarray(rows, np.int64), minlength=m))
    return rowptr, eid


def with_mirrors_ref(rows, cols, vals):
    """the edges, then the mirror of every edge off the diagonal, in edge order"""
    off = np.flatnonzero(rows != cols)
    return (np.concatenate([rows, cols[off]]), np.concatenate([cols, rows[off]]),
            np.concatenate([vals, vals[off]]) if vals is not None else None)


def symmetrize_ref(rowptr, col, val, reduce="max"):
    """A ∪ Aᵀ of a square CSR -> (rowptr, col, val)"""
    m = len(rowptr) - 1
    rows = np.repeat(np.arange(m), np.diff(rowptr))
    r2, c2, v2 = with_mirrors_ref(rows, np.asarray(col, np.int64), val)
    rp, eid = sorted_csr_ref(r2, c2, m)
    return coalesce_ref(rp, c2[eid], v2[eid], m, reduce)[:3]


def degree_ref(rowptr, val):
    """fp64 row sums (row lengths for a pattern)"""
    if val is None:
        return np.diff(rowptr).astype(np.float64)
    return np.array([np.sum(val[b:e].astype(np.float64)) for b, e in zip(rowptr[:-1], rowptr[1:])], np.float64).reshape(-1)


def normalize_ref(rowptr, col, val, deg, mode="sym"):
    """the scaled values in fp64 (not yet rounded): s_r v s_c or v t_r, a zero degree scales by zero"""
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    v = np.ones(len(col)) if val is None else val.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if mode == "sym":
            s = np.where(deg == 0, 0.0, 1.0 / np.sqrt(deg))
            return s[rows] * v * s[col]
        t = np.where(deg == 0, 0.0, 1.0 / deg)
        return v * t[rows]


def gcn_adjacency_ref(rows, cols, n, values=None, symmetrize=True, reduce="max", self_loops="fill", norm="sym"):
    """the pipeline of gcn_amd.gcn_adjacency -> (rowptr, col, val fp32)"""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    vals = np.ones(len(rows), np.float32) if values is None else np.asarray(values, np.float32)
    if symmetrize:
        rows, cols, vals = with_mirrors_ref(rows, cols, vals)
    rp, eid = sorted_csr_ref(rows, cols, n)
    orp, oci, ova, _, _ = coalesce_ref(rp, cols[eid], vals[eid], n, reduce, self_loops, 1.0)
    if norm is not None:
        ova = normalize_ref(orp, oci, ova, degree_ref(orp, ova), norm).astype(np.float32)
    return orp, oci, ova


def within_one_ulp(got, ref64):
    """got (fp32) is within one fp32 ulp of the fp32 rounding of ref64"""
    want = np.asarray(ref64, np.float64).astype(np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)
