"""Merging repeated entries on the device, and what the GCN adjacency needs on top of the merge: the union with the
transpose, self-loops, and the normalisation — an edge list becomes Â without leaving the device.

    merged, seg = gcn_amd.coalesce_csr(adj, reduce="sum")            # one entry per distinct (row, column) pair
    sym = gcn_amd.symmetrize(adj)                                    # A ∪ Aᵀ
    a_hat = gcn_amd.normalize_csr(adj, "sym")                        # D^-1/2 A D^-1/2 on the stored entries
    a_hat = gcn_amd.gcn_adjacency(rows, cols, n)                     # edge list -> D^-1/2 (A ∪ Aᵀ ∪ I) D^-1/2

The primitive is an exact contract written out in include/gcn_spmm.h (``gcn_csr_coalesce_count`` / ``_fill``,
``gcn_csr_degree_f64``, ``gcn_csr_normalize_f32``) and runs on gcn_amd/csrc/coalesce.hip; tests/coalesce_ref.py is its
numpy twin.  The column order the merge needs comes from the two stable bucketings of construct.py.  There is no CPU path:
CPU tensors raise.
"""
import torch

from . import _lib
from .construct import _bucket, _check_ids, _check_size, _transpose_arrays
from ._lib import call
from .spmm import CsrAdjacency

REDUCE = {"sum": _lib.COALESCE_SUM, "max": _lib.COALESCE_MAX, "min": _lib.COALESCE_MIN, "first": _lib.COALESCE_FIRST}
DIAGONAL = {"keep": _lib.DIAG_KEEP, "drop": _lib.DIAG_DROP, "fill": _lib.DIAG_FILL, "add": _lib.DIAG_ADD}
NORM = {"sym": _lib.NORM_SYM, "row": _lib.NORM_ROW}


def _check_choice(v, name, table, what):
    if not isinstance(v, str) or v not in table:
        raise ValueError(f"{what}: {name} must be one of {', '.join(repr(k) for k in table)}, not {v!r}")


def _check_adj(adj, what):
    if not isinstance(adj, CsrAdjacency):
        raise TypeError(f"{what}: adj must be a CsrAdjacency")
    if adj.device.type != "cuda":
        raise _lib.GcnAmdError(f"{what}: the adjacency must live on a CUDA/HIP device (no CPU path in gcn_amd)")


def _coalesce(rowptr, col, val, m, n, reduce, diagonal, diag_value, want_seg=True):
    """(out_rowptr int32 [m + 1], out_col int32, out_val fp32 or None, seg int32 [nnz] or None) for contiguous device
    arrays: count, scan, ONE READ OF THE TOTAL (the output has to be allocated), fill.  val None: a pattern"""
    dev = rowptr.device
    nnz = int(col.numel())
    if nnz + min(m, n) >= 2 ** 31:
        raise ValueError("coalesce: the merged matrix must hold fewer than 2^31 entries")
    ws = torch.empty(_lib.COALESCE_WS_BYTES, dtype=torch.uint8, device=dev)
    out_rowptr = torch.zeros(m + 1, dtype=torch.int32, device=dev)
    if m > 0:
        call("gcn_csr_coalesce_count", rowptr, col if nnz else None, m, n, nnz, diagonal, out_rowptr[1:], ws, ws.numel(),
             device=dev)
        out_rowptr.cumsum_(0)                              # (the total is below 2^31: int32 holds every partial sum)
    total = int(out_rowptr[-1])                            # the one synchronisation
    out_col = torch.empty(total, dtype=torch.int32, device=dev)
    out_val = torch.empty(total, dtype=torch.float32, device=dev) if val is not None else None
    seg = torch.full((nnz,), -1, dtype=torch.int32, device=dev) if want_seg else None
    if total > 0:
        call("gcn_csr_coalesce_fill", rowptr, col if nnz else None, val if nnz else None, m, n, nnz, reduce, diagonal,
             float(diag_value), out_rowptr, out_col, out_val if nnz else None, None, seg if nnz else None, ws, ws.numel(),
             device=dev)
        if val is not None and nnz == 0:                   # (only inserted diagonals: no input values to hand to the call)
            out_val.fill_(float(diag_value))
    return out_rowptr, out_col, out_val, seg


def _sorted_csr(r32, c32, m, n):
    """(rowptr int32 [m + 1], eid int32 [E]) of the column-sorted CSR of an edge list whose ids are known to be in range:
    two stable bucketings, by column and then by row (np.lexsort((cols, rows)))"""
    _, by_col = _bucket(c32, n)                            # LSD: the minor key first
    rowptr, by_row = _bucket(r32.index_select(0, by_col), m)
    return rowptr, by_col.index_select(0, by_row)


def coalesce_csr(adj, reduce="sum", diagonal="keep", diag_value=1.0, assume_sorted=False):
    """Merge the repeated (row, column) entries of a CsrAdjacency on the device: returns ``(CsrAdjacency, seg int32
    [adj.nnz])``; ``seg[e]`` is the entry of the result that entry ``e`` of ``adj`` went into, or -1 when it was dropped.

    reduce: the value of a merged pair, folded in fp32 over its entries in ``adj``'s entry order — "sum", "max", "min" (a
    NaN propagates, as in ``np.maximum``) or "first".
    diagonal (rows r < n): "keep"; "drop": no (r, r) in the result; "fill": a missing (r, r) is inserted with
    ``diag_value``, an existing one stays as merged; "add": the same insertion, and an existing one becomes merged +
    ``diag_value``.
    assume_sorted=False: the rows are first column-sorted — two stable bucketings, by column and then by row, what
    ``csr_from_edges(sort_columns=True)`` does — so every distinct pair is merged and every row of the result ascends by
    column; ``seg`` is given in ``adj``'s own entry order.  True: ``adj``'s rows are taken as they are and only ADJACENT
    equal columns merge — a full merge exactly when the rows are column-sorted.
    The result inherits ``adj.symmetric`` for "sum", "max" and "min" and is flagged ``symmetric=False`` for "first" (the
    first of (i, j) and the first of (j, i) need not agree).  It is not differentiable; for merged learnable weights ``seg``
    is what the gradient needs (``grad_in = grad_out[seg]`` for "sum").
    One host synchronisation (the number of entries of the result, needed to allocate it): not capturable.
    ValueError for a bad reduce, diagonal or diag_value, TypeError for a non-CsrAdjacency, GcnAmdError for an adjacency that
    is not on a device."""
    what = "coalesce_csr"
    _check_choice(reduce, "reduce", REDUCE, what)
    _check_choice(diagonal, "diagonal", DIAGONAL, what)
    if isinstance(diag_value, bool) or not isinstance(diag_value, (int, float)):
        raise ValueError(f"{what}: diag_value must be a number, not {diag_value!r}")
    _check_adj(adj, what)
    rowptr, col, val, eid = adj.rowptr, adj.col, adj.val, None
    if not assume_sorted and adj.nnz > 0:
        _, trow, _, by_col = _transpose_arrays(adj, with_values=False)     # (trow: the row of entry by_col[t])
        rowptr, by_row = _bucket(trow, adj.m)
        eid = by_col.index_select(0, by_row)
        col, val = col.index_select(0, eid), val.index_select(0, eid)
    orp, oci, ova, seg = _coalesce(rowptr, col, val, adj.m, adj.n, REDUCE[reduce], DIAGONAL[diagonal], diag_value)
    if eid is not None:
        seg = torch.empty_like(seg).index_copy_(0, eid.long(), seg)        # (eid is a permutation: every element is written)
    symmetric = adj.symmetric if reduce != "first" else False
    return CsrAdjacency(orp, oci, ova, (adj.m, adj.n), symmetric=symmetric, chunk_nnz=adj.chunk_nnz), seg


def _with_mirrors(r32, c32, vals):
    """the edges plus the mirror (c, r) of every edge with r != c, appended in edge order.  One host synchronisation (the
    number of mirrors)"""
    off = torch.nonzero(r32 != c32).squeeze(1)
    rows = torch.cat([r32, c32.index_select(0, off)])
    cols = torch.cat([c32, r32.index_select(0, off)])
    return rows, cols, (torch.cat([vals, vals.index_select(0, off)]) if vals is not None else None)


def _entry_rows(adj):
    """the row of every entry, int32 [nnz] (no synchronisation: the length is adj.nnz)"""
    lens = adj.rowptr[1:] - adj.rowptr[:-1]
    return torch.repeat_interleave(torch.arange(adj.m, dtype=torch.int32, device=adj.device), lens.long(), output_size=adj.nnz)


def symmetrize(adj, reduce="max"):
    """A ∪ Aᵀ of a square CsrAdjacency on the device: its entries and the mirror (j, i) of every entry with i != j (a
    diagonal entry is not mirrored), column-sorted by two stable bucketings and merged by one coalesce.

    reduce: "sum" (A + Aᵀ off the diagonal, A on it), "max" (``A.maximum(A.T)`` for stored entries) or "min"; repeated
    entries of ``adj`` fall under the same rule, an entry's own repeats first and in order, the mirrors after them.  The
    result is flagged ``symmetric=True`` and its rows ascend by column.  Not differentiable.
    Two host synchronisations (the number of mirrors, the number of entries of the result): not capturable.
    ValueError for a bad reduce or a matrix that is not square, TypeError for a non-CsrAdjacency, GcnAmdError for an
    adjacency that is not on a device."""
    what = "symmetrize"
    _check_choice(reduce, "reduce", {k: v for k, v in REDUCE.items() if k != "first"}, what)
    _check_adj(adj, what)
    if adj.m != adj.n:
        raise ValueError(f"{what}: the matrix must be square, not {adj.m}x{adj.n}")
    rows, cols, vals = _with_mirrors(_entry_rows(adj), adj.col, adj.val)
    rowptr, eid = _sorted_csr(rows, cols, adj.m, adj.n)
    orp, oci, ova, _ = _coalesce(rowptr, cols.index_select(0, eid), vals.index_select(0, eid), adj.m, adj.n, REDUCE[reduce],
                                 _lib.DIAG_KEEP, 0.0, want_seg=False)
    return CsrAdjacency(orp, oci, ova, (adj.m, adj.n), symmetric=True, chunk_nnz=adj.chunk_nnz)


def _normalized_values(rowptr, col, val, m, n, mode):
    """fp32 [nnz]: the degrees (fp64 row sums of val, row lengths for val None) and the scaled values, two calls"""
    dev = rowptr.device
    nnz = int(col.numel())
    deg = torch.zeros(m, dtype=torch.float64, device=dev)
    out = torch.empty(nnz, dtype=torch.float32, device=dev)
    if m > 0 and nnz > 0:
        call("gcn_csr_degree_f64", rowptr, val, m, nnz, deg, device=dev)
        call("gcn_csr_normalize_f32", rowptr, col, val, m, n, nnz, deg, mode, out, device=dev)
    return out


def normalize_csr(adj, norm="sym"):
    """The same pattern with normalised values, on the device: "sym": ``D^-1/2 A D^-1/2`` (a square matrix), "row":
    ``D^-1 A``, D the row sums of the stored values accumulated in fp64; every value is computed in fp64 and rounded to
    fp32 once, and a row (or column) whose sum is zero is scaled by zero, not by inf.  Repeated entries are scaled one by
    one (they still add); nothing is merged and no self-loop is added: ``coalesce_csr`` does that.
    The result shares ``adj``'s rowptr and col; it inherits ``adj.symmetric`` for "sym" and is flagged ``symmetric=False``
    for "row".  Not differentiable.  No host synchronisation.
    ValueError for a bad norm or "sym" on a matrix that is not square, TypeError for a non-CsrAdjacency, GcnAmdError for an
    adjacency that is not on a device."""
    what = "normalize_csr"
    _check_choice(norm, "norm", NORM, what)
    _check_adj(adj, what)
    if norm == "sym" and adj.m != adj.n:
        raise ValueError(f"{what}: norm=\"sym\" needs a square matrix, not {adj.m}x{adj.n}")
    val = _normalized_values(adj.rowptr, adj.col, adj.val, adj.m, adj.n, NORM[norm])
    return CsrAdjacency(adj.rowptr, adj.col, val, (adj.m, adj.n), symmetric=adj.symmetric if norm == "sym" else False,
                        chunk_nnz=adj.chunk_nnz)


def gcn_adjacency(rows, cols, n, values=None, symmetrize=True, reduce="max", self_loops="fill", norm="sym"):
    """Â from an edge list, entirely on the device: returns a CsrAdjacency [n x n] with column-sorted rows.

    The steps: the edges (rows[i], cols[i]) with ``values`` (None: ones), plus with ``symmetrize`` the mirror of every edge
    off the diagonal; two stable bucketings into a column-sorted CSR; one merge, in which repeated pairs (and an edge with its
    mirror) combine by ``reduce`` ("sum", "max" or "min") and the diagonal is treated by ``self_loops`` with the value 1 —
    "fill": a vertex without a self-loop gets one, "add": every vertex gets 1 more on its diagonal, "keep", "drop"; then
    ``norm``: "sym" ``D^-1/2 · D^-1/2``, "row" ``D^-1 ·``, None: the merged values.
    The defaults are the usual GCN preprocessing of an unweighted graph: the union with the transpose, one unit self-loop
    per vertex, the symmetric normalisation in fp64 rounded to fp32 once.
    rows, cols: 1-D int32 or int64 device tensors of equal length E, ids in [0, n), 2 E + n < 2^31.  values: None or an
    fp32 device tensor [E].  The result is flagged ``symmetric=True`` with ``symmetrize`` unless norm="row", else False.
    The result is NOT DIFFERENTIABLE: nothing flows back to ``values`` (``coalesce_csr`` returns the ``seg`` map a caller
    needs for that).  Three host synchronisations (the range of the ids, the number of mirrors, the number of entries of the
    result): not capturable.
    ValueError for a bad dtype, shape, length, n, values, id out of range or option, GcnAmdError for CPU tensors."""
    what = "gcn_adjacency"
    _check_ids(rows, "rows", what)
    _check_ids(cols, "cols", what)
    if rows.numel() != cols.numel():
        raise ValueError(f"{what}: rows and cols must have the same length, not {rows.numel()} and {cols.numel()}")
    _check_size(n, "n", what)
    E = int(rows.numel())
    if values is not None:
        if not isinstance(values, torch.Tensor) or values.dtype != torch.float32 or values.dim() != 1 or values.numel() != E:
            raise ValueError(f"{what}: values must be None or an fp32 tensor [E]")
    _check_choice(reduce, "reduce", {k: v for k, v in REDUCE.items() if k != "first"}, what)
    _check_choice(self_loops, "self_loops", DIAGONAL, what)
    if norm is not None:
        _check_choice(norm, "norm", NORM, what)
    if 2 * E + n >= 2 ** 31:
        raise ValueError(f"{what}: 2 E + n must stay below 2^31")
    if not (rows.is_cuda and cols.is_cuda and (values is None or values.is_cuda)):
        raise _lib.GcnAmdError(f"{what}: rows, cols and values must be CUDA/HIP tensors (no CPU path in gcn_amd)")
    dev = rows.device
    if E > 0:
        lo, hi = torch.stack([torch.minimum(rows.min(), cols.min()), torch.maximum(rows.max(), cols.max())]).tolist()
        if lo < 0 or hi >= n:
            raise ValueError(f"{what}: rows and cols must lie in [0, {n}), found {lo if lo < 0 else hi}")
    r32, c32 = rows.to(torch.int32).contiguous(), cols.to(torch.int32).contiguous()
    # without values, "max" / "min" of ones and a unit diagonal leave every value 1: the merge runs on the pattern alone
    pattern = values is None and reduce != "sum" and self_loops != "add"
    vals = None if pattern else (values if values is not None else torch.ones(E, dtype=torch.float32, device=dev))
    if symmetrize:
        r32, c32, vals = _with_mirrors(r32, c32, vals)
    rowptr, eid = _sorted_csr(r32, c32, n, n)
    orp, oci, ova, _ = _coalesce(rowptr, c32.index_select(0, eid), None if pattern else vals.index_select(0, eid), n, n,
                                 REDUCE[reduce], DIAGONAL[self_loops], 1.0, want_seg=False)
    if norm is not None:
        ova = _normalized_values(orp, oci, ova, n, n, NORM[norm])
    elif pattern:
        ova = torch.ones(oci.numel(), dtype=torch.float32, device=dev)
    return CsrAdjacency(orp, oci, ova, (n, n), symmetric=bool(symmetrize) and norm != "row")
