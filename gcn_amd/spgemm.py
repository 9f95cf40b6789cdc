"""Sparse x sparse products on the device, and the hypergraph Laplacian built from one.

    c = gcn_amd.spgemm(a, b)                               # C = A · B, both CsrAdjacency; rows of C ascend by column
    g = gcn_amd.hypergraph_laplacian(h)                    # G = Dv^-1/2 H W De^-1 Hᵀ Dv^-1/2 from an incidence matrix H
    P = gcn_amd.SparseProduct(a, b); v = P.values(av, bv)  # the same product with a fixed pattern: refreshed in place, with gradients
    L = gcn_amd.HypergraphLaplacian(h); v = L.values(w)    # the same Laplacian with a fixed pattern, differentiable in w

The primitive is an exact contract written out in include/gcn_spmm.h (``gcn_spgemm_count_csr`` / ``_fill_csr``) and runs on
gcn_amd/csrc/spgemm.hip; tests/spgemm_ref.py is its numpy twin.  What flows back through it, and what refreshes it, is the
product sampled on a pattern (``gcn_csr_sampled_dot_f32``, gcn_amd/csrc/sampled_dot.hip, twin tests/sampled_dot_ref.py).  There
is no CPU path: CPU operands raise.
"""
import ctypes

import torch

from . import _lib
from .coalesce import _check_adj, _entry_rows, coalesce_csr
from .construct import transpose_csr
from ._lib import call
from .spmm import CsrAdjacency


def _ws_bytes(m, n):
    out = ctypes.c_size_t(0)
    call("gcn_spgemm_ws_bytes", m, n, ctypes.byref(out))
    return int(out.value)


def _spgemm(a, b, bad=None, refusal=None):
    """(out_rowptr int32 [m + 1], out_col int32, out_val fp32) of a · b for operands on one device, b holding every column
    once per row: count, an int64 scan, ONE READ OF THE TOTAL (the output has to be allocated), fill.  bad: a device count
    read together with the total (no second synchronisation); ValueError(refusal) before the fill when it is not zero"""
    dev = a.device
    m, p, n = a.m, a.n, b.n
    out_len = torch.zeros(m, dtype=torch.int32, device=dev)
    ws = None
    if m > 0 and a.nnz > 0 and b.nnz > 0 and n > 0:
        ws = torch.empty(_ws_bytes(m, n), dtype=torch.uint8, device=dev)
        call("gcn_spgemm_count_csr", a.rowptr, a.col, m, p, a.nnz, b.rowptr, b.col, n, b.nnz, out_len, ws, ws.numel(), device=dev)
    scan = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    scan[1:] = out_len.cumsum(0, dtype=torch.int64)
    if bad is None:
        total = int(scan[-1])                              # the one synchronisation
    else:
        total, nbad = torch.stack([scan[-1], bad.to(torch.int64)]).tolist()
        if nbad:
            raise ValueError(refusal)
    if total >= 2 ** 31:
        raise ValueError(f"spgemm: the product holds {total} entries; it must hold fewer than 2^31 (row-partition a first)")
    out_rowptr = scan.to(torch.int32)
    out_col = torch.empty(total, dtype=torch.int32, device=dev)
    out_val = torch.empty(total, dtype=torch.float32, device=dev)
    if total > 0:
        call("gcn_spgemm_fill_csr", a.rowptr, a.col, a.val, m, p, a.nnz, b.rowptr, b.col, b.val, n, b.nnz, out_rowptr, out_col,
             out_val, ws, ws.numel(), device=dev)
    return out_rowptr, out_col, out_val


def spgemm(a, b, assume_coalesced=False):
    """C = A · B for two CsrAdjacency operands on the device: returns a CsrAdjacency [a.m x b.n].

    Row i of the result has one entry for every column c for which an entry (i, j) of ``a`` and an entry (j, c) of ``b``
    exist — the pattern is structural: explicit zeros and sums that cancel keep their entry — and its entries ascend by
    column.  The value of an entry is the fp32 sum of its products ``fl32(a_ij * b_jc)``, added left to right with ``a``'s
    entries of row i in entry order as the outer loop and ``b``'s entries of row j as the inner loop: a pure function of the
    operands, the same bits at every call (include/gcn_spmm.h has the contract).  ``a`` may repeat (row, column) pairs.
    assume_coalesced=False: ``b`` is first merged with ``coalesce_csr(b, "sum")``, so that it holds every column once per
    row, which the kernels need.  True: ``b`` is taken as it is; its rows need not be sorted, and where it does repeat a
    column inside a row the pattern of the result is still right and the values that column feeds are unspecified.
    The result is flagged ``symmetric=False`` and takes ``a.chunk_nnz``.  It is not differentiable: nothing flows back to
    the values of ``a`` or ``b`` (``SparseProduct`` is the product that is).
    One host synchronisation (the number of entries of the result, needed to allocate it), two when ``b`` is coalesced
    first: not capturable.
    The checks, in this order: TypeError for an operand that is not a CsrAdjacency; GcnAmdError for an operand that is not on
    a device, or operands on two devices; ValueError for ``a.n != b.m``; ValueError if the result would hold 2^31 entries or
    more."""
    what = "spgemm"
    for x in (a, b):
        if not isinstance(x, CsrAdjacency):
            raise TypeError(f"{what}: a and b must be CsrAdjacency")
    for x in (a, b):
        _check_adj(x, what)
    if a.device != b.device:
        raise _lib.GcnAmdError(f"{what}: a and b must live on one device, not {a.device} and {b.device}")
    if a.n != b.m:
        raise ValueError(f"{what}: a is {a.m}x{a.n} and b is {b.m}x{b.n}: a.n must equal b.m")
    if not assume_coalesced:
        b, _ = coalesce_csr(b, "sum")
    orp, oci, ova = _spgemm(a, b)
    return CsrAdjacency(orp, oci, ova, (a.m, b.n), symmetric=False, chunk_nnz=a.chunk_nnz)


def _degree(adj, val):
    """fp64 [adj.m]: the row sums of val (fp32 [nnz]) over adj's rows, in fp64 and in a fixed order"""
    deg = torch.zeros(adj.m, dtype=torch.float64, device=adj.device)
    if adj.m > 0 and adj.nnz > 0:
        call("gcn_csr_degree_f64", adj.rowptr, val, adj.m, adj.nnz, deg, device=adj.device)
    return deg


def hypergraph_laplacian(H, edge_weight=None):
    """G = Dv^-1/2 · H · W · De^-1 · Hᵀ · Dv^-1/2 of a hypergraph, on the device: returns a CsrAdjacency [n x n] flagged
    ``symmetric=True`` whose rows ascend by column — the matrix an HGNN layer multiplies with (``torch.sparse.mm(G, x)``).

    H: the incidence matrix, a CsrAdjacency [n vertices x e hyperedges] with non-negative values (membership, or a weight
    of the vertex in the hyperedge).  Its rows are first column-sorted and repeated entries added (``coalesce_csr``).
    edge_weight: None (ones) or an fp32 device tensor [e] of non-negative hyperedge weights, the diagonal of W.
    ``Dv = H · w`` and ``De = Hᵀ · 1`` are accumulated in fp64 in a fixed order; a vertex in no hyperedge and a hyperedge
    without weight or members get the factor zero, not inf (the rule of ``normalize_csr``).  The product is split
    symmetrically: ``L = Dv^-1/2 · H · (W · De^-1)^1/2``, every value computed in fp64 as ``(h / sqrt(Dv_i)) *
    sqrt(w_e / De_e)`` and rounded to fp32 once, and ``G = spgemm(L, Lᵀ)``.  Entries (i, j) and (j, i) of G then add the
    same products over the same hyperedges in the same ascending order, so G equals its transpose bit for bit.
    Not differentiable (``HypergraphLaplacian`` is the one that is, in ``edge_weight``).  Two host synchronisations (the
    entries of the merged H, the entries of G): not capturable.
    The checks, in this order: TypeError for an H that is not a CsrAdjacency; GcnAmdError for an H that is not on a device;
    ValueError for an edge_weight that is not None or an fp32 tensor [e]; GcnAmdError for an edge_weight on another
    device."""
    what = "hypergraph_laplacian"
    _check_adj(H, what)
    if edge_weight is not None:
        if not isinstance(edge_weight, torch.Tensor) or edge_weight.dtype != torch.float32 or edge_weight.dim() != 1 \
                or edge_weight.numel() != H.n:
            raise ValueError(f"{what}: edge_weight must be None or an fp32 tensor [{H.n}]")
        if edge_weight.device != H.device:
            raise _lib.GcnAmdError(f"{what}: edge_weight must live on H's device")
    Hc, _ = coalesce_csr(H, "sum")
    Ht, eid = transpose_csr(Hc)
    col = Hc.col.long()
    h = Hc.val.double()
    if edge_weight is None:
        dv = _degree(Hc, Hc.val)
        w = None
    else:
        # h * w has at most 48 significant bits: hi + lo holds it exactly, and the two fp64 row sums add up to H · w
        w = edge_weight.detach().contiguous().double()
        hw = h * w.index_select(0, col)
        hi = hw.float()
        dv = _degree(Hc, hi) + _degree(Hc, (hw - hi.double()).float())
    de = _degree(Ht, Ht.val)
    zero = torch.zeros((), dtype=torch.float64, device=H.device)
    inv_dv = torch.where(dv == 0, zero, 1.0 / torch.sqrt(dv))
    edge = torch.where(de == 0, zero, torch.sqrt((w if w is not None else torch.ones_like(de)) / de))
    rows = torch.repeat_interleave(torch.arange(Hc.m, device=H.device), (Hc.rowptr[1:] - Hc.rowptr[:-1]).long(),
                                   output_size=Hc.nnz)
    lval = ((h * inv_dv.index_select(0, rows)) * edge.index_select(0, col)).float()
    L = CsrAdjacency(Hc.rowptr, Hc.col, lval, (Hc.m, Hc.n), symmetric=False, chunk_nnz=H.chunk_nnz)
    Lt = CsrAdjacency(Ht.rowptr, Ht.col, lval.index_select(0, eid.long()), (Hc.n, Hc.m), symmetric=False)
    orp, oci, ova = _spgemm(L, Lt)
    return CsrAdjacency(orp, oci, ova, (H.m, H.m), symmetric=True, chunk_nnz=H.chunk_nnz)


# ---- the product sampled on a pattern ----------------------------------------------------------------------------------------------
def _sampled_dot(pattern, x, xv, y, yv, x_by_col):
    """fp32 [pattern.nnz] of gcn_csr_sampled_dot_f32 for checked operands on one device; xv / yv: fp32 [nnz] or None (ones).
    No host read, no synchronisation: capturable."""
    dev = pattern.device
    out = torch.empty(pattern.nnz, dtype=torch.float32, device=dev)
    if pattern.m == 0 or pattern.nnz == 0:
        return out
    ws = torch.empty(_lib.SAMPLED_DOT_WS_BYTES, dtype=torch.uint8, device=dev)
    call("gcn_csr_sampled_dot_f32", pattern.rowptr, pattern.col, pattern.m, pattern.n, pattern.nnz,
         x.rowptr, x.col if x.nnz else None, xv if x.nnz else None, x.nnz,
         y.rowptr, y.col if y.nnz else None, yv if y.nnz else None, y.nnz,
         x.n, 1 if x_by_col else 0, out, ws, ws.numel(), device=dev)
    return out


def _operand(op):
    """(adjacency, replaces its values?, the replacement) of an operand given as adj, (adj, values) or (adj, None)"""
    if isinstance(op, tuple) and len(op) == 2:
        return op[0], True, op[1]
    return op, False, None


def _check_values(v, adj, name, what):
    if not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or v.dim() != 1 or v.numel() != adj.nnz:
        raise ValueError(f"{what}: {name} must be an fp32 tensor [{adj.nnz}], one value per entry in CSR order")
    if v.device != adj.device:
        raise _lib.GcnAmdError(f"{what}: {name} must live on the operand's device")
    return v.detach().contiguous()


def sampled_dot(pattern, x, y, x_by_col=False):
    """The product of two sparse matrices sampled on a pattern: an fp32 tensor [pattern.nnz] with, for the entry (i, j) of
    ``pattern``, the dot product of row i of ``x`` and row j of ``y`` over their common columns — the entry (i, j) of
    ``x · yᵀ``.  With ``x_by_col=True`` the roles of the entry swap: row j of ``x`` and row i of ``y``, the entry (i, j) of
    ``y · xᵀ`` with ``x``'s entries still the ones that set the order.

    The products of an entry are ``fl32(x_t * y)``, one rounding each, added left to right over ``x``'s entries of the row in
    entry order; no common column gives +0.0 (include/gcn_spmm.h has the contract: ``gcn_csr_sampled_dot_f32``).  ``y``'s
    rows must ascend strictly by column (what ``coalesce_csr`` and ``transpose_csr`` of such a matrix return): it is not
    checked, and where a row does not the entries that use it are unspecified.  ``x`` may be unsorted and repeat columns.
    ``x`` or ``y`` may be given as ``(adj, values)`` to replace the stored values by an fp32 tensor [adj.nnz], or as
    ``(adj, None)`` for a pattern (ones); only the pattern of ``pattern`` is used.
    Not differentiable (``SparseProduct`` is what wraps it with gradients).  No host synchronisation: capturable.
    The checks, in this order: TypeError for an operand that is not a CsrAdjacency; GcnAmdError for an operand that is not on
    a device, or operands on more than one; ValueError for shapes that do not fit the mode (x_by_col=False: x.m == pattern.m,
    y.m == pattern.n; True: x.m == pattern.n, y.m == pattern.m; always x.n == y.n); ValueError for replacement values that
    are not fp32 [nnz], GcnAmdError for ones on another device."""
    what = "sampled_dot"
    (xa, x_given, xv), (ya, y_given, yv) = _operand(x), _operand(y)
    for t in (pattern, xa, ya):
        if not isinstance(t, CsrAdjacency):
            raise TypeError(f"{what}: pattern, x and y must be CsrAdjacency (x and y possibly with values: (adj, values))")
    for t in (pattern, xa, ya):
        _check_adj(t, what)
    if not pattern.device == xa.device == ya.device:
        raise _lib.GcnAmdError(f"{what}: the operands must live on one device, not {pattern.device}, {xa.device} and {ya.device}")
    xm, ym = (pattern.n, pattern.m) if x_by_col else (pattern.m, pattern.n)
    if xa.m != xm or ya.m != ym or xa.n != ya.n:
        raise ValueError(f"{what}: pattern is {pattern.m}x{pattern.n}, x is {xa.m}x{xa.n} and y is {ya.m}x{ya.n}: with "
                         f"x_by_col={bool(x_by_col)} x needs {xm} rows, y needs {ym}, and both the same number of columns")
    xv = (_check_values(xv, xa, "x's values", what) if xv is not None else None) if x_given else xa.val
    yv = (_check_values(yv, ya, "y's values", what) if yv is not None else None) if y_given else ya.val
    return _sampled_dot(pattern, xa, xv, ya, yv, x_by_col)


class _SparseProductFunction(torch.autograd.Function):
    """values of C = A · B on C's fixed pattern from the two value vectors; the backward is the same kernel on A's and on B's
    pattern, each call made only when its gradient is asked for"""

    @staticmethod
    def forward(ctx, prod, a_values, b_values):
        av = prod.a.val if a_values is None else a_values.detach().contiguous()
        bv = prod.b.val if b_values is None else b_values.detach().contiguous()
        ctx.prod = prod
        ctx.save_for_backward(av, bv)
        return prod._forward(av, bv)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        av, bv = ctx.saved_tensors
        prod = ctx.prod
        grad = grad.contiguous()
        ga = prod._grad_a(bv, grad) if ctx.needs_input_grad[1] else None
        gb = prod._grad_b(av, grad) if ctx.needs_input_grad[2] else None
        return None, ga, gb


class SparseProduct:
    """C = A · B with a FIXED PATTERN: built once, its values refreshed from new operand values without a count, a scan or a
    host read, and differentiable in both value vectors.

        P = SparseProduct(a, b)
        v = P.values(a_values, b_values)                       # fp32 [P.adj.nnz], bit for bit spgemm's on those values
        y = spmm(P.adj, x, values=v)                           # gradients reach a_values, b_values and x

    Construction checks that ``b``'s rows ascend strictly by column (one device reduction, read together with the number of
    entries of C: ONE host synchronisation; ValueError otherwise — call ``coalesce_csr(b, "sum")`` first), runs spgemm's
    count and fill once, and keeps the pattern of C as ``.adj`` — a CsrAdjacency made with ``mutable_values=True`` whose own
    values are those of ``spgemm(a, b)``, flagged ``symmetric`` as given — together with the transposed patterns of A, B
    and C and their entry maps (``transpose_csr``).  ``a`` may repeat (row, column) pairs and be unsorted.  The checks come in
    spgemm's order: TypeError, GcnAmdError for the devices, ValueError for ``a.n != b.m``, then the rows of ``b``."""

    def __init__(self, a, b, symmetric=None):
        what = "SparseProduct"
        for x in (a, b):
            if not isinstance(x, CsrAdjacency):
                raise TypeError(f"{what}: a and b must be CsrAdjacency")
        for x in (a, b):
            _check_adj(x, what)
        if a.device != b.device:
            raise _lib.GcnAmdError(f"{what}: a and b must live on one device, not {a.device} and {b.device}")
        if a.n != b.m:
            raise ValueError(f"{what}: a is {a.m}x{a.n} and b is {b.m}x{b.n}: a.n must equal b.m")
        bad = torch.zeros((), dtype=torch.int64, device=b.device)
        if b.nnz > 1:
            rows = _entry_rows(b)
            bad = ((b.col[1:] <= b.col[:-1]) & (rows[1:] == rows[:-1])).sum()
        orp, oci, ova = _spgemm(a, b, bad, f"{what}: the rows of b must ascend strictly by column (sorted, every column once "
                                           "per row): call coalesce_csr(b, \"sum\") first")
        self.a, self.b = a, b
        self.adj = CsrAdjacency(orp, oci, ova, (a.m, b.n), symmetric=symmetric, chunk_nnz=a.chunk_nnz, mutable_values=True)
        (self.at, eid_a), (self.bt, eid_b), (self.ct, eid_c) = transpose_csr(a), transpose_csr(b), transpose_csr(self.adj)
        self.eid_a, self.eid_b, self.eid_c = eid_a.long(), eid_b.long(), eid_c.long()

    # (the three calls of the kernel; values are detached, contiguous fp32 tensors on the device)
    def _forward(self, av, bv):
        return _sampled_dot(self.adj, self.a, av, self.bt, bv.index_select(0, self.eid_b), False)

    def _grad_a(self, bv, grad):
        return _sampled_dot(self.a, self.b, bv, self.adj, grad, True)

    def _grad_b(self, av, grad):
        return _sampled_dot(self.b, self.at, av.index_select(0, self.eid_a), self.ct, grad.index_select(0, self.eid_c), False)

    def values(self, a_values=None, b_values=None):
        """fp32 [adj.nnz]: the values of C for operands carrying ``a_values`` (fp32 [a.nnz]) and ``b_values`` (fp32 [b.nnz]),
        in the entry order of ``.adj`` — the product sampled on C's pattern with X = A and Y = Bᵀ, bit-identical to
        ``spgemm`` on operands carrying those values.  None: the operand's own values, and no gradient for it.
        No host synchronisation: capturable.  Differentiable (once) in both vectors: grad_a is the kernel on A's pattern with
        X = (B, b_values), Y = (C, grad) and ``x_by_col``; grad_b is the kernel on B's pattern with X = Aᵀ, Y = Cᵀ; each
        is computed only when its vector requires a gradient.  Every call gives the same bits, the backward included.  The
        result feeds ``spmm(P.adj, x, values=...)``; it is not written into ``.adj`` by this call.
        ValueError for values that are not fp32 [nnz]; GcnAmdError for values on another device."""
        what = "SparseProduct.values"
        for v, adj, name in ((a_values, self.a, "a_values"), (b_values, self.b, "b_values")):
            if v is not None:
                _check_values(v, adj, name, what)
        return _SparseProductFunction.apply(self, a_values, b_values)


def _split_sum(adj, v, parts=3):
    """fp64 [adj.m]: the row sums over adj's rows of fp64 values given per entry, by gcn_csr_degree_f64 on an exact split:
    v = hi + mid + lo with three fp32 terms (72 bits hold the 53 of an fp64 inside fp32's range), each summed in fp64 in
    the kernel's fixed order — the same bits at every call, unlike index_add_"""
    total = torch.zeros(adj.m, dtype=torch.float64, device=adj.device)
    for _ in range(parts):
        part = v.float()
        total = total + _degree(adj, part)
        v = v - part.double()
    return total


class _LaplacianFunction(torch.autograd.Function):
    """values of G from the hyperedge weights; the backward written out (see HypergraphLaplacian.values)"""

    @staticmethod
    def forward(ctx, lap, edge_weight):
        w = edge_weight.detach().contiguous().double()
        lval, inv_dv, edge = lap._factor(w)
        ctx.lap = lap
        ctx.save_for_backward(w, lval, inv_dv, edge)
        return lap.product._forward(lval, lval.index_select(0, lap.eid))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        if not ctx.needs_input_grad[1]:
            return None, None
        w, lval, inv_dv, edge = ctx.saved_tensors
        lap = ctx.lap
        P, rows, col, eid, h = lap.product, lap.rows, lap.col, lap.eid, lap.h
        grad = grad.contiguous()
        lt = lval.index_select(0, eid)
        # the gradient of l (H's entry order): the product's two operand gradients, the second carried back through the
        # transpose's entry map (a permutation: every element is written once)
        ga = P._grad_a(lt, grad)
        gb = P._grad_b(lval, grad)
        gl = ga.double() + torch.empty_like(gb).index_copy_(0, eid, gb).double()
        zero = torch.zeros((), dtype=torch.float64, device=grad.device)
        s = inv_dv.index_select(0, rows)
        # through r_e = sqrt(w_e / De_e):  sum_i gl_ie h_ie s_i / (2 sqrt(w_e De_e))
        wd = w * lap.de
        half_inv = torch.where(wd == 0, zero, 0.5 / torch.sqrt(wd))
        t1 = _split_sum(lap.Ht, (gl * h * s).index_select(0, eid)) * half_inv
        # through s_i = Dv_i^-1/2, Dv_i = sum_e h_ie w_e:  -1/2 sum_i h_ie Dv_i^-3/2 (sum_e' gl_ie' h_ie' r_e')
        inner = _split_sum(lap.Hc, gl * h * edge.index_select(0, col))
        per_vertex = inv_dv * inv_dv * inv_dv * inner
        t2 = _split_sum(lap.Ht, (h * per_vertex.index_select(0, rows)).index_select(0, eid))
        gw = torch.where(wd == 0, zero, t1 - 0.5 * t2)
        return None, gw.float()


class HypergraphLaplacian:
    """``hypergraph_laplacian`` with a FIXED PATTERN: G = Dv^-1/2 · H · W · De^-1 · Hᵀ · Dv^-1/2 whose values follow the
    hyperedge weights W without a host synchronisation and with a gradient — learnable hyperedge weights.

        L = HypergraphLaplacian(H)
        y = spmm(L.adj, x, values=L.values(w))                 # gradients reach w and x

    Construction does once what ``hypergraph_laplacian`` does up to the product — H merged (``coalesce_csr``) and transposed,
    ``De = Hᵀ · 1`` in fp64, the row and the column of every entry — and builds ``SparseProduct(L, Lᵀ)`` for unit weights:
    two host synchronisations (the entries of the merged H, the entries of G).  ``.adj`` is G's adjacency, made with
    ``mutable_values=True`` and flagged ``symmetric=True``; its own values are those of ``hypergraph_laplacian(H)``.
    TypeError for an H that is not a CsrAdjacency; GcnAmdError for an H that is not on a device."""

    def __init__(self, H):
        what = "HypergraphLaplacian"
        _check_adj(H, what)
        self.Hc, _ = coalesce_csr(H, "sum")
        self.Ht, eid = transpose_csr(self.Hc)
        self.eid = eid.long()
        self.col = self.Hc.col.long()
        self.rows = _entry_rows(self.Hc).long()
        self.h = self.Hc.val.double()
        self.de = _degree(self.Ht, self.Ht.val)
        self.m, self.n_edges = self.Hc.m, self.Hc.n
        lval, _, _ = self._factor(torch.ones(self.n_edges, dtype=torch.float64, device=H.device))
        L = CsrAdjacency(self.Hc.rowptr, self.Hc.col, lval, (self.Hc.m, self.Hc.n), symmetric=False, chunk_nnz=H.chunk_nnz)
        Lt = CsrAdjacency(self.Ht.rowptr, self.Ht.col, lval.index_select(0, self.eid), (self.Hc.n, self.Hc.m), symmetric=False)
        self.product = SparseProduct(L, Lt, symmetric=True)
        self.adj = self.product.adj

    def _factor(self, w):
        """(values of L fp32 [nnz_H], Dv^-1/2 fp64 [n], sqrt(w / De) fp64 [e]) for weights w fp64 [e]: hypergraph_laplacian's
        own arithmetic, operation for operation"""
        Hc, h = self.Hc, self.h
        hw = h * w.index_select(0, self.col)
        hi = hw.float()                                    # (hi + lo holds h * w exactly: at most 48 significant bits)
        dv = _degree(Hc, hi) + _degree(Hc, (hw - hi.double()).float())
        zero = torch.zeros((), dtype=torch.float64, device=Hc.device)
        inv_dv = torch.where(dv == 0, zero, 1.0 / torch.sqrt(dv))
        edge = torch.where(self.de == 0, zero, torch.sqrt(w / self.de))
        lval = ((h * inv_dv.index_select(0, self.rows)) * edge.index_select(0, self.col)).float()
        return lval, inv_dv, edge

    def values(self, edge_weight):
        """fp32 [adj.nnz]: the values of G for the hyperedge weights ``edge_weight`` (an fp32 device tensor [e],
        non-negative: negative weights are the caller's error, as in ``hypergraph_laplacian``), bit-identical to
        ``hypergraph_laplacian(H, edge_weight).val`` on the identical pattern.  No host synchronisation.
        Differentiable (once) in ``edge_weight``, the backward written out: with s_i = Dv_i^-1/2, r_e = sqrt(w_e / De_e) and
        l_ie = h_ie · s_i · r_e, the gradient of l is the sum of the product's two operand gradients, and
        d/dw_e = sum_i gl_ie h_ie s_i / (2 sqrt(w_e De_e)) - 1/2 sum_i h_ie Dv_i^-3/2 (sum_e' gl_ie' h_ie' r_e'),
        all of it in fp64 and every sum a row sum over H or Hᵀ in a fixed order: the same bits at every call.  A vertex in
        no hyperedge and a hyperedge without members or of weight zero take no part and receive exactly 0 — the forward's
        inf -> 0 rule (at w_e = 0 the one-sided derivative of sqrt is infinite; the hyperedge counts as absent).
        ValueError for an edge_weight that is not an fp32 tensor [e]; GcnAmdError for one on another device."""
        what = "HypergraphLaplacian.values"
        if not isinstance(edge_weight, torch.Tensor) or edge_weight.dtype != torch.float32 or edge_weight.dim() != 1 \
                or edge_weight.numel() != self.n_edges:
            raise ValueError(f"{what}: edge_weight must be an fp32 tensor [{self.n_edges}]")
        if edge_weight.device != self.Hc.device:
            raise _lib.GcnAmdError(f"{what}: edge_weight must live on H's device")
        return _LaplacianFunction.apply(self, edge_weight)
