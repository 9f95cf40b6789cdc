"""Sparse x sparse products on the device, and the hypergraph Laplacian built from one.

    c = gcn_amd.spgemm(a, b)                               # C = A · B, both CsrAdjacency; rows of C ascend by column
    g = gcn_amd.hypergraph_laplacian(h)                    # G = Dv^-1/2 H W De^-1 Hᵀ Dv^-1/2 from an incidence matrix H

The primitive is an exact contract written out in include/gcn_spmm.h (``gcn_spgemm_count_csr`` / ``_fill_csr``) and runs on
gcn_amd/csrc/spgemm.hip; tests/spgemm_ref.py is its numpy twin.  There is no CPU path: CPU operands raise.
"""
import ctypes

import torch

from . import _lib
from .coalesce import _check_adj, coalesce_csr
from .construct import transpose_csr
from .spmm import CsrAdjacency, _ptr, _stream_ptr


def _ws_bytes(lib, m, n):
    out = ctypes.c_size_t(0)
    _lib.check(lib.gcn_spgemm_ws_bytes(m, n, ctypes.byref(out)), "gcn_spgemm_ws_bytes")
    return int(out.value)


def _spgemm(a, b):
    """(out_rowptr int32 [m + 1], out_col int32, out_val fp32) of a · b for operands on one device, b holding every column
    once per row: count, an int64 scan, ONE READ OF THE TOTAL (the output has to be allocated), fill"""
    dev = a.device
    m, p, n = a.m, a.n, b.n
    lib = _lib.load()
    out_len = torch.zeros(m, dtype=torch.int32, device=dev)
    ws = None
    if m > 0 and a.nnz > 0 and b.nnz > 0 and n > 0:
        ws = torch.empty(_ws_bytes(lib, m, n), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            st = lib.gcn_spgemm_count_csr(_ptr(a.rowptr), _ptr(a.col), m, p, a.nnz, _ptr(b.rowptr), _ptr(b.col), n, b.nnz,
                                          _ptr(out_len), _ptr(ws), ws.numel(), _stream_ptr(dev))
        _lib.check(st, "gcn_spgemm_count_csr")
    scan = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    scan[1:] = out_len.cumsum(0, dtype=torch.int64)
    total = int(scan[-1])                                  # the one synchronisation
    if total >= 2 ** 31:
        raise ValueError(f"spgemm: the product holds {total} entries; it must hold fewer than 2^31 (row-partition a first)")
    out_rowptr = scan.to(torch.int32)
    out_col = torch.empty(total, dtype=torch.int32, device=dev)
    out_val = torch.empty(total, dtype=torch.float32, device=dev)
    if total > 0:
        with torch.cuda.device(dev):
            st = lib.gcn_spgemm_fill_csr(_ptr(a.rowptr), _ptr(a.col), _ptr(a.val), m, p, a.nnz, _ptr(b.rowptr), _ptr(b.col),
                                         _ptr(b.val), n, b.nnz, _ptr(out_rowptr), _ptr(out_col), _ptr(out_val), _ptr(ws),
                                         ws.numel(), _stream_ptr(dev))
        _lib.check(st, "gcn_spgemm_fill_csr")
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
    the values of ``a`` or ``b``.
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
        with torch.cuda.device(adj.device):
            st = _lib.load().gcn_csr_degree_f64(_ptr(adj.rowptr), _ptr(val), adj.m, adj.nnz, _ptr(deg), _stream_ptr(adj.device))
        _lib.check(st, "gcn_csr_degree_f64")
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
    Not differentiable.  Two host synchronisations (the entries of the merged H, the entries of G): not capturable.
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
