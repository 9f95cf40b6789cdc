"""Relation-typed aggregation: the message passing of relational graph convolutions with basis decomposition (R-GCN;
PyG's ``RGCNConv``, DGL's ``RelGraphConv``) from ONE gather per stored entry.

    types = gcn_amd.EdgeTypes(adj, etype, num_relations)           # once per graph (or per sampled block)
    y = gcn_amd.relation_aggregate(types, x, coeff, values)        # [m, B k]: y[r, b k + j] = sum_e coeff[etype[e], b] values[e] x[col[e], j]
    out = y @ V.view(B * k, out_dim)                               # one dense product for all relations
    y = gcn_amd.relation_aggregate(types, x)                       # typed mode, [m, R k]: plane t sums the entries of type t

Runs on gcn_amd/csrc/relational.hip (fp32): plan-free kernels that only enqueue, so after one eager call — which
allocates the scratch, the transposed pattern and, for a coefficient gradient, the relation-major view — everything here
runs inside a captured step.  No atomics; two calls give the same bits.  There is no CPU path: CPU tensors raise.
"""
import torch

from . import _lib
from ._lib import call
from .attention import _segment_sum_raw
from .construct import bucket_by_key
from .segment_mm import _check_fp32, _forward_raw, _wgrad_raw
from .spmm import CsrAdjacency

_CHUNK = 4096                # entries per workspace partial: gcn_relation_aggregate_ws_bytes in include/gcn_spmm.h


class EdgeTypes:
    """The relation type of every stored entry of ``adj``, and what the gradients need of it, built once per graph.

    etype: [adj.nnz] int32 or int64 device tensor in the entry order of ``adj``; a type outside [0, num_relations) masks
    its entry (it contributes nothing, forward and backward), so -1 is a mask.  For a sampled block:
    ``EdgeTypes(block.adj, etype[block.eid.long()], R)``.
    TypeError for a non-CsrAdjacency, ValueError for a wrong shape, dtype or num_relations, GcnAmdError for CPU tensors."""

    def __init__(self, adj, etype, num_relations):
        if not isinstance(adj, CsrAdjacency):
            raise TypeError("EdgeTypes: adj must be a CsrAdjacency")
        if isinstance(num_relations, bool) or not isinstance(num_relations, int) or not 1 <= num_relations < 2 ** 31 - 1:
            raise ValueError(f"EdgeTypes: num_relations must be an int in [1, 2^31 - 1), not {num_relations!r}")
        if not isinstance(etype, torch.Tensor) or etype.dim() != 1 or etype.shape[0] != adj.nnz or \
                etype.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"EdgeTypes: etype must be a 1-D int32 or int64 tensor of nnz = {adj.nnz} entries")
        if not etype.is_cuda:
            raise _lib.GcnAmdError("EdgeTypes: etype must be a CUDA/HIP tensor (no CPU path in gcn_amd)")
        R = num_relations
        if etype.dtype == torch.int64:                       # (a type that does not fit int32 is out of range: the mask)
            etype = torch.where((etype >= 0) & (etype < R), etype, torch.full_like(etype, -1))
        self.adj, self.num_relations = adj, R
        self.etype = etype.to(device=adj.device, dtype=torch.int32).contiguous()
        self._view = self._norm = self._grouped = None

    def _keys(self):
        """the type of every entry, out-of-range types as num_relations (int64)"""
        t = self.etype.long()
        return torch.where((t >= 0) & (t < self.num_relations), t, torch.full_like(t, self.num_relations))

    def _rows(self):
        rp = self.adj.rowptr.long()
        return torch.repeat_interleave(torch.arange(self.adj.m, device=self.adj.device), rp[1:] - rp[:-1], output_size=self.adj.nnz)

    def relation_view(self):
        """(relptr int32 [R + 2], row, col, perm int32 [nnz]): the entries in type-major stable order — relation t holds
        relptr[t] .. relptr[t + 1], masked entries sit in the bucket behind the last relation — each with its row, its
        column and its index in ``adj``.  Built at the first coefficient gradient (one host synchronisation) and kept."""
        if self._view is None:
            relptr, perm = bucket_by_key(self._keys().to(torch.int32), self.num_relations + 1)
            at = perm.long()
            self._view = (relptr, self._rows().index_select(0, at).to(torch.int32), self.adj.col.index_select(0, at).contiguous(), perm)
        return self._view

    def grouped_positions(self):
        """(perm int64 [nnz], inverse int32 [nnz], tpos int32 [nnz]) for ``relation_transform_aggregate``: the view's perm
        as an index, the position in the view of every entry of ``adj`` (its inverse), and the position in the view of
        every entry of the transposed pattern (``adj.tpattern()``).  Built once, with the view, and kept."""
        if self._grouped is None:
            perm = self.relation_view()[3].long()
            inverse = torch.empty(self.adj.nnz, dtype=torch.int32, device=self.adj.device)
            inverse[perm] = torch.arange(self.adj.nnz, dtype=torch.int32, device=self.adj.device)
            self._grouped = (perm, inverse, inverse.index_select(0, self.adj.tpattern()[2].long()).contiguous())
        return self._grouped

    def norm(self):
        """fp32 [nnz]: 1 / the number of entries with the same (row, type), R-GCN's 1 / c_{i,r} (PyG's aggr="mean");
        0 for a masked entry.  Computed once and kept."""
        if self._norm is None:
            keys = self._keys()
            _, inverse, counts = torch.unique(self._rows() * (self.num_relations + 1) + keys, return_inverse=True, return_counts=True)
            inv = 1.0 / counts.index_select(0, inverse).to(torch.float32)
            self._norm = torch.where(keys < self.num_relations, inv, torch.zeros_like(inv)).contiguous()
        return self._norm


def _scratch(adj, k, planes, device):
    """the "relation_aggregate" buffer of the adjacency (gcn_relation_aggregate_ws_bytes: a flag and a float per chunk,
    long row, column and plane of a pass), shared by the forward and both gradients; None for a pattern without entries"""
    planes = 8 if planes > 4 else 4 if planes > 2 else int(planes)        # the planes of the widest pass: 1, 2, 4 or 8
    nbytes = 16 + 8 * planes * int(k) * ((adj.nnz + _CHUNK - 1) // _CHUNK)
    return adj._scratch.get("relation_aggregate", nbytes, device) if adj.nnz else None


class _RelationFunction(torch.autograd.Function):
    """out [m, B k]; the gradient in x by one walk of the transposed pattern, in coeff by one walk of the relation-major view"""

    @staticmethod
    def forward(ctx, types, x, coeff, values):
        adj, R = types.adj, types.num_relations
        x = x.detach().contiguous()
        coeff = coeff.detach().contiguous() if coeff is not None else None
        values = values.detach().contiguous() if values is not None else None
        k = int(x.shape[1])
        B = int(coeff.shape[1]) if coeff is not None else R
        out = torch.empty((adj.m, B * k), dtype=torch.float32, device=x.device)
        ws = _scratch(adj, k, B, x.device)
        call("gcn_relation_aggregate_csr_f32", adj.rowptr, adj.col, types.etype, adj.m, adj.n, adj.nnz, x, k, coeff, R, B, values,
             out, ws, ws.numel() if ws is not None else 0, device=x.device)
        ctx.types, ctx.B = types, B
        ctx.save_for_backward(x, coeff, values)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, coeff, values = ctx.saved_tensors
        types, B = ctx.types, ctx.B
        adj, R = types.adj, types.num_relations
        g = g.contiguous()
        k = int(x.shape[1])
        ws = _scratch(adj, k, B, g.device)
        ws_bytes = ws.numel() if ws is not None else 0
        gx = gcoeff = None
        if ctx.needs_input_grad[1]:
            gx = torch.empty((adj.n, k), dtype=torch.float32, device=g.device)
            trowptr, trow, tperm = adj.tpattern()
            call("gcn_relation_aggregate_backward_x_csr_f32", trowptr, trow, tperm, types.etype, adj.n, adj.m, adj.nnz, g, k, coeff,
                 R, B, values, gx, ws, ws_bytes, device=g.device)
        if coeff is not None and ctx.needs_input_grad[2]:
            gcoeff = torch.empty((R, B), dtype=torch.float32, device=g.device)
            relptr, rrow, rcol, rperm = types.relation_view()
            call("gcn_relation_aggregate_backward_coeff_f32", relptr, rrow, rcol, rperm, R, adj.m, adj.n, adj.nnz, g, x, k, B,
                 values, gcoeff, ws, ws_bytes, device=g.device)
        return None, gx, gcoeff, None


def relation_aggregate(types, x, coeff=None, values=None):
    """out[r, b k + j] = sum over the stored entries e of row r of ``coeff[etype[e], b] * values[e] * x[col[e], j]``: the B
    basis planes of R-GCN side by side, [m, B k], from one gather of x per entry (duplicates are separate entries).

    types: an ``EdgeTypes``.  x: [n, k] fp32 device tensor, differentiable.  coeff: [R, B] fp32, differentiable, or None —
    the typed mode: [m, R k], plane t sums exactly the entries of type t (a selection: a non-finite row of x reached only
    through relation t touches plane t alone; with coeff, 0 * NaN = NaN reaches every plane as in the dense formula).
    values: [nnz] fp32 in the entry order of the adjacency, or None (ones); NOT differentiable: no gradient flows to it.
    An entry with a type outside [0, R) contributes nothing.  An empty row gives zeros.  B > 8 runs as passes of 8 planes.
    TypeError for a non-EdgeTypes, ValueError for a wrong shape, GcnAmdError for a CPU tensor or a dtype other than fp32."""
    if not isinstance(types, EdgeTypes):
        raise TypeError("relation_aggregate: types must be an EdgeTypes")
    adj, R = types.adj, types.num_relations
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[0] != adj.n or x.shape[1] < 1:
        raise ValueError(f"relation_aggregate: x must be a 2-D tensor of n = {adj.n} rows and at least one column")
    if coeff is not None and (not isinstance(coeff, torch.Tensor) or coeff.dim() != 2 or coeff.shape[0] != R or coeff.shape[1] < 1):
        raise ValueError(f"relation_aggregate: coeff must be a 2-D tensor of R = {R} rows and at least one column")
    if values is not None and (not isinstance(values, torch.Tensor) or values.dim() != 1 or values.shape[0] != adj.nnz):
        raise ValueError(f"relation_aggregate: values must be a 1-D tensor of nnz = {adj.nnz} entries")
    for name, t in (("x", x), ("coeff", coeff), ("values", values)):
        if t is not None and not t.is_cuda:
            raise _lib.GcnAmdError(f"relation_aggregate: {name} must be a CUDA/HIP tensor (no CPU path in gcn_amd)")
        if t is not None and t.dtype != torch.float32:
            raise _lib.GcnAmdError(f"relation_aggregate: {name} must be fp32")
    if values is not None and values.requires_grad:
        raise ValueError("relation_aggregate: values is not differentiable (detach it)")
    planes = int(coeff.shape[1]) if coeff is not None else R
    if planes * int(x.shape[1]) >= 2 ** 31:
        raise ValueError("relation_aggregate: the output's width B * k must stay below 2^31")
    return _RelationFunction.apply(types, x, coeff, values)


class _RelationTransformFunction(torch.autograd.Function):
    """out [m, O]; one gathered segment GEMM over the relation-major view and the row sums back, forward and backward"""

    @staticmethod
    def forward(ctx, types, x, weight, values):
        adj = types.adj
        x, weight = x.detach().contiguous(), weight.detach().contiguous()
        relptr, _rrow, rcol, _rperm = types.relation_view()
        perm, inverse, _tpos = types.grouped_positions()
        scale = values.detach().index_select(0, perm) if values is not None else None      # values in the view's order
        msg = _forward_raw(adj._scratch, x, rcol, scale, relptr, weight, False, adj.nnz)     # [nnz, O]; the masked bucket zeros
        out = torch.empty((adj.m, weight.shape[2]), dtype=torch.float32, device=x.device)
        ctx.types = types
        ctx.save_for_backward(x, weight, scale)
        return _segment_sum_raw(adj, adj.rowptr, adj.m, msg, inverse, out)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, weight, scale = ctx.saved_tensors
        types = ctx.types
        adj = types.adj
        g = g.contiguous()
        relptr, rrow, rcol, _rperm = types.relation_view()
        gx = gw = None
        if ctx.needs_input_grad[1]:
            gz = _forward_raw(adj._scratch, g, rrow, scale, relptr, weight, True, adj.nnz)   # [nnz, K]
            gx = torch.empty((adj.n, x.shape[1]), dtype=torch.float32, device=g.device)
            _segment_sum_raw(adj, adj.tpattern()[0], adj.n, gz, types.grouped_positions()[2], gx)
        if ctx.needs_input_grad[2]:
            gw = _wgrad_raw(adj._scratch, x, rcol, g, rrow, scale, relptr, types.num_relations, adj.nnz)
        return None, gx, gw, None


def relation_transform_aggregate(types, x, weight, values=None):
    """out[r] = sum over the stored entries e of row r of ``values[e] * x[col[e]] @ weight[etype[e]]``: [m, O], a matrix per
    relation WITHOUT the [m, R k] planes of the typed mode, so the number of relations may be in the hundreds.

    Forward: one gathered segment GEMM (``segment_mm.hip``) over ``types.relation_view()`` — the entries in type-major
    order, x gathered by their columns, scaled by their values — then atomic-free row sums (``segment_sum``) back into the
    rows.  Gradient in x: the same kernel on the transposed weights with the rows of g gathered, then the row sums over
    ``adj.tpattern()``; in weight: the weight-gradient kernel with both operands gathered.  The only nnz-sized intermediates
    are [nnz, O] forward and [nnz, K] backward (DGL's low-memory path); nnz * max(K, O) must stay below 2^31.
    types: an ``EdgeTypes``; an entry with a type outside [0, R) contributes nothing.  x: [n, K] fp32, differentiable.
    weight: [R, K, O] fp32, differentiable.  values: [nnz] fp32 in the entry order of the adjacency, or None (ones); NOT
    differentiable.  The first call builds the view (one host synchronisation); later calls only enqueue (capturable).
    TypeError for a non-EdgeTypes, ValueError for a wrong shape, GcnAmdError for a CPU tensor or a dtype other than fp32."""
    if not isinstance(types, EdgeTypes):
        raise TypeError("relation_transform_aggregate: types must be an EdgeTypes")
    adj, R = types.adj, types.num_relations
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[0] != adj.n or x.shape[1] < 1:
        raise ValueError(f"relation_transform_aggregate: x must be a 2-D tensor of n = {adj.n} rows and at least one column")
    if not isinstance(weight, torch.Tensor) or weight.dim() != 3 or tuple(weight.shape[:2]) != (R, x.shape[1]) or weight.shape[2] < 1:
        raise ValueError(f"relation_transform_aggregate: weight must be [R, K, O] with R = {R} and K = {x.shape[1]}")
    if values is not None and (not isinstance(values, torch.Tensor) or values.dim() != 1 or values.shape[0] != adj.nnz):
        raise ValueError(f"relation_transform_aggregate: values must be a 1-D tensor of nnz = {adj.nnz} entries")
    _check_fp32("relation_transform_aggregate", (("x", x), ("weight", weight), ("values", values)))
    if values is not None and values.requires_grad:
        raise ValueError("relation_transform_aggregate: values is not differentiable (detach it)")
    if adj.nnz * max(int(x.shape[1]), int(weight.shape[2])) >= 2 ** 31:
        raise ValueError("relation_transform_aggregate: nnz * max(K, O) must stay below 2^31")
    return _RelationTransformFunction.apply(types, x, weight, values)
