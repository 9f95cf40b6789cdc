"""Neighbourhood aggregation by pattern: max, min, sum and mean over the stored entries of each row of a CSR adjacency —
GraphSAGE's aggregators (PyG ``SAGEConv(aggr=...)``, DGL ``copy_u_max``).

    h = gcn_amd.aggregate(adj, x, "max")                      # h[r, j] = max over the entries e of row r of x[col[e], j]
    h, arg = gcn_amd.aggregate(adj, x, "min", return_arg=True)  # arg[r, j]: the CSR entry index that supplied h[r, j]
    h = gcn_amd.aggregate(adj, x, "mean")                     # the SpMM on a pattern-valued twin of adj

Only the pattern of ``adj`` is used: its values are ignored, and every stored entry counts, duplicated (row, column)
pairs included.  max / min run on gcn_amd/csrc/aggregate.hip (fp32 or bf16, exact: a selection rounds nothing); an empty
row gives 0 (arg -1), ties go to the lowest entry index, a NaN wins over every number.  Their gradient goes to the
selected entry only — torch's ``scatter_reduce`` splits it among ties — and is computed without atomics, as a walk of
the transposed pattern.  The kernels take no plan and only enqueue, so after one eager call everything here runs
inside a captured step.  There is no CPU path: CPU tensors raise.
"""
import torch

from . import _lib
from ._lib import call
from .spmm import CsrAdjacency, spmm

_CHUNK = 4096                # entries per workspace partial: GCN_AGGREGATE_WS_BYTES in include/gcn_spmm.h
_REDUCE = {"max": _lib.REDUCE_MAX, "min": _lib.REDUCE_MIN}
_DTYPE = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16}


def _ws_bytes(nnz, k):
    return 16 + 16 * int(k) * ((int(nnz) + _CHUNK - 1) // _CHUNK)


def _scratch(adj, k, device):
    """the "aggregate" buffer of the adjacency (a flag and the partials of rows longer than 4096 entries), shared by its
    calls, which one stream orders; None for a pattern without entries.  Its size grows with k, so a first call of a width
    must come before a capture of it, as everywhere here (the buffer it replaces stays allocated: spmm.Scratch)"""
    return adj._scratch.get("aggregate", _ws_bytes(adj.nnz, k), device) if adj.nnz else None


def _pattern_twin(adj, reduce):
    """adj's pattern with values 1 ("sum") or 1 / row length ("mean"): an adjacency of its own, built once"""
    twins = getattr(adj, "_agg_twins", None)
    if twins is None:
        twins = adj._agg_twins = {}
    twin = twins.get(reduce)
    if twin is None:
        if reduce == "sum":
            val = torch.ones(adj.nnz, dtype=torch.float32, device=adj.device)
        else:
            rp = adj.rowptr.long()
            lens = rp[1:] - rp[:-1]
            val = torch.repeat_interleave(1.0 / lens.clamp(min=1).to(torch.float32), lens, output_size=adj.nnz)
        twin = twins[reduce] = CsrAdjacency(adj.rowptr, adj.col, val, (adj.m, adj.n), symmetric=False, chunk_nnz=adj.chunk_nnz)
    return twin


class _SelectFunction(torch.autograd.Function):
    """(out, arg) = the row-wise max / min and the entry that supplied it; the gradient goes to x[col[arg]]"""

    @staticmethod
    def forward(ctx, adj, x, reduce):
        x = x.detach().contiguous()
        k = int(x.shape[1])
        out = torch.empty((adj.m, k), dtype=x.dtype, device=x.device)
        arg = torch.empty((adj.m, k), dtype=torch.int32, device=x.device)
        ws = _scratch(adj, k, x.device)
        call("gcn_aggregate_csr", adj.rowptr, adj.col, adj.m, adj.n, adj.nnz, x, _DTYPE[x.dtype], k, _REDUCE[reduce], out, arg,
             ws, ws.numel() if ws is not None else 0, device=x.device)
        ctx.adj = adj
        ctx.save_for_backward(arg)
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_arg):
        if not ctx.needs_input_grad[1]:
            return None, None, None
        (arg,) = ctx.saved_tensors
        adj = ctx.adj
        g = g.contiguous()
        k = int(g.shape[1])
        gx = torch.empty((adj.n, k), dtype=g.dtype, device=g.device)
        trowptr, trow, tperm = adj.tpattern()
        ws = _scratch(adj, k, g.device)
        call("gcn_aggregate_backward_csr", trowptr, trow, tperm, adj.n, adj.m, adj.nnz, g, _DTYPE[g.dtype], arg, k, gx,
             ws, ws.numel() if ws is not None else 0, device=g.device)
        return None, gx, None


def aggregate(adj, x, reduce="max", return_arg=False):
    """out[r, :] = the element-wise ``reduce`` of x[c, :] over the stored entries (r, c) of row r of ``adj`` (any
    CsrAdjacency: only its pattern is used, its values are ignored; duplicates are separate entries).

    x: [n, k] fp32 or bf16 device tensor, differentiable; the result has its dtype.  reduce: "max", "min", "sum", "mean".
    An empty row gives zeros.  max / min: ties go to the lowest entry index (-0.0 ties with +0.0), a NaN wins and the first
    NaN entry is reported, +-inf are ordinary values; ``return_arg=True`` also returns the int32 [m, k] CSR entry indices
    that supplied the values (-1 for an empty row), not differentiable.  sum / mean run the SpMM on a twin of ``adj``
    whose values are 1 or 1 / row length, built at the first call and kept.
    TypeError for a non-CsrAdjacency, ValueError for a wrong shape or an unknown reduce (or return_arg with sum / mean),
    GcnAmdError for a CPU tensor or a dtype other than fp32 / bf16."""
    if not isinstance(adj, CsrAdjacency):
        raise TypeError("aggregate: adj must be a CsrAdjacency")
    if return_arg and reduce in ("sum", "mean"):
        raise ValueError("aggregate: return_arg needs reduce='max' or 'min'")
    if reduce not in ("max", "min", "sum", "mean"):
        raise ValueError(f"aggregate: reduce must be 'max', 'min', 'sum' or 'mean', not {reduce!r}")
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[0] != adj.n or x.shape[1] < 1:
        raise ValueError(f"aggregate: x must be a 2-D tensor of n = {adj.n} rows and at least one column")
    if not x.is_cuda:
        raise _lib.GcnAmdError("aggregate: x must be a CUDA/HIP tensor (no CPU path in gcn_amd)")
    if x.dtype not in _DTYPE:
        raise _lib.GcnAmdError("aggregate: x must be fp32 or bf16")
    if reduce in _REDUCE:
        out, arg = _SelectFunction.apply(adj, x, reduce)
        return (out, arg) if return_arg else out
    if adj.m == 0 or adj.nnz == 0:                       # (nothing to sum: no twin, no plan)
        return x.new_zeros((adj.m, int(x.shape[1])))
    return spmm(_pattern_twin(adj, reduce), x)
