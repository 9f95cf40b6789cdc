"""Neighbourhood aggregation by pattern: max, min, sum and mean over the stored entries of each row of a CSR adjacency —
GraphSAGE's aggregators (PyG ``SAGEConv(aggr=...)``, DGL ``copy_u_max``).

    h = gcn_amd.aggregate(adj, x, "max")                      # h[r, j] = max over the entries e of row r of x[col[e], j]
    h, arg = gcn_amd.aggregate(adj, x, "min", return_arg=True)  # arg[r, j]: the CSR entry index that supplied h[r, j]
    h = gcn_amd.aggregate(adj, x, "mean")                     # the SpMM on a pattern-valued twin of adj
    h = gcn_amd.aggregate_multi(adj, x, ("mean", "max", "min", "std"))   # [m, 4 k]: four statistics from one gather per entry
    h = gcn_amd.aggregate_quantile(adj, x, 0.5)               # the lower median of every neighbourhood (Median-GCN)

Only the pattern of ``adj`` is used: its values are ignored, and every stored entry counts, duplicated (row, column)
pairs included.  max / min run on gcn_amd/csrc/aggregate.hip (fp32 or bf16, exact: a selection rounds nothing); an empty
row gives 0 (arg -1), ties go to the lowest entry index, a NaN wins over every number.  Their gradient goes to the
selected entry only — torch's ``scatter_reduce`` splits it among ties — and is computed without atomics, as a walk of
the transposed pattern.  The kernels take no plan and only enqueue, so after one eager call everything here runs
inside a captured step.  There is no CPU path: CPU tensors raise.
"""
import ctypes

import torch

from . import _lib
from ._lib import call
from .spmm import CsrAdjacency, spmm

_CHUNK = 4096                # entries per workspace partial: GCN_AGGREGATE_WS_BYTES in include/gcn_spmm.h
_REDUCE = {"max": _lib.REDUCE_MAX, "min": _lib.REDUCE_MIN}
_DTYPE = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16}
_MULTI = {"max": _lib.REDUCE_MAX, "min": _lib.REDUCE_MIN, "sum": _lib.REDUCE_SUM, "mean": _lib.REDUCE_MEAN,
          "var": _lib.REDUCE_VAR, "std": _lib.REDUCE_STD}


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


def _multi_scratch(adj, k, device):
    """the "aggregate_multi" buffer of the adjacency (GCN_AGGREGATE_MULTI_WS_BYTES: a flag and a 32-byte column state per
    chunk, long row and column), shared by the forward and the backward; None for a pattern without entries"""
    return adj._scratch.get("aggregate_multi", 16 + 64 * int(k) * ((adj.nnz + _CHUNK - 1) // _CHUNK), device) if adj.nnz else None


class _MultiFunction(torch.autograd.Function):
    """(out, argmax, argmin) = the requested statistics side by side and the entries that supplied the extrema (None for a
    plane not requested); the gradient in x by one walk of the transposed pattern"""

    @staticmethod
    def forward(ctx, adj, x, reduce, eps):
        x = x.detach().contiguous()
        k, nred = int(x.shape[1]), len(reduce)
        codes = (ctypes.c_int32 * nred)(*[_MULTI[r] for r in reduce])
        new = lambda dtype, width=k: torch.empty((adj.m, width), dtype=dtype, device=x.device)
        out = new(torch.float32, nred * k)
        argmax = new(torch.int32) if "max" in reduce else None
        argmin = new(torch.int32) if "min" in reduce else None
        moments = "var" in reduce or "std" in reduce
        # the backward of var / std reads the mean: a plane of out, or a buffer of its own
        mean = new(torch.float32) if ctx.needs_input_grad[1] and moments and "mean" not in reduce else None
        ws = _multi_scratch(adj, k, x.device)
        call("gcn_aggregate_multi_csr_f32", adj.rowptr, adj.col, adj.m, adj.n, adj.nnz, x, k, nred, codes, eps, out, argmax, argmin,
             mean, ws, ws.numel() if ws is not None else 0, device=x.device)
        ctx.adj, ctx.reduce, ctx.codes = adj, reduce, codes
        ctx.slots = [t is not None for t in (argmax, argmin, mean)]
        ctx.save_for_backward(x, out, *[t for t in (argmax, argmin, mean) if t is not None])
        ctx.mark_non_differentiable(*[t for t in (argmax, argmin) if t is not None])
        return out, argmax, argmin

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_max, _g_min):
        if not ctx.needs_input_grad[1]:
            return None, None, None, None
        x, out, *rest = ctx.saved_tensors
        rest = iter(rest)
        argmax, argmin, mean = [next(rest) if have else None for have in ctx.slots]
        adj, reduce = ctx.adj, ctx.reduce
        g = g.contiguous()
        k = int(x.shape[1])
        gx = torch.empty((adj.n, k), dtype=torch.float32, device=g.device)
        affine = any(r in reduce for r in ("sum", "mean", "var", "std"))
        ab = torch.empty((adj.m, 2 * k), dtype=torch.float32, device=g.device) if affine else None
        trowptr, trow, tperm = adj.tpattern()
        ws = _multi_scratch(adj, k, g.device)
        call("gcn_aggregate_multi_backward_csr_f32", trowptr, trow, tperm, adj.rowptr, adj.n, adj.m, adj.nnz, g, x, k, len(reduce),
             ctx.codes, out, argmax, argmin, mean, ab, gx, ws, ws.numel() if ws is not None else 0, device=g.device)
        return None, gx, None, None


def aggregate_multi(adj, x, reduce=("mean", "max", "min", "std"), eps=1e-5, return_arg=False):
    """Several statistics of every row's neighbourhood from ONE gather per stored entry (PNA's aggregators, PyG's
    ``MultiAggregation(mode="cat")``): out[r, p k : (p + 1) k] = the element-wise ``reduce[p]`` of x[c, :] over the stored
    entries (r, c) of row r of ``adj`` (any CsrAdjacency: pattern only, duplicates are separate entries).

    x: [n, k] fp32 device tensor, differentiable (one walk of the transposed pattern for all planes).  reduce: distinct
    names of "max", "min", "sum", "mean", "var" (population variance, from sums shifted by the row's first entry: no
    cancellation), "std" = sqrt(var + eps); eps >= 0, and > 0 with "std".  An empty row gives zeros in every plane; a row of
    one entry or of equal entries has var exactly 0; a non-finite entry makes the row's var / std NaN.  max / min follow
    ``aggregate``'s rule and their gradient goes to the selected entry.  ``return_arg=True`` also returns (argmax, argmin),
    int32 [m, k] CSR entry indices (-1 for an empty row), None for a plane not requested, not differentiable.
    TypeError for a non-CsrAdjacency, ValueError for a wrong shape, an empty, unknown or repeated reduce or a bad eps,
    GcnAmdError for a CPU tensor or a dtype other than fp32 (bf16 is not served by this unit)."""
    if not isinstance(adj, CsrAdjacency):
        raise TypeError("aggregate_multi: adj must be a CsrAdjacency")
    reduce = (reduce,) if isinstance(reduce, str) else tuple(reduce)
    if not reduce or any(r not in _MULTI for r in reduce) or len(set(reduce)) != len(reduce):
        raise ValueError(f"aggregate_multi: reduce must be distinct names of {sorted(_MULTI)}, not {reduce!r}")
    eps = float(eps)
    if not 0.0 <= eps < float("inf") or (eps == 0.0 and "std" in reduce):
        raise ValueError(f"aggregate_multi: eps must be finite and >= 0 (> 0 with 'std'), not {eps!r}")
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[0] != adj.n or x.shape[1] < 1:
        raise ValueError(f"aggregate_multi: x must be a 2-D tensor of n = {adj.n} rows and at least one column")
    if not x.is_cuda:
        raise _lib.GcnAmdError("aggregate_multi: x must be a CUDA/HIP tensor (no CPU path in gcn_amd)")
    if x.dtype != torch.float32:
        raise _lib.GcnAmdError("aggregate_multi: x must be fp32")
    out, argmax, argmin = _MultiFunction.apply(adj, x, reduce, eps)
    return (out, argmax, argmin) if return_arg else out


class _QuantileFunction(torch.autograd.Function):
    """(out, arg) = the order statistics of every row, plane by plane, and the entries that supplied them; the gradient of
    each plane goes to x[col[arg]] by the max / min backward walk, and the planes' gradients are summed"""

    @staticmethod
    def forward(ctx, adj, x, q):
        x = x.detach().contiguous()
        k, nq = int(x.shape[1]), len(q)
        out = torch.empty((adj.m, nq * k), dtype=torch.float32, device=x.device)
        arg = torch.empty((adj.m, nq * k), dtype=torch.int32, device=x.device)
        ws = adj._scratch.get("aggregate_quantile", 16, x.device) if adj.nnz else None   # GCN_AGGREGATE_QUANTILE_WS_BYTES
        call("gcn_aggregate_quantile_csr_f32", adj.rowptr, adj.col, adj.m, adj.n, adj.nnz, x, k, (ctypes.c_double * nq)(*q), nq,
             out, arg, ws, ws.numel() if ws is not None else 0, device=x.device)
        ctx.adj, ctx.nq = adj, nq
        ctx.save_for_backward(arg)
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_arg):
        if not ctx.needs_input_grad[1]:
            return None, None, None
        (arg,) = ctx.saved_tensors
        adj, nq = ctx.adj, ctx.nq
        k = int(g.shape[1]) // nq
        trowptr, trow, tperm = adj.tpattern()
        ws = _scratch(adj, k, g.device)
        total = None
        for i in range(nq):                              # one walk of the transposed pattern per plane
            gi, ai = g[:, i * k:(i + 1) * k].contiguous(), arg[:, i * k:(i + 1) * k].contiguous()
            gx = torch.empty((adj.n, k), dtype=torch.float32, device=g.device)
            call("gcn_aggregate_backward_csr", trowptr, trow, tperm, adj.n, adj.m, adj.nnz, gi, _lib.DTYPE_F32, ai, k, gx,
                 ws, ws.numel() if ws is not None else 0, device=g.device)
            total = gx if total is None else total.add_(gx)
        return None, total, None


def _quantiles(q, what):
    """q as a tuple of 1 to 4 floats in [0, 1]; ValueError otherwise"""
    try:
        qs = (float(q),) if isinstance(q, (int, float)) and not isinstance(q, bool) else tuple(float(v) for v in q)
    except (TypeError, ValueError):
        qs = ()
    if not 1 <= len(qs) <= 4 or not all(0.0 <= v <= 1.0 for v in qs):
        raise ValueError(f"{what}: q must be a float or a tuple of 1 to 4 floats in [0, 1], not {q!r}")
    return qs


def aggregate_quantile(adj, x, q=0.5, return_arg=False):
    """Order statistics of every row's neighbourhood (PyG's ``QuantileAggregation(interpolation="lower")``; q = 0.5 is
    ``MedianAggregation`` / ``torch.median``'s lower median, the reduction of Median-GCN): for each quantile q[i],
    out[r, i k + j] = the element of rank floor(q[i] (d - 1)) of x[c, j] over the d stored entries (r, c) of row r of ``adj``
    (any CsrAdjacency: pattern only, duplicates are separate entries), on gcn_amd/csrc/aggregate_quantile.hip.

    x: [n, k] fp32 device tensor, differentiable.  q: a float or a tuple of 1 to 4 floats in [0, 1]; the result is
    [m, len(q) k] fp32, the planes side by side as in ``aggregate_multi``.  Entries are ordered by (value, entry index),
    -0.0 equal to +0.0, +-inf ordinary values; a column that holds a NaN gives the first NaN entry in every plane; an empty
    row gives zeros.  Exact: a selection rounds nothing.  The gradient of each plane goes to the selected entry only (the
    max / min backward walk, once per plane).  ``return_arg=True`` also returns the int32 [m, len(q) k] CSR entry indices
    that supplied the values (-1 for an empty row), not differentiable.
    TypeError for a non-CsrAdjacency, ValueError for a bad q or a wrong shape, GcnAmdError for a CPU tensor or a dtype other
    than fp32."""
    if not isinstance(adj, CsrAdjacency):
        raise TypeError("aggregate_quantile: adj must be a CsrAdjacency")
    qs = _quantiles(q, "aggregate_quantile")
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[0] != adj.n or x.shape[1] < 1:
        raise ValueError(f"aggregate_quantile: x must be a 2-D tensor of n = {adj.n} rows and at least one column")
    if not x.is_cuda:
        raise _lib.GcnAmdError("aggregate_quantile: x must be a CUDA/HIP tensor (no CPU path in gcn_amd)")
    if x.dtype != torch.float32:
        raise _lib.GcnAmdError("aggregate_quantile: x must be fp32")
    out, arg = _QuantileFunction.apply(adj, x, qs)
    return (out, arg) if return_arg else out
