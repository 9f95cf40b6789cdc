"""Grouped matrix product: rows sorted by type, a weight matrix per type (DGL's ``segment_mm`` / ``gather_mm`` /
``TypedLinear``, pyg_lib's ``segment_matmul`` / PyG's ``HeteroLinear`` on sorted input).

    y = gcn_amd.segment_matmul(x, segptr, weight)                    # y[i] = x[i] @ weight[t], segptr[t] <= i < segptr[t + 1]
    y = gcn_amd.segment_matmul(x, segptr, weight, index=idx, scale=s) # y[i] = s[i] * (x[idx[i]] @ weight[t])
    lin = gcn_amd.TypedLinear(in_dim, out_dim, num_types); y = lin(x, segptr)

Runs on gcn_amd/csrc/segment_mm.hip (fp32, the matrix cores): plan-free kernels that only enqueue and never read ``segptr``
on the host, so after one eager call (which allocates the scratch) a call with a ``RowGather`` or without an index runs
inside a captured step.  No atomics; two calls give the same bits.  There is no CPU path: CPU tensors raise.
"""
import ctypes
import functools
import math

import torch
from torch import nn
from torch.nn.parameter import Parameter

from . import _lib
from ._lib import call
from .attention import _loose_scratch, _segment_sum_raw
from .construct import bucket_by_key


@functools.lru_cache(maxsize=None)
def _ws_bytes(N, T, K, O):
    """gcn_segment_mm_ws_bytes: the segment, tile and chunk prefixes and a [K, O] partial per possible chunk"""
    need = ctypes.c_size_t(0)
    call("gcn_segment_mm_ws_bytes", N, T, K, O, ctypes.byref(need))
    return need.value


def _forward_raw(keeper, x, x_index, scale, segptr, weight, transpose_w, N):
    """y [N, O] = scale * (x[x_index] @ op(weight[t])) on contiguous detached operands; keeper: the Scratch that owns the
    workspace.  weight [T, K, O], or [T, O, K] with transpose_w"""
    T, K = int(weight.shape[0]), int(x.shape[1])
    O = int(weight.shape[1 if transpose_w else 2])
    y = torch.empty((N, O), dtype=torch.float32, device=x.device)
    if N:
        ws = keeper.get("segment_mm", _ws_bytes(N, T, K, O), x.device)
        call("gcn_segment_mm_f32", x, int(x.shape[0]), x_index, scale, segptr, weight, int(transpose_w), N, T, K, O, y, ws,
             ws.numel(), device=x.device)
    return y


def _wgrad_raw(keeper, x, x_index, g, g_index, scale, segptr, T, N):
    """dW [T, K, O] = per segment the sum of scale * x[x_index]^T (x) g[g_index]"""
    K, O = int(x.shape[1]), int(g.shape[1])
    dw = torch.empty((T, K, O), dtype=torch.float32, device=x.device)
    if T:
        ws = keeper.get("segment_mm", _ws_bytes(N, T, K, O), x.device)
        call("gcn_segment_mm_wgrad_f32", x, int(x.shape[0]), x_index, g, int(g.shape[0]), g_index, scale, segptr, N, T, K, O, dw,
             ws, ws.numel(), device=x.device)
    return dw


class RowGather:
    """A row index for ``segment_matmul`` and what its gradient needs, built once: ``index`` int32 [N] with every entry in
    [0, n), repeats allowed, and the stable bucketing of its positions by target row (one host synchronisation, here), which
    turns the gradient's scatter into atomic-free row sums.  ValueError for a wrong shape, dtype, n or an index out of range,
    GcnAmdError for a CPU tensor."""

    def __init__(self, index, n):
        if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n < 2 ** 31:
            raise ValueError(f"RowGather: n must be an int in [0, 2^31), not {n!r}")
        if not isinstance(index, torch.Tensor) or index.dim() != 1 or index.dtype != torch.int32:
            raise ValueError("RowGather: index must be a 1-D int32 tensor")
        if not index.is_cuda:
            raise _lib.GcnAmdError("RowGather: index must be a CUDA/HIP tensor (no CPU path in gcn_amd)")
        self.index, self.n = index.contiguous(), n
        self.ptr, self.perm = bucket_by_key(self.index, n)


class _SegmentMatmulFunction(torch.autograd.Function):
    """y [N, O]; the gradient in x by the same kernel on the transposed weights (then row sums by index), in weight by the
    weight-gradient kernel"""

    @staticmethod
    def forward(ctx, x, segptr, weight, gather, scale):
        x, weight = x.detach().contiguous(), weight.detach().contiguous()
        scale = scale.detach().contiguous() if scale is not None else None
        index = gather.index if gather is not None else None
        N = int(index.shape[0]) if index is not None else int(x.shape[0])
        ctx.gather, ctx.N = gather, N
        ctx.save_for_backward(x, segptr, weight, scale)
        return _forward_raw(_loose_scratch(x.device), x, index, scale, segptr, weight, False, N)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, segptr, weight, scale = ctx.saved_tensors
        gather, N = ctx.gather, ctx.N
        g = g.contiguous()
        keeper = _loose_scratch(g.device)
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = _forward_raw(keeper, g, None, scale, segptr, weight, True, N)               # [N, K], per row of the output
            if gather is not None:
                gx = _segment_sum_raw(keeper, gather.ptr, gather.n, gx, gather.perm,
                                      torch.empty((gather.n, x.shape[1]), dtype=torch.float32, device=g.device))
        if ctx.needs_input_grad[2]:
            gw = _wgrad_raw(keeper, x, gather.index if gather is not None else None, g, None, scale, segptr,
                            int(weight.shape[0]), N)
        return gx, None, gw, None, None


def _check_fp32(what, items):
    """device, then dtype, of the float operands (GcnAmdError), as relation_aggregate does"""
    for name, t in items:
        if t is not None and not t.is_cuda:
            raise _lib.GcnAmdError(f"{what}: {name} must be a CUDA/HIP tensor (no CPU path in gcn_amd)")
        if t is not None and t.dtype != torch.float32:
            raise _lib.GcnAmdError(f"{what}: {name} must be fp32")


def segment_matmul(x, segptr, weight, index=None, scale=None):
    """y[i] = scale[i] * (x[index[i]] @ weight[t]) for the rows i of segment t, ``segptr[t] <= i < segptr[t + 1]``: [N, O],
    N = len(index), or the rows of x without one.

    x: [n, K] fp32 device tensor, differentiable.  segptr: int32 [T + 1] device tensor, never read on the host; a decreasing
    pointer is an empty segment, and rows in front of segptr[0] or behind segptr[T] come out as zeros (and pass no gradient).
    weight: [T, K, O] fp32, differentiable.  index: None, an int32 [N] device tensor with entries in [0, n) (wrapped in a
    ``RowGather`` at every call: one host synchronisation, eager only), or a ``RowGather(index, n)`` built once (capturable).
    scale: [N] fp32 or None, applied once to the finished dot product; NOT differentiable.
    The gradient in weight comes from the weight-gradient kernel, the gradient in x from the forward kernel on the transposed
    weights, followed with an index by atomic-free row sums (``segment_sum`` over the index's bucketing).  A non-finite row
    of x reaches the rows that gather it only, a non-finite weight[t] segment t only.  Exact fp32 fma chains in a fixed
    order: the same bits at every call.  No second derivatives.
    TypeError for an index that is neither, ValueError for a wrong shape or a scale that requires grad, GcnAmdError for a
    CPU tensor or a dtype other than fp32."""
    if index is not None and not isinstance(index, (torch.Tensor, RowGather)):
        raise TypeError("segment_matmul: index must be None, an int32 tensor or a RowGather")
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[1] < 1:
        raise ValueError("segment_matmul: x must be a 2-D tensor of at least one column")
    if not isinstance(segptr, torch.Tensor) or segptr.dim() != 1 or segptr.shape[0] < 1 or segptr.dtype != torch.int32:
        raise ValueError("segment_matmul: segptr must be a 1-D int32 tensor of T + 1 entries")
    T, K = int(segptr.shape[0]) - 1, int(x.shape[1])
    if not isinstance(weight, torch.Tensor) or weight.dim() != 3 or tuple(weight.shape[:2]) != (T, K) or weight.shape[2] < 1:
        raise ValueError(f"segment_matmul: weight must be [T, K, O] with T = {T} segments and K = {K} columns of x")
    if isinstance(index, RowGather):
        if index.n != x.shape[0]:
            raise ValueError(f"segment_matmul: the RowGather indexes {index.n} rows, x has {x.shape[0]}")
        N = int(index.index.shape[0])
    elif index is not None:
        if index.dim() != 1 or index.dtype != torch.int32:
            raise ValueError("segment_matmul: index must be a 1-D int32 tensor")
        N = int(index.shape[0])
    else:
        N = int(x.shape[0])
    if scale is not None and (not isinstance(scale, torch.Tensor) or scale.dim() != 1 or scale.shape[0] != N):
        raise ValueError(f"segment_matmul: scale must be a 1-D tensor of N = {N} entries")
    if scale is not None and scale.requires_grad:
        raise ValueError("segment_matmul: scale is not differentiable (detach it)")
    if int(weight.shape[2]) * K >= 2 ** 31:
        raise ValueError("segment_matmul: K * O must stay below 2^31")
    _check_fp32("segment_matmul", (("x", x), ("weight", weight), ("scale", scale)))
    if not segptr.is_cuda:
        raise _lib.GcnAmdError("segment_matmul: segptr must be a CUDA/HIP tensor (no CPU path in gcn_amd)")
    if isinstance(index, torch.Tensor):
        index = RowGather(index, int(x.shape[0]))
    return _SegmentMatmulFunction.apply(x, segptr.contiguous(), weight, index, scale)


class TypedLinear(nn.Module):
    """A linear layer per type on rows sorted by type (DGL's ``TypedLinear(..., sorted_by_type=True)``, PyG's ``HeteroLinear``
    on sorted input): ``forward(x, segptr)`` gives ``x[i] @ weight[t] + bias[t]`` for the rows i of
    ``segptr[t] .. segptr[t + 1]``, one grouped product (``segment_matmul``); the bias goes through the same segments, as
    the product of a column of ones with ``bias`` [num_types, 1, out_dim].  Rows no segment covers give zeros.  An unsorted
    input is bucketed first: ``ptr, perm = bucket_by_key(types, num_types)``, then
    ``segment_matmul(x, ptr, lin.weight, index=perm)``.  ``weight`` and ``bias`` are uniform in +-1/sqrt(out_dim)."""

    def __init__(self, in_dim, out_dim, num_types, bias=True):
        super().__init__()
        for name, v in (("in_dim", in_dim), ("out_dim", out_dim), ("num_types", num_types)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"TypedLinear: {name} must be an int >= 1, not {v!r}")
        self.in_dim, self.out_dim, self.num_types = in_dim, out_dim, num_types
        self.weight = Parameter(torch.empty(num_types, in_dim, out_dim))
        if bias:
            self.bias = Parameter(torch.empty(num_types, out_dim))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1.0 / math.sqrt(self.out_dim)
        for p in (self.weight, self.bias):
            if p is not None:
                p.data.uniform_(-stdv, stdv)

    def forward(self, x, segptr):
        if not isinstance(segptr, torch.Tensor) or segptr.dim() != 1 or segptr.shape[0] != self.num_types + 1:
            raise ValueError(f"TypedLinear: segptr must hold num_types + 1 = {self.num_types + 1} entries")
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[1] != self.in_dim:
            raise ValueError(f"TypedLinear: x must be [N, {self.in_dim}]")
        out = segment_matmul(x, segptr, self.weight)
        if self.bias is not None:
            ones = torch.ones((x.shape[0], 1), dtype=torch.float32, device=x.device)
            out = out + segment_matmul(ones, segptr, self.bias.unsqueeze(1))
        return out

    def __repr__(self):
        return f"TypedLinear ({self.in_dim} -> {self.out_dim}, types={self.num_types}, bias={self.bias is not None})"
