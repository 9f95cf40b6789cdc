"""The callers of the aggregation op, mirrored from pygcn/gcn6.py on top of the native API:

* ``GraphConvolution``  — A(XW) layer  (gcn6.py:66-148)
* ``GraphConvolution2`` — (AX)W layer  (gcn6.py:151-199)
* ``GCN``               — the 2-layer model with gcn6's four preprocessing steps in ``fit``
                          (renumber → schedule → to GPU → permute features; gcn6.py:262-410)
* ``HGNNConv`` / ``HGNN`` — the hypergraph convolution and the two-layer model of pyhgnn/models/HGNN.py, optionally with
                          learnable hyperedge weights through ``HypergraphLaplacian``

Same constructor arguments, parameter initialisation, layer-order rule (A(XW) for layer 2 on
pubmed/flickr, (AX)W otherwise, gcn6.py:214-218), per-layer ``xw / af / bi`` timers and training
loop (Adam, nll_loss on the training rows).  Differences are the ones the path forces: the
adjacency is a ``CsrAdjacency`` handle instead of the nine tile arguments, labels ARE permuted with
the features (the reference forgets to, SURVEY defect D4), and the bias add (+ ReLU for layer 1)
can ride in the SpMM epilogue (``fuse_epilogue=True``).
"""
import math

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.parameter import Parameter

from . import preprocess, reorder, timers
from .aggregate import aggregate
from .edgefeat import edge_aggregate
from .attention import edge_softmax, gat_edge_softmax, gatv2_scores, spmm_heads
from .spgemm import HypergraphLaplacian
from .spmm import CsrAdjacency, _SpmmFunction, _check_values_version, _values_version, dropout_rows, gather_rows, spmm


def _spmm_operand(x):
    """the dense operand of an SpMM inside the model: under a bf16 autocast region the aggregation runs in bf16 like the
    dense products around it (autocast does not cast the operands of a custom autograd Function by itself)"""
    if torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16 and x.dtype == torch.float32:
        return x.to(torch.bfloat16)
    return x


class _FusedSpmmBiasRelu(torch.autograd.Function):
    """out = dropout(relu(Â·X + b)) in one pass over the SpMM output (gcn6.py:141-142, 245-246 as one epilogue);
    backward through the regenerated dropout mask, the ReLU mask, Âᵀ and the bias sum.  dropout = None or
    (p, seed, offset)."""

    @staticmethod
    def forward(ctx, adj, x, bias, relu, dropout=None):
        out = adj.matmul_raw(x, bias=bias, relu=relu, dropout=dropout)
        ctx.adj, ctx.relu, ctx.has_bias, ctx.dropout = adj, relu, bias is not None, dropout
        ctx.values_version = _values_version(adj)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        (out,) = ctx.saved_tensors
        if ctx.dropout is not None and ctx.dropout[0] > 0:
            g = dropout_rows(g, *ctx.dropout)          # the same mask, the same 1/(1-p)
        if ctx.relu:
            g = g * ~(out <= 0)                        # a NaN passes its gradient, as torch's threshold_backward does
                                                       # (dropped elements are 0 in `out`, and their gradient is 0 already)
        g = g.contiguous()
        if ctx.needs_input_grad[1]:
            _check_values_version(ctx.adj, ctx.values_version, "fused SpMM epilogue")
        gx = ctx.adj.transpose().matmul_raw(g) if ctx.needs_input_grad[1] else None
        gb = g.float().sum(0) if ctx.has_bias and ctx.needs_input_grad[2] else None     # (fp32 bias, bf16 activations too)
        return None, gx, gb, None, None


class _Layer(nn.Module):
    def __init__(self, in_features, out_features, with_bias=True, name="dataset", layer="layer0"):
        super().__init__()
        self.in_features, self.out_features, self.layer = in_features, out_features, layer
        self.weight = Parameter(torch.empty(in_features, out_features))
        if with_bias:
            self.bias = Parameter(torch.empty(out_features))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()
        self.timers = timers.Timers()

    def reset_parameters(self):                    # gcn6.py:86-94
        stdv = 1.0 / math.sqrt(self.weight.size(1))
        self.weight.data.uniform_(-stdv, stdv)
        if self.bias is not None:
            self.bias.data.uniform_(-stdv, stdv)

    def reset_timing(self):
        self.timers.reset()

    def __repr__(self):
        return f"{self.__class__.__name__} ({self.in_features} -> {self.out_features})"


class GraphConvolution(_Layer):
    """A(XW): support = X·W, output = Â·support (+ bias)  — gcn6.py:99-143."""

    def forward(self, input, adj, relu=False, fuse_epilogue=False, dropout=None):
        with self.timers.hc.xw:
            support = torch.spmm(input, self.weight) if input.is_sparse else torch.mm(input, self.weight)
        if fuse_epilogue:
            with self.timers.hc.af:
                return _FusedSpmmBiasRelu.apply(adj, _spmm_operand(support), self.bias, relu, dropout)
        with self.timers.hc.af:
            output = _SpmmFunction.apply(adj, _spmm_operand(support))
        if self.bias is not None:
            with self.timers.hc.bi:
                output = output + self.bias
        return F.relu(output) if relu else output


class GraphConvolution2(_Layer):
    """(AX)W: support = Â·X, output = support·W (+ bias)  — gcn6.py:184-194."""

    def forward(self, input, adj, relu=False, fuse_epilogue=False):
        with self.timers.hc.af:
            support = _SpmmFunction.apply(adj, _spmm_operand(input))
        with self.timers.hc.xw:
            output = torch.mm(support, self.weight)
        if self.bias is not None:
            with self.timers.hc.bi:
                output = output + self.bias
        return F.relu(output) if relu else output


class GraphAttention(nn.Module):
    """Graph attention layer (GAT, Velickovic et al. 2018) on the native kernels.  Per head k, with h = x·W_k:

        a_dst = h·att_dst[k],  a_src = h·att_src[k]
        p[e]  = softmax over the stored entries of row(e) of leaky_relu(a_dst[row(e)] + a_src[col(e)], negative_slope)
        out_k = spmm(adj, h, values=p)                          (row r aggregates its stored columns, weighted by p)

    and the heads are concatenated (``concat=True``: heads·out_features columns) or averaged, then the bias is added.
    The scores are fused into the softmax kernel (gat_edge_softmax), the aggregation is the learnable-value SpMM with its
    SDDMM backward; nothing nnz-sized but p and its gradient is ever stored.

    ``adj``: a square CsrAdjacency made with ``mutable_values=True``; its pattern is the attention mask (self-loops
    included or not, as the caller built it) and its own values are ignored — they are overwritten with p.  Heads are a
    Python loop over that one plan: each head's backward re-lays the values its forward saved, so interleaving is safe.

    ``head_batched=True`` runs all heads in one pass instead (gcn_amd/csrc/multihead.hip): a_dst and a_src
    as [n, heads] from one batched reduction of h viewed as [n, heads, out_features], p [nnz, heads] from one fused softmax
    and ``spmm_heads(adj, h, p)`` — one walk of the adjacency per direction that gathers whole heads·out_features-wide rows,
    no plan and no value refresh, so any CsrAdjacency will do.  Same parameters and state_dict; the results differ from the
    loop's by rounding only (other summation orders).  The default stays the loop.

    Parameters: ``weight`` [in_features, heads·out_features], ``att_dst`` and ``att_src`` [heads, out_features] — Glorot
    uniform, as in the paper's code — and ``bias`` [heads·out_features] (concat) or [out_features] (mean), zeros.
    Under a bf16 autocast region x·W runs in bf16 like any matmul; the scores, the softmax and the weighted SpMM run in
    fp32 (h is widened): there is no bf16 softmax kernel, and p's gradient comes from the fp32 SDDMM."""

    def __init__(self, in_features, out_features, heads=1, concat=True, negative_slope=0.2, with_bias=True, head_batched=False):
        super().__init__()
        self.in_features, self.out_features, self.heads = int(in_features), int(out_features), int(heads)
        self.concat, self.negative_slope = bool(concat), float(negative_slope)
        self.head_batched = bool(head_batched)
        if self.heads < 1:
            raise ValueError("heads must be at least 1")
        self.weight = Parameter(torch.empty(self.in_features, self.heads * self.out_features))
        self.att_dst = Parameter(torch.empty(self.heads, self.out_features))
        self.att_src = Parameter(torch.empty(self.heads, self.out_features))
        if with_bias:
            self.bias = Parameter(torch.empty(self.heads * self.out_features if self.concat else self.out_features))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.weight)
        nn.init.xavier_uniform_(self.att_dst)
        nn.init.xavier_uniform_(self.att_src)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward(self, input, adj):
        if adj.m != adj.n or input.shape[0] != adj.n:
            raise ValueError(f"GraphAttention needs a square adjacency over the rows of its input: adjacency {adj.m}x{adj.n}, "
                             f"input {tuple(input.shape)}")
        h = torch.mm(input, self.weight)                # (bf16 under a bf16 autocast region, like any matmul)
        # everything after x·W runs with autocast off: inside the region it would cast torch.mv's operands back to
        # bf16 (mv is on its lower-precision list), and the scores must be fp32 dot products of the widened h
        with torch.autocast("cuda", enabled=False):
            h = h.float()
            if self.head_batched:
                hv = h.view(h.shape[0], self.heads, self.out_features)
                a_dst = (hv * self.att_dst.float()).sum(-1)
                a_src = (hv * self.att_src.float()).sum(-1)
                p = gat_edge_softmax(adj, a_dst, a_src, self.negative_slope)
                out = spmm_heads(adj, h, p)
                if not self.concat and self.heads > 1:
                    out = out.view(h.shape[0], self.heads, self.out_features).mean(1)
                return out + self.bias.float() if self.bias is not None else out
            outs = []
            for k in range(self.heads):
                hk = h[:, k * self.out_features:(k + 1) * self.out_features].contiguous()
                a_dst = torch.mv(hk, self.att_dst[k].float())
                a_src = torch.mv(hk, self.att_src[k].float())
                p = gat_edge_softmax(adj, a_dst, a_src, self.negative_slope)
                outs.append(spmm(adj, hk, values=p))
            if self.heads == 1:
                out = outs[0]
            else:
                out = torch.cat(outs, dim=1) if self.concat else torch.stack(outs).mean(0)
            return out + self.bias.float() if self.bias is not None else out

    def __repr__(self):
        return (f"GraphAttention ({self.in_features} -> {self.out_features}, heads={self.heads}, "
                f"{'concat' if self.concat else 'mean'}{', head-batched' if self.head_batched else ''})")


class GraphAttentionV2(nn.Module):
    """GATv2 layer (Brody et al. 2022; PyG's ``GATv2Conv``) on the native kernels, all heads in one pass:

        h_src = x_src·weight_src,  h_dst = x_dst·weight_dst                        ([n, heads·out_features], [m, ...])
        s[e, k] = sum_j att[k, j] · leaky_relu(h_dst[row(e), kF + j] + h_src[col(e), kF + j], negative_slope)
        p = edge_softmax(adj, s)                                                    (per head, over each row's entries)
        out = spmm_heads(adj, h_src, p)

    and the heads are concatenated (``concat=True``) or averaged, then the bias is added.  The nonlinearity sits between the
    sum of the two node vectors and the dot with ``att`` — the "dynamic" attention GAT's score cannot express.  The score
    kernel (``gatv2_scores``, gcn_amd/csrc/multihead.hip) gathers the rows per entry, forward and backward; nothing wider
    than [nnz, heads] is stored per entry.

    ``forward(input, adj)`` takes one feature matrix over a square adjacency; ``forward((x_src, x_dst), adj)`` takes the two
    sides of a rectangular one (a sampled block: ``adj`` is m x n, x_src has n rows, x_dst m).  Any CsrAdjacency: no plan is
    used and its values are ignored.

    Parameters: ``weight_src`` [in_features, heads·out_features]; ``weight_dst`` of the same shape, absent with
    ``share_weights=True`` (the one weight then serves both sides); ``att`` [heads, out_features]; ``bias``
    [heads·out_features] (concat) or [out_features] (mean), zeros.  Glorot uniform, like GraphAttention.  Under a bf16
    autocast region the two matmuls run in bf16; everything after them runs in fp32 with autocast off."""

    def __init__(self, in_features, out_features, heads=1, concat=True, negative_slope=0.2, with_bias=True, share_weights=False):
        super().__init__()
        self.in_features, self.out_features, self.heads = int(in_features), int(out_features), int(heads)
        self.concat, self.negative_slope = bool(concat), float(negative_slope)
        self.share_weights = bool(share_weights)
        if self.heads < 1:
            raise ValueError("heads must be at least 1")
        self.weight_src = Parameter(torch.empty(self.in_features, self.heads * self.out_features))
        if self.share_weights:
            self.register_parameter("weight_dst", None)
        else:
            self.weight_dst = Parameter(torch.empty(self.in_features, self.heads * self.out_features))
        self.att = Parameter(torch.empty(self.heads, self.out_features))
        if with_bias:
            self.bias = Parameter(torch.empty(self.heads * self.out_features if self.concat else self.out_features))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.weight_src)
        if self.weight_dst is not None:
            nn.init.xavier_uniform_(self.weight_dst)
        nn.init.xavier_uniform_(self.att)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward(self, input, adj):
        x_src, x_dst = input if isinstance(input, (tuple, list)) else (input, input)
        if x_src.shape[0] != adj.n or x_dst.shape[0] != adj.m:
            raise ValueError(f"GraphAttentionV2: adjacency {adj.m}x{adj.n} needs x_src with {adj.n} rows and x_dst with {adj.m}, "
                             f"got {tuple(x_src.shape)} and {tuple(x_dst.shape)}")
        h_src = torch.mm(x_src, self.weight_src)        # (bf16 under a bf16 autocast region, like any matmul)
        if x_dst is x_src and self.weight_dst is None:
            h_dst = h_src
        else:
            h_dst = torch.mm(x_dst, self.weight_src if self.weight_dst is None else self.weight_dst)
        with torch.autocast("cuda", enabled=False):
            h_src, h_dst = h_src.float(), h_dst.float()
            s = gatv2_scores(adj, h_dst, h_src, self.att.float(), self.negative_slope)
            out = spmm_heads(adj, h_src, edge_softmax(adj, s))
            if not self.concat and self.heads > 1:
                out = out.view(out.shape[0], self.heads, self.out_features).mean(1)
            return out + self.bias.float() if self.bias is not None else out

    def __repr__(self):
        return (f"GraphAttentionV2 ({self.in_features} -> {self.out_features}, heads={self.heads}, "
                f"{'concat' if self.concat else 'mean'}{', shared weights' if self.share_weights else ''})")


class SAGEConv(nn.Module):
    """GraphSAGE layer (Hamilton et al. 2017; PyG's ``SAGEConv``) on the native aggregators:

        out = aggregate(adj, x, aggr) · weight_neigh  (+ x · weight_root)  (+ bias)

    ``aggr``: "mean", "max", "min" or "sum" over the stored entries of each row of ``adj`` (pattern only: the values of
    ``adj`` are ignored, see ``gcn_amd.aggregate``).  Sum and mean commute with the linear map, so they aggregate at the
    narrower of ``in_features`` and ``out_features`` — aggregate(x · W) when the layer narrows, the rule of
    ``GCN(layer_order="auto")``; max and min always aggregate x itself.  ``root_weight=True`` adds the vertex's own
    features through a second matrix and needs a square adjacency.

    ``forward((x_src, x_dst), adj)`` takes a bipartite ``adj`` (a sampled block, ``gcn_amd.sample_blocks``): ``x_src`` has
    ``adj.n`` rows and feeds the neighbour term, ``x_dst`` has ``adj.m`` rows and feeds the root term.

    Parameters: ``weight_neigh`` and ``weight_root`` [in_features, out_features] and ``bias`` [out_features], uniform in
    +-1/sqrt(out_features) like the GCN layers.  Under a bf16 autocast region the aggregated operand is bf16 like the
    dense products around it; max and min run on bf16 directly (a selection: exact)."""

    def __init__(self, in_features, out_features, aggr="mean", root_weight=True, with_bias=True):
        super().__init__()
        if aggr not in ("mean", "max", "min", "sum"):
            raise ValueError(f"aggr must be 'mean', 'max', 'min' or 'sum', not {aggr!r}")
        self.in_features, self.out_features, self.aggr = int(in_features), int(out_features), aggr
        self.weight_neigh = Parameter(torch.empty(self.in_features, self.out_features))
        if root_weight:
            self.weight_root = Parameter(torch.empty(self.in_features, self.out_features))
        else:
            self.register_parameter("weight_root", None)
        if with_bias:
            self.bias = Parameter(torch.empty(self.out_features))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1.0 / math.sqrt(self.out_features)
        for p in (self.weight_neigh, self.weight_root, self.bias):
            if p is not None:
                p.data.uniform_(-stdv, stdv)

    def forward(self, input, adj):
        if isinstance(input, (tuple, list)):               # a bipartite block: (x_src [adj.n rows], x_dst [adj.m rows])
            if len(input) != 2:
                raise ValueError("SAGEConv: a bipartite input is the pair (x_src, x_dst)")
            input, root = input
            if input.dim() != 2 or input.shape[0] != adj.n or root.dim() != 2 or root.shape[0] != adj.m:
                raise ValueError(f"SAGEConv: adjacency {adj.m}x{adj.n}, input ({tuple(input.shape)}, {tuple(root.shape)})")
        else:
            if input.dim() != 2 or input.shape[0] != adj.n or (self.weight_root is not None and adj.m != adj.n):
                raise ValueError(f"SAGEConv: adjacency {adj.m}x{adj.n} (square with root_weight), input {tuple(input.shape)}")
            root = input
        if self.aggr in ("sum", "mean") and self.out_features < self.in_features:
            out = aggregate(adj, _spmm_operand(torch.mm(input, self.weight_neigh)), self.aggr)
        else:
            out = torch.mm(aggregate(adj, _spmm_operand(input), self.aggr), self.weight_neigh)
        if self.weight_root is not None:
            out = out + torch.mm(root, self.weight_root)
        return out + self.bias if self.bias is not None else out

    def __repr__(self):
        return (f"SAGEConv ({self.in_features} -> {self.out_features}, aggr={self.aggr}"
                f"{'' if self.weight_root is not None else ', no root weight'})")


class _GINBase(nn.Module):
    """what GINConv and GINEConv share: the wrapped network, eps (a buffer, or a parameter with train_eps) and the
    (x_src, x_dst) form of a sampled block"""

    def __init__(self, net, eps=0.0, train_eps=False):
        super().__init__()
        self.nn = net
        self.initial_eps = float(eps)
        if train_eps:
            self.eps = Parameter(torch.empty(()))
        else:
            self.register_buffer("eps", torch.empty(()))
        self.eps.data.fill_(self.initial_eps)

    def _pair(self, input, adj):
        name = type(self).__name__
        if isinstance(input, (tuple, list)):               # a bipartite block: (x_src [adj.n rows], x_dst [adj.m rows])
            if len(input) != 2:
                raise ValueError(f"{name}: a bipartite input is the pair (x_src, x_dst)")
            x, root = input
        else:
            x = root = input
            if adj.m != adj.n:
                raise ValueError(f"{name}: adjacency {adj.m}x{adj.n} needs the pair (x_src, x_dst)")
        if x.dim() != 2 or x.shape[0] != adj.n or root.dim() != 2 or root.shape[0] != adj.m or root.shape[1] != x.shape[1]:
            raise ValueError(f"{name}: adjacency {adj.m}x{adj.n}, input ({tuple(x.shape)}, {tuple(root.shape)})")
        return x, root


class GINConv(_GINBase):
    """Graph isomorphism layer (Xu et al. 2019; PyG's ``GINConv``): ``out = nn((1 + eps) * x_dst + sum_j x_j)`` over the
    stored entries of each row of ``adj`` (pattern only), on ``aggregate(adj, x, "sum")``.  ``nn`` is any module mapping
    [rows, in] to [rows, out]; ``eps`` is a buffer, or a parameter with ``train_eps=True``.  ``forward((x_src, x_dst), adj)``
    takes a sampled block."""

    def forward(self, input, adj):
        x, root = self._pair(input, adj)
        return self.nn((1.0 + self.eps) * root + aggregate(adj, _spmm_operand(x), "sum"))

    def __repr__(self):
        return f"GINConv (nn={self.nn})"


class GINEConv(_GINBase):
    """GIN with edge features (Hu et al. 2020; PyG's ``GINEConv``) on the native edge-feature aggregation:

        out = nn((1 + eps) * x_dst + sum_j relu(x_j + e_ji))

    ``forward(x, adj, edge_attr)``: ``edge_attr`` [adj.nnz, in_features] in the entry order of ``adj``, or
    [adj.nnz, edge_dim] with ``edge_dim`` given, which adds ``lin = Linear(edge_dim, in_features)`` in front (``in_features``
    is then needed, unless ``nn`` starts with a layer that has ``in_features``).  ``forward((x_src, x_dst), adj, edge_attr)``
    takes a sampled block; the caller passes ``edge_attr[block.eid.long()]``.  The [nnz, in_features] messages are never
    formed: ``gcn_amd.edge_aggregate(adj, x, e, "add", "relu")``."""

    def __init__(self, nn, eps=0.0, train_eps=False, edge_dim=None, in_features=None):
        super().__init__(nn, eps, train_eps)
        if edge_dim is not None:
            if in_features is None:
                first = nn[0] if isinstance(nn, torch.nn.Sequential) and len(nn) else nn
                in_features = getattr(first, "in_features", None)
            if in_features is None:
                raise ValueError("GINEConv: edge_dim needs in_features (the wrapped network does not tell its input width)")
            self.lin = torch.nn.Linear(int(edge_dim), int(in_features))
        else:
            self.lin = None

    def forward(self, input, adj, edge_attr):
        x, root = self._pair(input, adj)
        if self.lin is not None:
            edge_attr = self.lin(edge_attr)
        if edge_attr.dim() != 2 or tuple(edge_attr.shape) != (adj.nnz, int(x.shape[1])):
            raise ValueError(f"GINEConv: edge_attr {tuple(edge_attr.shape)} for {adj.nnz} entries of width {int(x.shape[1])} "
                             "(set edge_dim to map another width)")
        return self.nn((1.0 + self.eps) * root + edge_aggregate(adj, x.float(), edge_attr.float(), "add", "relu", "sum"))

    def __repr__(self):
        return f"GINEConv (nn={self.nn})"


class GraphSAGE(nn.Module):
    """A stack of ``num_layers`` SAGEConv layers with ReLU and dropout between them (Hamilton et al. 2017), for the whole
    graph or for sampled mini-batches:

        logits = model(x, adj)                         # adj: one CsrAdjacency, used by every layer
        blocks, input_ids = gcn_amd.sample_blocks(adj, seeds, fanouts)
        logits = model(x[input_ids], blocks)           # one row per seed; len(blocks) == num_layers

    With blocks, layer i runs on ``(h, h[:blocks[i].num_dst])``: a block's first ``num_dst`` src vertices are its rows.
    The output is the last layer's (no softmax).  There is no ``fit``: the training loop stays with the caller."""

    def __init__(self, in_features, hidden, out_features, num_layers=2, aggr="mean", dropout=0.5, root_weight=True):
        super().__init__()
        if isinstance(num_layers, bool) or not isinstance(num_layers, int) or num_layers < 1:
            raise ValueError(f"GraphSAGE: num_layers must be an int >= 1, not {num_layers!r}")
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"GraphSAGE: dropout must lie in [0, 1), not {dropout!r}")
        widths = [int(in_features)] + [int(hidden)] * (num_layers - 1) + [int(out_features)]
        self.layers = nn.ModuleList(SAGEConv(widths[i], widths[i + 1], aggr=aggr, root_weight=root_weight)
                                    for i in range(num_layers))
        self.dropout = float(dropout)

    def reset_parameters(self):
        for layer in self.layers:
            layer.reset_parameters()

    def forward(self, x, adjs):
        blocks = None
        if not isinstance(adjs, CsrAdjacency):
            blocks = list(adjs)
            if len(blocks) != len(self.layers):
                raise ValueError(f"GraphSAGE: {len(self.layers)} layers need {len(self.layers)} blocks, not {len(blocks)}")
        h = x
        for i, layer in enumerate(self.layers):
            if blocks is None:
                h = layer(h, adjs)
            else:
                h = layer((h, h[:blocks[i].num_dst]), blocks[i].adj)
            if i + 1 < len(self.layers):
                h = F.dropout(F.relu(h), self.dropout, training=self.training)
        return h

    def __repr__(self):
        first, last = self.layers[0], self.layers[-1]
        hidden = f" -> {first.out_features}" if len(self.layers) > 1 else ""
        return (f"GraphSAGE ({first.in_features}{hidden} -> {last.out_features}, layers={len(self.layers)}, "
                f"aggr={first.aggr}, dropout={self.dropout})")


class HGNNConv(nn.Module):
    """The hypergraph convolution of HGNN (Feng et al. 2019; pyhgnn/models/HGNN.py ``HGNN_conv``): ``G · (x·W + b)`` — the
    bias is added BEFORE the aggregation, unlike GraphConvolution.  ``weight`` [in x out] and ``bias`` [out] are drawn from
    uniform(±1/sqrt(out)) as the reference does.

    forward(x, G, values=None): ``G`` is a CsrAdjacency (``hypergraph_laplacian``, or ``HypergraphLaplacian(...).adj``);
    ``values``: nnz fp32 values that replace G's own and may require a gradient (``spmm(G, ·, values=values)``: G must be
    a mutable adjacency).  Returns the output only, not the reference's timing tuple."""

    def __init__(self, in_features, out_features, with_bias=True):
        super().__init__()
        self.in_features, self.out_features = int(in_features), int(out_features)
        self.weight = Parameter(torch.empty(self.in_features, self.out_features))
        if with_bias:
            self.bias = Parameter(torch.empty(self.out_features))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1.0 / math.sqrt(self.weight.size(1))
        self.weight.data.uniform_(-stdv, stdv)
        if self.bias is not None:
            self.bias.data.uniform_(-stdv, stdv)

    def forward(self, x, G, values=None):
        x = x.matmul(self.weight)
        if self.bias is not None:
            x = x + self.bias
        return spmm(G, _spmm_operand(x), values=values)

    def __repr__(self):
        return f"HGNNConv ({self.in_features} -> {self.out_features})"


class HGNN(nn.Module):
    """The two-layer hypergraph network of pyhgnn/models/HGNN.py: ``hgc1 -> relu -> dropout -> hgc2``, with the reference's
    parameter names (``hgc1.weight``, ``hgc1.bias``, ``hgc2.weight``, ``hgc2.bias``), so its checkpoints load strictly.

    forward(x, G) returns the logits only (the reference returns them with four timings).  Dropout follows
    ``self.training``; the reference calls ``F.dropout(x, p)`` without the flag, which is ALWAYS on, evaluation included.
    ``G`` is a CsrAdjacency (``hypergraph_laplacian``).  learn_edge_weights=True: ``G`` is a ``HypergraphLaplacian`` and the
    model owns ``log_edge_weight`` [n_edges], zeros at the start; the hyperedge weights are ``w = exp(log_edge_weight)``,
    which stay positive and whose gradient never dies, and ``G.values(w)`` is computed once per forward and used by both
    layers, so the loss reaches the weights through the Laplacian (``n_edges`` is then required)."""

    def __init__(self, in_ch, n_class, n_hid, dropout=0.5, learn_edge_weights=False, n_edges=None):
        super().__init__()
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"HGNN: dropout must lie in [0, 1), not {dropout!r}")
        self.dropout = float(dropout)
        self.hgc1 = HGNNConv(in_ch, n_hid)
        self.hgc2 = HGNNConv(n_hid, n_class)
        self.learn_edge_weights = bool(learn_edge_weights)
        if self.learn_edge_weights:
            if isinstance(n_edges, bool) or not isinstance(n_edges, int) or n_edges < 1:
                raise ValueError(f"HGNN: learn_edge_weights=True needs n_edges, an int >= 1, not {n_edges!r}")
            self.log_edge_weight = Parameter(torch.zeros(n_edges))

    def forward(self, x, G):
        values = None
        if self.learn_edge_weights:
            if not isinstance(G, HypergraphLaplacian):
                raise TypeError("HGNN: with learn_edge_weights=True, G must be a HypergraphLaplacian")
            values = G.values(torch.exp(self.log_edge_weight))
            G = G.adj
        x = F.relu(self.hgc1(x, G, values))
        x = F.dropout(x, self.dropout, training=self.training)
        return self.hgc2(x, G, values)

    def __repr__(self):
        return (f"HGNN ({self.hgc1.in_features} -> {self.hgc1.out_features} -> {self.hgc2.out_features}, "
                f"dropout={self.dropout}, learn_edge_weights={self.learn_edge_weights})")


class GCN(nn.Module):
    """2-layer GCN with the gcn6 training flow on the native SpMM (gcn6.py:201-441)."""

    def __init__(self, nfeat, nhid, nclass, dataset="dataset", dropout=0.5, lr=0.01, weight_decay=5e-4,
                 with_relu=True, with_bias=True, device=None, order="rabbit", fuse_epilogue=False,
                 layer_order="reference", precompute_ax=False, compute_dtype=torch.float32):
        super().__init__()
        assert device is not None, "Please specify 'device'!"
        self.device, self.nfeat, self.hidden_sizes, self.nclass = device, nfeat, [nhid], nclass
        self.dataname = dataset
        self.gc1 = GraphConvolution(nfeat, nhid, with_bias=with_bias, name=dataset, layer="layer1")
        # Â(XW) or (ÂX)W for layer 2: the reference hard-codes it per dataset (gcn6.py:214-218);
        # layer_order="auto" runs the SpMM at the narrower of the two widths instead —
        # Reddit-shaped, hidden 128 -> 41 classes: SpMM at k = 41 (2.0 ms) instead of k = 128 (3.7 ms)
        if layer_order not in ("reference", "auto"):
            raise ValueError("layer_order must be 'reference' or 'auto'")
        a_xw = (nclass <= nhid) if layer_order == "auto" else dataset in ("pubmed", "flickr")
        if a_xw:
            self.gc2 = GraphConvolution(nhid, nclass, with_bias=with_bias, name=dataset, layer="layer2")
        else:
            self.gc2 = GraphConvolution2(nhid, nclass, with_bias=with_bias, name=dataset, layer="layer2")
        self.dropout, self.lr = dropout, lr
        self.weight_decay = weight_decay if with_relu else 0
        self.with_relu, self.with_bias = with_relu, with_bias
        self.order = order                    # None | "dfs" | "gorder" | "rabbit" (gcn6.py:27-30: RBT default) | "rcm" | "deg" | "rabbit_device" (GPU)
        self.fuse_epilogue = fuse_epilogue
        # precompute_ax: layer 1 is Â·(X·W1) with X the CONSTANT input features (the reference applies dropout behind layer 1,
        # gcn6.py:245-246, never to X), and Â(XW) = (ÂX)W: ÂX is aggregated ONCE (one SpMM at the input width) and every
        # epoch's layer 1 is a dense product — no SpMM in its forward pass and none in its backward pass (W1's gradient is
        # (ÂX)ᵀ·g).  Same function, fp32 rounding apart; n x nfeat floats of memory.  Off by default (the reference recomputes).
        self.precompute_ax = precompute_ax
        # compute_dtype=torch.bfloat16: the forward passes of fit / forward / test / predict run under
        # torch.autocast("cuda", bfloat16) — the dense products and the SpMMs (bf16 operands, fp32 sums) in bf16; the
        # parameters, Adam's state and the loss stay fp32
        if compute_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("compute_dtype must be torch.float32 or torch.bfloat16")
        self.compute_dtype = compute_dtype
        self._ax = None
        self.output = None
        self.adj = self.features = self.labels = self.vo_mp = None
        self.tuning = None                    # {(slices, column tile): ms} measured by prepare() on a renumbered graph
        # fused-epilogue dropout: Philox keyed on (seed, offset).  The seed is drawn from torch's default generator at
        # the first training forward (so torch.manual_seed governs it like F.dropout's masks, two models or two
        # restarts differ unless seeded alike), the offset counts forward passes; both are part of state_dict-less
        # extra state (get_extra_state) so a checkpoint resumes the same mask sequence
        self.dropout_seed, self._dropout_calls = None, 0
        # ... and OPTIONAL on load: a reference-format checkpoint holds the four weight tensors only
        # (profiling_gcn.py:165-170: torch.save(model.state_dict()) / load_state_dict), as do checkpoints of this class
        # written before the extra state existed; a strict load of those must not fail on a missing "_extra_state"
        self._register_load_state_dict_pre_hook(self._default_extra_state)
        self.dur_fwd = timers.Timer()

    @staticmethod
    def _default_extra_state(state_dict, prefix, *_unused):
        state_dict.setdefault(prefix + "_extra_state", {"dropout_seed": None, "dropout_calls": 0})

    def reset_timing(self):
        self.dur_fwd.reset()
        for gc in (self.gc1, self.gc2):
            gc.reset_timing()

    def _layer1_from_cached_ax(self, x, adj):
        if self._ax is None:
            with torch.no_grad():
                self._ax = adj.matmul_raw(x.contiguous())
        with self.gc1.timers.hc.xw:
            h = torch.mm(self._ax, self.gc1.weight)
        if self.gc1.bias is not None:
            with self.gc1.timers.hc.bi:
                h = h + self.gc1.bias
        return F.relu(h) if self.with_relu else h

    def _autocast(self):
        return torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.compute_dtype == torch.bfloat16)

    def forward(self, x, adj):
        with self.dur_fwd, self._autocast():
            if self.precompute_ax and x is self.features and adj is self.adj and not x.requires_grad:
                x = self._layer1_from_cached_ax(x, adj)
                x = F.dropout(x, self.dropout, training=self.training)
                x = self.gc2(x, adj)
                return F.log_softmax(x.float(), dim=1)
            # (under HIP-graph capture the Philox offset, a host integer, would be frozen into the graph — every replay the
            #  same mask; torch's own dropout draws from the generator state the graph registers, so it takes over there)
            if self.fuse_epilogue and self.training and self.dropout > 0 and not torch.cuda.is_current_stream_capturing():
                # bias + ReLU + dropout mask in the SpMM epilogue; a fresh Philox offset per forward pass
                if self.dropout_seed is None:
                    self.dropout_seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
                self._dropout_calls += 1
                x = self.gc1(x, adj, relu=self.with_relu, fuse_epilogue=True,
                             dropout=(float(self.dropout), self.dropout_seed, self._dropout_calls))
            else:
                x = self.gc1(x, adj, relu=self.with_relu, fuse_epilogue=self.fuse_epilogue)
                x = F.dropout(x, self.dropout, training=self.training)
            x = self.gc2(x, adj)
            return F.log_softmax(x.float(), dim=1)

    def get_extra_state(self):
        return {"dropout_seed": self.dropout_seed, "dropout_calls": self._dropout_calls}

    def set_extra_state(self, state):
        self.dropout_seed, self._dropout_calls = state.get("dropout_seed"), int(state.get("dropout_calls", 0))

    def initialize(self):
        self.gc1.reset_parameters()
        self.gc2.reset_parameters()

    def prepare(self, features, adj, labels, normalize=True):
        """gcn6.fit steps 1-4 (gcn6.py:271-379): normalise, renumber on the host, build the SpMM
        schedule, move to the GPU, permute features (and labels)."""
        if sp.issparse(features):
            features = np.asarray(features.todense())
        features = torch.as_tensor(np.asarray(features), dtype=torch.float32)
        adj_norm = preprocess.normalize_adj_tensor(adj) if normalize else preprocess.sparse_mx_to_torch_sparse_tensor(adj)
        rp, ci, va, vo_mp = preprocess.to_csr_int32(adj_norm)
        dev = torch.device(self.device)
        if self.order in ("rcm", "deg", "communities", "rabbit_device"):          # step 1 on the GPU
            # the reference library's internal orderings (order_rcm.cu, order_deg.cu), computed by the
            # device kernels — same integers as the host code, ~100x faster (reorder_device.hip)
            rp, ci, va = rp.to(dev), ci.to(dev), va.to(dev)
            rank = (reorder.order_rcm_device(rp, ci) if self.order == "rcm"
                    else reorder.order_communities_device(rp, ci) if self.order == "communities"
                    else reorder.order_rabbit_device(rp, ci) if self.order == "rabbit_device"    # parallel Rabbit (Arai'16)
                    else reorder.order_deg_device(rp, ci, "total", True))
            rp, ci, va, vo_mp = reorder.apply_rank_device(rp, ci, va, rank)
        else:
            rp, ci, va, vo_mp = rp.numpy(), ci.numpy(), va.numpy(), vo_mp.numpy()
            if self.order:                                                       # step 1 on the host
                rp, ci, va, vo_mp = getattr(reorder, self.order)(rp, ci, va)
            rp, ci, va, vo_mp = (torch.from_numpy(x).to(dev) for x in (rp, ci, va, vo_mp))
        n = rp.numel() - 1
        self.adj = CsrAdjacency(rp, ci, va, (n, n), symmetric=True)             # steps 2+3
        if self.order:
            # A renumbered graph may sit near its diagonal (Rabbit / RCM / Gorder on a graph with communities):
            # the XCD-contiguous chunk ranges then already keep neighbours in one L2 and the column slicing the
            # automatic rule picks for UNORDERED graphs of this size can lose to the plain pass (planted
            # partition, n = 60 k, Rabbit: 0.55 ms unsliced, 0.73 ms sliced).  Measure once, keep the faster.
            self.tuning = self.adj.autotune(k=max(self.hidden_sizes[0], 64))
        self.vo_mp = vo_mp
        self._ax = None
        self.features = gather_rows(features.to(dev), self.vo_mp)                # step 4
        self.labels = torch.as_tensor(np.asarray(labels), dtype=torch.int64).to(dev)[self.vo_mp.long()]
        inv = torch.empty(n, dtype=torch.int64)
        inv[vo_mp.cpu().long()] = torch.arange(n)
        self._new_index = inv                 # old vertex id -> row in the renumbered graph (gcn6.py:255-260)
        return self

    def fit(self, features, adj, labels, idx_train, train_iters=200, initialize=True, verbose=False,
            normalize=True, reuse_prepared=False, hip_graph=False):
        """gcn6.fit (gcn6.py:262-410).  hip_graph=True: the training step — forward, loss, backward, Adam — is captured
        once in a HIP graph after three eager iterations and replayed for the rest: for graphs small enough that an epoch
        is a few dozen launch-bound kernels (Cora-, Pubmed-shaped), where the launches, not the kernels, set the pace."""
        if hip_graph and self.compute_dtype != torch.float32:
            raise ValueError("hip_graph=True with compute_dtype=torch.bfloat16: not supported yet")
        if initialize:
            self.initialize()
        if not (reuse_prepared and self.adj is not None):   # (a second fit on the same graph keeps steps 1-4)
            self.prepare(features, adj, labels, normalize)
        idx = self._new_index[torch.as_tensor(np.asarray(idx_train)).long()].to(self.labels.device)
        self.train()
        if hip_graph:
            return self._fit_captured(idx, train_iters, verbose)
        opt = torch.optim.Adam(self.parameters(), lr=self.lr, weight_decay=self.weight_decay)
        ti = timers.Timers()
        losses = []
        for i in range(train_iters):
            opt.zero_grad()
            with ti.h.fwd:
                output = self.forward(self.features, self.adj)
            loss = F.nll_loss(output[idx], self.labels[idx])
            with ti.h.bwd:
                loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
            if verbose and i % 10 == 0:
                print(f"Epoch {i:3d}, training loss: {losses[-1]:.6f}  Fwd: {ti.h.fwd.avms():.3f} ms/iter"
                      f"  Bwd: {ti.h.bwd.avms():.3f} ms/iter")
                ti.reset()
        self.output = output.detach()       # (detached: a live autograd graph would keep this run's AccumulateGrad nodes —
        return losses                       #  and the stream they were made on — alive into the next fit, see _fit_captured)

    def _fit_captured(self, idx, train_iters, verbose):
        dev = self.labels.device
        # Nothing may keep an autograd graph of an earlier (eager, default-stream) run alive: its AccumulateGrad nodes would
        # be reused, and their work on the default stream inside the capture is what hipStreamEndCapture dies of.
        self.output = None
        for p_ in self.parameters():
            p_.grad = None
        opt = torch.optim.Adam(self.parameters(), lr=self.lr, weight_decay=self.weight_decay, capturable=True)
        target = self.labels[idx]
        losses = torch.zeros(train_iters, dtype=torch.float32, device=dev)

        def step():
            output = self.forward(self.features, self.adj)
            loss = F.nll_loss(output[idx], target)
            loss.backward()
            opt.step()
            return output, loss

        # eager iterations first, on the stream the capture will use: every workspace of the SpMM plans (forward and
        # backward widths) and Adam's state exist before the capture begins
        warm = min(3, train_iters)
        cur = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(dev)
        side.wait_stream(cur)
        output = None
        with torch.cuda.stream(side):
            for i in range(warm):
                opt.zero_grad(set_to_none=True)
                output, loss = step()
                losses[i] = loss.detach()
            if train_iters > warm:
                opt.zero_grad(set_to_none=True)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=side):
                    output, loss = step()
                for i in range(warm, train_iters):
                    graph.replay()
                    losses[i].copy_(loss.detach())
        cur.wait_stream(side)
        self.output = output.detach() if output is not None else None
        out = [float(v) for v in losses.tolist()]           # one synchronisation, at the end
        if verbose:
            print(f"captured fit: {train_iters} iterations ({warm} eager), loss {out[0]:.6f} -> {out[-1]:.6f}")
        return out

    def timing_report(self):
        """the per-layer lines gcn6 prints after fit (gcn6.py:401-410)"""
        lines = [f"Forward time: {self.dur_fwd.s():.4f} s for {self.dur_fwd.n_calls} calls."]
        for gc in (self.gc1, self.gc2):
            t = gc.timers
            lines.append(f"{gc.layer} xw: {t.h.xw.avms():6.4f} ms  cu {t.c.xw.avms():6.4f} ms "
                         f" af: {t.h.af.avms():7.4f} ms  cu {t.c.af.avms():7.4f} ms "
                         f" bi: {t.h.bi.avms():7.4f} ms  cu {t.c.bi.avms():7.4f} ms")
        return "\n".join(lines)

    @torch.no_grad()
    def predict(self):
        """log-probabilities in the ORIGINAL vertex order"""
        self.eval()
        out = self.forward(self.features, self.adj)
        return out[self._new_index.to(out.device)]

    def test(self, idx_test, labels):
        out = self.predict()
        idx = torch.as_tensor(np.asarray(idx_test)).long().to(out.device)
        lab = torch.as_tensor(np.asarray(labels), dtype=torch.int64).to(out.device)
        return preprocess.accuracy(out[idx], lab[idx])
