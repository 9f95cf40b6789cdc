"""All attention heads in one pass (gcn_amd/csrc/edge_softmax.hip, multihead.hip) on the GPU, against the fp64 twins of tests/heads_ref.py.

* spmm_heads (forward and the transposed form through its permutation) and sddmm_heads: bit for bit on an exact grid (x
  integers in [-3, 3], values eighths in [0, 7/8]: every partial sum of at most 300 000 terms is below 2^24 eighths, so any
  correct order gives the same bits and any dropped, doubled or misrouted entry shows), and within the project's standing
  1e-5 * sum|terms| + 1e-30 on random fp32 inputs; so is segment_sum.
* the per-head softmax family, plain and fused, forward and backward, on every entry, with the bounds of DESIGN §4.9 and
  the longest addition path A(len, H) of these kernels, derived from the code:
    fast route (H a power of two <= 16): a row of at most 8192 entries is summed by one wave whose lanes each own one head
      and ceil(len H / 64) of its elements, then a butterfly of at most 6 steps: A = ceil(len H / 64) + 6 (the 8-lane form
      of short rows, <= 4 + 3, is below that); a longer row by 256-thread blocks per chunk of 8192 entries, 32 H elements
      a thread, a butterfly and the 4 waves (<= 6 + 3), then the row's nc <= ceil(len / 8192) + 1 chunk partials
      (ceil(nc / 256) a thread + 6 + 3): A = 32 H + 9 + ceil(nc / 256) + 9;
    slow route (any other H): the single-head kernel's path per head, the formula above with H = 1.
* head isolation, determinism, aliasing, capture, operands shifted by one element, autograd against fp64 dense autograd,
  the GraphAttention(head_batched=True) layer against a dense fp64 GAT and against the loop form, a seeded sweep."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F_

import gcn_amd
import heads_ref
from gcn_amd import graphgen
from util import random_csr, rel_err

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
DEV = "cuda:0"
CHUNK = 8192
SHAPES = [(1, 16), (2, 4), (8, 8), (8, 16), (4, 64), (3, 5), (8, 1), (16, 4)]
HEADS = sorted({h for h, _f in SHAPES})
GRAPHS = ["cora", "hubs", "empty_tail", "boundaries"]


def A_of(lens, H):
    """additions on the longest path of a (row, head) sum: see the module docstring"""
    lens = np.asarray(lens, np.float64)
    hp = H if H <= 16 and H & (H - 1) == 0 else 1
    nc = np.ceil(lens / CHUNK) + 1
    return np.where(lens <= CHUNK, np.ceil(lens * hp / 64) + 6, 32 * hp + 9 + np.ceil(nc / 256) + 9)


# ---- graphs ----------------------------------------------------------------------------------------------------------------
def _csr_from_lens(lens, n, seed, popular=None):
    rng = np.random.default_rng(seed)
    rowptr = np.zeros(len(lens) + 1, np.int64)
    rowptr[1:] = np.cumsum(lens)
    col = rng.integers(0, n, rowptr[-1]).astype(np.int32)      # (duplicates allowed: each stored entry is its own)
    if popular is not None:                                     # a long row of the transposed pattern too
        col[rng.random(len(col)) < 0.05] = popular
    return rowptr.astype(np.int32), col, n


# every branch of both dispatches, a row on both sides of each threshold: the single-head list (1 | 32 | 256 | 1024 | 8192
# elements, here reached at len = threshold / H for H = 1 .. 16), the chunk of the gather kernels (4096) and its multiples
BOUNDARY_LENS = [1, 5, 0, 32, 33, 64, 0, 0, 256, 257, 300, 1024, 1025, 5000, 8192, 8193, 20000, 0, 3, 2, 1, 0, 0, 0, 0, 0, 7,
                 16385, 31, 32, 1, 1, 1, 4, 0, 16384, 8191, 2, 4095, 4096, 4097, 12289, 8, 9, 16, 17, 65, 128, 129, 512, 513,
                 10, 11, 85, 86, 341, 342]


class Graph:
    _cache = {}

    def __init__(self, rowptr, col, n, live=None):
        self.rowptr, self.col, self.n = rowptr.astype(np.int32), col.astype(np.int32), int(n)
        self.m, self.nnz = len(rowptr) - 1, len(col)
        self.live = self.m if live is None else live           # rows from `live` on are empty
        self.rp_live = self.rowptr[:self.live + 1]
        self.lens = np.diff(self.rp_live.astype(np.int64))
        self.row = heads_ref.entry_rows(self.rp_live)
        self.len_e = self.lens[self.row]
        self._t = self._adj = self._dev_t = None

    @classmethod
    def get(cls, name):
        if name in cls._cache:
            return cls._cache[name]
        if name == "cora":
            rp, col, _v, n = graphgen.make_graph("cora", device="cpu", seed=1)
            g = cls(rp.numpy(), col.numpy(), n)
        elif name == "hubs":                               # 30 % empty rows, hub rows of 5 000 and 300 000 entries
            # (20 000 columns, repeats allowed, so that the gathered operand stays small at k = 256; 5 % of the entries
            # name column 3: a row of about 16 000 entries in the transposed pattern, long for both dispatches)
            rng = np.random.default_rng(5)
            lens = rng.poisson(10, 3000)
            lens[rng.random(3000) < 0.3] = 0
            lens[7], lens[1500] = 5000, 300000
            g = cls(*_csr_from_lens(lens, 20000, 6, popular=3))
        elif name == "empty_tail":                         # the last million rows are empty
            lens = np.concatenate([np.random.default_rng(3).poisson(40, 2000), np.zeros(1_000_000, np.int64)])
            g = cls(*_csr_from_lens(lens, 5000, 4), live=2000)
        elif name == "boundaries":
            g = cls(*_csr_from_lens(np.array(BOUNDARY_LENS, np.int64), 50000, 6))
        else:
            raise KeyError(name)
        cls._cache[name] = g
        return g

    @property
    def adj(self):
        if self._adj is None:
            self._adj = gcn_amd.CsrAdjacency(torch.from_numpy(self.rowptr).to(DEV), torch.from_numpy(self.col).to(DEV),
                                             torch.ones(self.nnz, device=DEV), (self.m, self.n))
        return self._adj

    @property
    def t(self):
        """host transposed pattern (trowptr, trow, tperm)"""
        if self._t is None:
            self._t = heads_ref.transpose_pattern(self.rp_live, self.col, self.n)
        return self._t

    def A_e(self, H):
        return A_of(self.len_e, H)[:, None]


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def node_rows(g, live_rows, width):
    """a [g.m, width] device tensor whose first g.live rows are `live_rows` (rows past that have no entry: zeros)"""
    if g.live == g.m:
        return dev(live_rows)
    out = torch.zeros(g.m, width, device=DEV)
    out[:g.live] = dev(live_rows)
    return out


def assert_rows_equal(g, got, ref_live, what):
    ref32 = ref_live.astype(np.float32)
    assert np.array_equal(ref32.astype(np.float64), ref_live), "the reference is not on the fp32 grid"
    assert torch.equal(got[:g.live], dev(ref32)), what
    assert int(torch.count_nonzero(got[g.live:])) == 0, what + " (empty tail)"


def assert_rows_close(g, got, ref_live, mag_live, what):
    err = np.abs(got[:g.live].cpu().numpy().astype(np.float64) - ref_live)
    ratio = float((err / (1e-5 * mag_live + 1e-30)).max()) if err.size else 0.0
    print(f"[heads] {what}: max error / bound = {ratio:.4f}")
    assert ratio <= 1.0, (what, ratio)
    assert int(torch.count_nonzero(got[g.live:])) == 0, what + " (empty tail)"


def grid_inputs(g, H, F, seed):
    rng = np.random.default_rng(seed)
    k = H * F
    x = rng.integers(-3, 4, (g.n, k)).astype(np.float32)
    a = rng.integers(-3, 4, (g.live, k)).astype(np.float32)
    vals = (rng.integers(0, 8, (g.nnz, H)) / 8.0).astype(np.float32)
    return x, a, vals


# ---- 1. exact arithmetic through the public functions and their autograd ---------------------------------------------------------
@pytest.mark.parametrize("H,F", SHAPES)
@pytest.mark.parametrize("name", GRAPHS)
def test_spmm_and_sddmm_are_exact_on_the_grid(name, H, F):
    g = Graph.get(name)
    x, a, vals = grid_inputs(g, H, F, seed=H * 100 + F)
    xd, vd, ad = dev(x).requires_grad_(True), dev(vals).requires_grad_(True), node_rows(g, a, H * F)
    out = gcn_amd.spmm_heads(g.adj, xd, vd)
    out.backward(ad)                                       # x.grad: the transposed form; vals.grad: the SDDMM of (a, x)
    sd = gcn_amd.sddmm_heads(g.adj, ad, xd.detach(), H)
    trp, trow, tperm = g.t
    assert_rows_equal(g, out.detach(), heads_ref.spmm_heads(g.rp_live, g.col, None, vals, x, H), f"spmm_heads {name} {H}x{F}")
    gx_ref = heads_ref.spmm_heads(trp, trow, tperm, vals, a, H)
    assert torch.equal(xd.grad, dev(gx_ref.astype(np.float32))) and np.array_equal(gx_ref.astype(np.float32), gx_ref)
    sd_ref = heads_ref.sddmm_heads(g.rp_live, g.col, a, x, H)
    assert np.array_equal(sd_ref.astype(np.float32), sd_ref)
    assert torch.equal(sd, dev(sd_ref.astype(np.float32))), f"sddmm_heads {name} {H}x{F}"
    assert torch.equal(vd.grad, sd), "the gradient with respect to the values is the SDDMM"


# ---- 2. random fp32 inputs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,F", SHAPES)
@pytest.mark.parametrize("name", GRAPHS)
def test_spmm_and_sddmm_random_inputs_keep_the_standing_bound(name, H, F):
    g = Graph.get(name)
    rng = np.random.default_rng(H * 7 + F)
    k = H * F
    x = rng.standard_normal((g.n, k)).astype(np.float32)
    a = rng.standard_normal((g.live, k)).astype(np.float32)
    vals = rng.standard_normal((g.nnz, H)).astype(np.float32)
    xd, vd, ad = dev(x).requires_grad_(True), dev(vals).requires_grad_(True), node_rows(g, a, k)
    out = gcn_amd.spmm_heads(g.adj, xd, vd)
    out.backward(ad)
    trp, trow, tperm = g.t
    ax, aa, av = np.abs(x), np.abs(a), np.abs(vals)
    assert_rows_close(g, out.detach(), heads_ref.spmm_heads(g.rp_live, g.col, None, vals, x, H),
                      heads_ref.spmm_heads(g.rp_live, g.col, None, av, ax, H), f"spmm_heads {name} {H}x{F}")
    gx = heads_ref.spmm_heads(trp, trow, tperm, vals, a, H)
    gmag = heads_ref.spmm_heads(trp, trow, tperm, av, aa, H)
    r = float((np.abs(xd.grad.cpu().numpy() - gx) / (1e-5 * gmag + 1e-30)).max())
    print(f"[heads] spmm_heads transposed {name} {H}x{F}: max error / bound = {r:.4f}")
    assert r <= 1.0
    sd, smag = heads_ref.sddmm_heads(g.rp_live, g.col, a, x, H), heads_ref.sddmm_heads(g.rp_live, g.col, aa, ax, H)
    r = float((np.abs(vd.grad.cpu().numpy() - sd) / (1e-5 * smag + 1e-30)).max())
    print(f"[heads] sddmm_heads {name} {H}x{F}: max error / bound = {r:.4f}")
    assert r <= 1.0


@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("name", GRAPHS)
def test_segment_sum_heads_matches_fp64(name, H):
    g = Graph.get(name)
    x = torch.randn(g.nnz, H, generator=torch.Generator().manual_seed(10 + H))
    perm = torch.randperm(g.nnz, generator=torch.Generator().manual_seed(11))
    rpd = g.adj.rowptr
    out = gcn_amd.segment_sum(rpd, x.to(DEV))
    outp = gcn_amd.segment_sum(rpd, x.to(DEV), perm=perm.to(DEV, torch.int32))
    assert out.shape == (g.m, H) and torch.equal(out, gcn_amd.segment_sum(rpd, x.to(DEV)))
    x64 = x.numpy().astype(np.float64)
    for got, p, what in ((out, None, "plain"), (outp, perm.numpy(), "permuted")):
        assert_rows_close(g, got, heads_ref.segment_sum(g.rp_live, x64, p), heads_ref.segment_sum(g.rp_live, np.abs(x64), p),
                          f"segment sum {name} H={H} {what}")
    if H == 1:                                             # the one-head 2-D form and the 1-D form are the same numbers
        one = gcn_amd.segment_sum(rpd, x[:, 0].contiguous().to(DEV))
        assert torch.equal(one[:, None], out)
        assert_rows_close(g, one[:, None], heads_ref.segment_sum(g.rp_live, x64), heads_ref.segment_sum(g.rp_live, np.abs(x64)),
                          f"segment sum {name} 1-D")


# ---- 3. the softmax family -------------------------------------------------------------------------------------------------------
def check_forward(g, H, s32, p32, what):
    pref = heads_ref.edge_softmax(g.rp_live, s32)
    s64 = s32.astype(np.float64)
    ne = g.lens > 0
    starts = g.rp_live[:-1][ne].astype(np.int64)
    rng_r = np.zeros((g.live, H))
    rng_r[ne] = np.maximum.reduceat(s64, starts, axis=0) - np.minimum.reduceat(s64, starts, axis=0)
    rng_e = rng_r[g.row]
    assert float(rng_e.max()) <= 16.0 + 1e-3, "the bound is meaningful for R <= 16"
    bound = EPS * (4 * rng_e + 2 * g.A_e(H) + 8) * pref + 1e-38
    ratio = float((np.abs(p32.astype(np.float64) - pref) / bound).max())
    print(f"[heads] forward {what}: max error / bound = {ratio:.4f} over {pref.size} elements")
    assert ratio <= 1.0, (what, ratio)
    sums = heads_ref.row_sums(g.rp_live, p32)[ne]
    srat = float((np.abs(sums - 1.0) / (EPS * (A_of(g.lens[ne], H)[:, None] + 4))).max())
    print(f"[heads] row sums {what}: max |sum - 1| / bound = {srat:.4f}")
    assert srat <= 1.0, (what, srat)


def scores_for(g, H, seed=0):
    return (torch.rand(g.nnz, H, generator=torch.Generator().manual_seed(seed)) * 16 - 8).to(DEV)


def gat_inputs(g, H, seed=1):
    gen = torch.Generator().manual_seed(seed)
    a_dst = torch.zeros(g.m, H)
    a_dst[:g.live] = torch.rand(g.live, H, generator=gen) * 8 - 4
    return a_dst.to(DEV), (torch.rand(g.n, H, generator=gen) * 8 - 4).to(DEV)


def ds_bound(g, H, p32, g32):
    p, gg = p32.astype(np.float64), g32.astype(np.float64)
    return EPS * (g.A_e(H) + 6) * p * (np.abs(gg) + heads_ref.row_sums(g.rp_live, p * np.abs(gg))[g.row]) + 1e-38


@pytest.mark.parametrize("H", HEADS)
@pytest.mark.parametrize("name", GRAPHS)
def test_edge_softmax_heads_forward_and_backward_match_fp64(name, H):
    g = Graph.get(name)
    s = scores_for(g, H, seed=H).requires_grad_(True)
    p = gcn_amd.edge_softmax(g.adj, s)
    assert p.shape == (g.nnz, H)
    gout = torch.randn(g.nnz, H, generator=torch.Generator().manual_seed(7)).to(DEV)
    p.backward(gout)
    pn, gn = p.detach().cpu().numpy(), gout.cpu().numpy()
    check_forward(g, H, s.detach().cpu().numpy(), pn, f"{name} H={H}")
    ratio = float((np.abs(s.grad.cpu().numpy() - heads_ref.edge_softmax_backward(g.rp_live, pn, gn)) / ds_bound(g, H, pn, gn)).max())
    print(f"[heads] backward {name} H={H}: max error / bound = {ratio:.4f}")
    assert ratio <= 1.0, (name, H, ratio)


@pytest.mark.parametrize("H,slope", [(h, 0.2) for h in HEADS] + [(8, 1.5), (3, 1.5)])
@pytest.mark.parametrize("name", GRAPHS)
def test_gat_edge_softmax_heads_forward_and_backward_match_fp64(name, H, slope):
    g = Graph.get(name)
    a_dst, a_src = gat_inputs(g, H, seed=8 + H)
    if name == "boundaries":                               # pre-activations of exactly 0: the derivative there is the slope
        a_dst[4] = 0.0
        a_src[dev(g.col[g.rowptr[4]:g.rowptr[4] + 10], torch.int64)] = 0.0
    a_dst.requires_grad_(True)
    a_src.requires_grad_(True)
    p = gcn_amd.gat_edge_softmax(g.adj, a_dst, a_src, slope)
    gout = torch.randn(g.nnz, H, generator=torch.Generator().manual_seed(9)).to(DEV)
    p.backward(gout)
    adn, asn = a_dst.detach().cpu().numpy()[:g.live], a_src.detach().cpu().numpy()
    pn, gn = p.detach().cpu().numpy(), gout.cpu().numpy()
    s32 = heads_ref.gat_scores(g.rp_live, g.col, adn, asn, slope)
    check_forward(g, H, s32, pn, f"{name} H={H} slope={slope} (fused)")
    # ds through the raw call (the autograd keeps it to itself), bit-identical over two runs
    ds, gd = raw_gat_backward(g.adj, a_dst.detach(), a_src.detach(), slope, p.detach(), gout)
    assert torch.equal(gd, a_dst.grad)
    ds_ref, gd_ref = heads_ref.gat_edge_softmax_backward(g.rp_live, g.col, adn, asn, slope, pn, gn)
    ratio = float((np.abs(ds.cpu().numpy() - ds_ref) / (ds_bound(g, H, pn, gn) * max(1.0, slope))).max())
    print(f"[heads] fused backward {name} H={H} slope={slope}: max error / bound = {ratio:.4f}")
    assert ratio <= 1.0, (name, H, ratio)
    assert_rows_close(g, a_dst.grad, gd_ref, heads_ref.row_sums(g.rp_live, np.abs(ds_ref)), f"grad_a_dst {name} H={H}")
    trp, _trow, tperm = g.t
    gs_ref, gs_mag = heads_ref.segment_sum(trp, ds_ref, tperm), heads_ref.segment_sum(trp, np.abs(ds_ref), tperm)
    r_src = float((np.abs(a_src.grad.cpu().numpy() - gs_ref) / (1e-5 * gs_mag + 1e-30)).max())
    print(f"[heads] grad_a_src {name} H={H}: max error / bound = {r_src:.4f}")
    assert r_src <= 1.0


@pytest.mark.parametrize("shift", [1e4, -1e4])
@pytest.mark.parametrize("H", [8, 3])
@pytest.mark.parametrize("name", ["boundaries", "hubs"])
def test_shifted_scores_keep_the_bound(name, H, shift):
    g = Graph.get(name)
    s = scores_for(g, H, seed=2) + shift                   # (rounded to fp32: the reference sees the same inputs)
    p = gcn_amd.edge_softmax(g.adj, s)
    check_forward(g, H, s.cpu().numpy(), p.cpu().numpy(), f"{name} H={H} shifted by {shift:+.0e}")


@pytest.mark.parametrize("H", [4, 3, 16])
def test_a_head_of_nan_or_minus_inf_leaves_the_other_heads_their_bits(H):
    g = Graph.get("boundaries")
    s = scores_for(g, H, seed=4)
    clean = gcn_amd.edge_softmax(g.adj, s)
    others = [h for h in range(H) if h != 1]
    for bad in (float("nan"), float("-inf")):
        s2 = s.clone()
        s2[:, 1] = bad
        p = gcn_amd.edge_softmax(g.adj, s2)
        assert torch.equal(p[:, others], clean[:, others]), bad
        if bad != bad:
            assert bool(torch.isnan(p[:, 1]).all())
        else:
            assert int(torch.count_nonzero(p[:, 1])) == 0 and not bool(torch.isnan(p).any())   # all -inf: exact zeros
    # one NaN entry poisons its own (row, head); an all -inf (row, head) gives zeros — rows of 1, 32, 300, 5000, 20000, 16385
    rows = [0, 3, 10, 13, 16, 27]
    s3, s4 = s.clone(), s.clone()
    hit = torch.zeros(g.nnz, H, dtype=torch.bool, device=DEV)
    for r in rows:
        b, e = int(g.rowptr[r]), int(g.rowptr[r + 1])
        s3[b + (2 * (e - b)) // 3, H - 1] = float("nan")
        s4[b:e, 0] = float("-inf")
        hit[b:e, H - 1] = True
    p3, p4 = gcn_amd.edge_softmax(g.adj, s3), gcn_amd.edge_softmax(g.adj, s4)
    assert bool(torch.isnan(p3[hit]).all()) and torch.equal(p3[~hit], clean[~hit])
    hit0 = torch.zeros_like(hit)
    for r in rows:
        hit0[int(g.rowptr[r]):int(g.rowptr[r + 1]), 0] = True
    assert int(torch.count_nonzero(p4[hit0])) == 0 and torch.equal(p4[~hit0], clean[~hit0])
    # the fused form: a head whose a_src is NaN
    a_dst, a_src = gat_inputs(g, H, seed=5)
    pc = gcn_amd.gat_edge_softmax(g.adj, a_dst, a_src, 0.2)
    a_bad = a_src.clone()
    a_bad[:, 1] = float("nan")
    pb = gcn_amd.gat_edge_softmax(g.adj, a_dst, a_bad, 0.2)
    assert torch.equal(pb[:, others], pc[:, others]) and bool(torch.isnan(pb[:, 1]).all())


# ---- raw calls (operands and outputs of the caller's choosing) -------------------------------------------------------------------
def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def shifted(t, by=1):
    """the same values in a view that starts `by` elements into its storage (by = 1: 4 bytes off every 16-byte boundary)"""
    if t is None or by == 0:
        return t
    buf = torch.empty(t.numel() + by, dtype=t.dtype, device=t.device)
    v = buf[by:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (buf.data_ptr() + by * t.element_size()) % 16 and v.is_contiguous()
    return v


def raw_ws(m, nnz, H, k):
    need = ctypes.c_size_t(0)
    assert gcn_amd.load_library().gcn_heads_ws_bytes(m, nnz, H, k, ctypes.byref(need)) == 0
    return torch.empty(need.value, dtype=torch.uint8, device=DEV)


def raw_gat_backward(adj, a_dst, a_src, slope, p, gout, by=0):
    H = p.shape[1]
    ds, gd = shifted(torch.empty_like(p), by), shifted(torch.empty(adj.m, H, device=DEV), by)
    ws = raw_ws(adj.m, adj.nnz, H, H)
    st = gcn_amd.load_library().gcn_gat_edge_softmax_heads_backward_csr_f32(
        vp(adj.rowptr), vp(adj.col), adj.m, adj.nnz, H, vp(a_dst), vp(a_src), slope, vp(p), vp(gout), vp(ds), vp(gd), vp(ws),
        ws.numel(), stream())
    torch.cuda.synchronize()                               # (the workspace is this function's)
    assert st == 0
    return ds, gd


class RawProblem:
    """a CSR pattern and its transpose on the device, every array shifted by `by` elements"""

    def __init__(self, rowptr, col, n, by):
        self.m, self.n, self.nnz, self.by = len(rowptr) - 1, n, len(col), by
        trp, trow, tperm = heads_ref.transpose_pattern(rowptr, col, n)
        self.host = (rowptr, col, trp, trow, tperm)
        self.rowptr, self.col, self.trp, self.trow, self.tperm = (shifted(dev(a, torch.int32), by) for a in self.host)
        self.lib = gcn_amd.load_library()

    def ws(self, H, k):
        return raw_ws(max(self.m, self.n), self.nnz, H, k)

    def spmm(self, vals, x, H, transposed=False):
        by, k = self.by, x.shape[1]
        rows = self.n if transposed else self.m
        out = shifted(torch.full((rows, k), float("nan"), device=DEV), by)
        ws = self.ws(H, k)
        rp, idx, perm = (self.trp, self.trow, self.tperm) if transposed else (self.rowptr, self.col, None)
        vs, xs = shifted(vals, by), shifted(x, by)         # (held until the call has run)
        st = self.lib.gcn_spmm_heads_csr_f32(vp(rp), vp(idx), vp(perm), rows, self.nnz, H, k, vp(vs), vp(xs), vp(out), vp(ws),
                                             ws.numel(), stream())
        torch.cuda.synchronize()
        assert st == 0
        return out

    def sddmm(self, a, b, H):
        by = self.by
        out = shifted(torch.full((self.nnz, H), float("nan"), device=DEV), by)
        ws = self.ws(H, a.shape[1])
        as_, bs = shifted(a, by), shifted(b, by)           # (held until the call has run)
        st = self.lib.gcn_sddmm_heads_csr_f32(vp(self.rowptr), vp(self.col), self.m, self.nnz, H, a.shape[1], vp(as_), vp(bs),
                                              vp(out), vp(ws), ws.numel(), stream())
        torch.cuda.synchronize()
        assert st == 0
        return out

    def exact(self, H, F, seed, what):
        """the three gather operations on the exact grid, bit for bit against the fp64 twins"""
        rowptr, col, trp, trow, tperm = self.host
        rng = np.random.default_rng(seed)
        k = H * F
        x = rng.integers(-3, 4, (self.n, k)).astype(np.float32)
        a = rng.integers(-3, 4, (self.m, k)).astype(np.float32)
        vals = (rng.integers(0, 8, (self.nnz, H)) / 8.0).astype(np.float32)
        for got, ref, op in (
                (self.spmm(dev(vals), dev(x), H), heads_ref.spmm_heads(rowptr, col, None, vals, x, H), "spmm"),
                (self.spmm(dev(vals), dev(a), H, transposed=True), heads_ref.spmm_heads(trp, trow, tperm, vals, a, H), "spmm T"),
                (self.sddmm(dev(a), dev(x), H), heads_ref.sddmm_heads(rowptr, col, a, x, H), "sddmm")):
            ref32 = ref.astype(np.float32)
            assert np.array_equal(ref32, ref), "the reference is not on the fp32 grid"
            if self.nnz == 0 and op != "sddmm":
                continue                                   # (nothing is launched and nothing written: the caller zeroes)
            assert torch.equal(got, dev(ref32)), f"{what}: {op} H={H} F={F} shifted by {self.by}"


# ---- 4. misaligned operands ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,F", SHAPES)
@pytest.mark.parametrize("name", ["cora", "boundaries"])
def test_gather_kernels_with_every_operand_shifted_by_one_element_are_exact(name, H, F):
    g = Graph.get(name)
    RawProblem(g.rowptr, g.col, g.n, by=1).exact(H, F, seed=3 * H + F, what=name)


@pytest.mark.parametrize("H,F", [(8, 8), (4, 64), (3, 5)])
def test_gather_kernels_shifted_keep_the_standing_bound(H, F):
    g = Graph.get("boundaries")
    P = RawProblem(g.rowptr, g.col, g.n, by=1)
    rng = np.random.default_rng(H + F)
    k = H * F
    x, a = rng.standard_normal((g.n, k)).astype(np.float32), rng.standard_normal((g.m, k)).astype(np.float32)
    vals = rng.standard_normal((g.nnz, H)).astype(np.float32)
    rowptr, col, trp, trow, tperm = P.host
    ax, aa, av = np.abs(x), np.abs(a), np.abs(vals)
    for got, ref, mag, op in (
            (P.spmm(dev(vals), dev(x), H), heads_ref.spmm_heads(rowptr, col, None, vals, x, H),
             heads_ref.spmm_heads(rowptr, col, None, av, ax, H), "spmm"),
            (P.spmm(dev(vals), dev(a), H, True), heads_ref.spmm_heads(trp, trow, tperm, vals, a, H),
             heads_ref.spmm_heads(trp, trow, tperm, av, aa, H), "spmm T"),
            (P.sddmm(dev(a), dev(x), H), heads_ref.sddmm_heads(rowptr, col, a, x, H), heads_ref.sddmm_heads(rowptr, col, aa, ax, H),
             "sddmm")):
        r = float((np.abs(got.cpu().numpy() - ref) / (1e-5 * mag + 1e-30)).max())
        print(f"[heads] shifted {op} {H}x{F}: max error / bound = {r:.4f}")
        assert r <= 1.0, (op, r)


@pytest.mark.parametrize("H,F", [(8, 40), (3, 25)])
def test_spmm_heads_second_column_tile_with_long_rows(H, F):
    """chunk partials in a column tile past the first (gather_rows.h: plane t, row 2 c + slot, column j of the tile
    blockIdx.y): k = 320 is a quarter of a second 256-column tile at VEC = 4 (five 64-column tiles once shifted), k = 75
    puts 11 columns into a second 64-column tile; rows on both sides of the chunk and of one, two and three chunks"""
    rowptr, col, n = _csr_from_lens(np.array([0, 1, 4095, 4096, 4097, 8193, 12289, 3], np.int64), 50000, 6)
    rng = np.random.default_rng(H + F)
    k = H * F
    x = dev(rng.integers(-3, 4, (n, k)).astype(np.float32))
    a = dev(rng.integers(-3, 4, (len(rowptr) - 1, k)).astype(np.float32))
    vals = dev((rng.integers(0, 8, (len(col), H)) / 8.0).astype(np.float32))
    for by in (0, 1):
        P = RawProblem(rowptr, col, n, by=by)
        P.exact(H, F, seed=5 * H + F, what="second column tile")
        assert torch.equal(P.spmm(vals, x, H), P.spmm(vals, x, H)), f"two calls, shifted by {by}"
        assert torch.equal(P.spmm(vals, a, H, transposed=True), P.spmm(vals, a, H, transposed=True)), f"two calls (T), shifted by {by}"


@pytest.mark.parametrize("H", [8, 3])
def test_softmax_family_with_every_operand_shifted_by_one_element(H):
    """these kernels use element accesses only: a shifted operand must give the bits of the aligned call, whose bounds the
    tests above check — plain and fused softmax, their backwards and the segment sum"""
    g = Graph.get("boundaries")
    adj, lib = g.adj, gcn_amd.load_library()
    s, gout = scores_for(g, H, seed=6), torch.randn(g.nnz, H, generator=torch.Generator().manual_seed(3)).to(DEV)
    a_dst, a_src = gat_inputs(g, H, seed=7)
    perm = torch.randperm(g.nnz, generator=torch.Generator().manual_seed(2)).to(DEV, torch.int32)
    sg = s.clone().requires_grad_(True)
    p = gcn_amd.edge_softmax(adj, sg)
    p.backward(gout)
    pf = gcn_amd.gat_edge_softmax(adj, a_dst, a_src, 0.2)
    ds_f, gd_f = raw_gat_backward(adj, a_dst, a_src, 0.2, pf, gout)
    seg = gcn_amd.segment_sum(adj.rowptr, s, perm=perm)
    rp, col = shifted(adj.rowptr), shifted(adj.col)
    ws = raw_ws(g.m, g.nnz, H, H)                          # (the workspace keeps its 16-byte alignment: the ABI asks for it)
    new = lambda *shape: shifted(torch.full(shape, float("nan"), device=DEV))
    p2, ds2, pf2, seg2 = new(g.nnz, H), new(g.nnz, H), new(g.nnz, H), new(g.m, H)
    ss, ps, gs, ads, ass, pfs, perms = (shifted(t) for t in (s, p.detach(), gout, a_dst, a_src, pf, perm))   # (held to the end)
    assert lib.gcn_edge_softmax_heads_csr_f32(vp(rp), g.m, g.nnz, H, vp(ss), vp(p2), vp(ws), ws.numel(), stream()) == 0
    assert lib.gcn_edge_softmax_heads_backward_csr_f32(vp(rp), g.m, g.nnz, H, vp(ps), vp(gs), vp(ds2), vp(ws), ws.numel(),
                                                       stream()) == 0
    assert lib.gcn_gat_edge_softmax_heads_csr_f32(vp(rp), vp(col), g.m, g.nnz, H, vp(ads), vp(ass), 0.2, vp(pf2), vp(ws), ws.numel(),
                                                  stream()) == 0
    assert lib.gcn_segment_sum_heads_csr_f32(vp(rp), g.m, g.nnz, H, vp(ss), vp(perms), vp(seg2), vp(ws), ws.numel(), stream()) == 0
    ds_f2, gd_f2 = raw_gat_backward(adj, ads, ass, 0.2, pfs, gs, by=1)
    torch.cuda.synchronize()
    assert torch.equal(p2, p.detach()) and torch.equal(ds2, sg.grad) and torch.equal(pf2, pf) and torch.equal(seg2, seg)
    assert torch.equal(ds_f2, ds_f) and torch.equal(gd_f2, gd_f)


# ---- 5. determinism, aliasing, capture -------------------------------------------------------------------------------------------
def test_two_calls_are_bit_identical_and_p_may_alias_scores():
    for name, H, F in (("boundaries", 8, 8), ("hubs", 3, 5), ("hubs", 16, 4)):
        g = Graph.get(name)
        adj = g.adj
        s = scores_for(g, H, seed=5)
        x = torch.randn(g.n, H * F, generator=torch.Generator().manual_seed(1)).to(DEV)
        a = torch.randn(g.m, H * F, generator=torch.Generator().manual_seed(2)).to(DEV)

        def run():
            xs, ss = x.clone().requires_grad_(True), s.clone().requires_grad_(True)
            p = gcn_amd.edge_softmax(adj, ss)
            out = gcn_amd.spmm_heads(adj, xs, p)
            out.backward(a)
            return [p.detach(), out.detach(), xs.grad, ss.grad, gcn_amd.sddmm_heads(adj, a, x, H)]

        for u, v in zip(run(), run()):
            assert torch.equal(u, v)
        p1 = gcn_amd.edge_softmax(adj, s)
        buf = s.clone()
        ws = raw_ws(g.m, g.nnz, H, H)
        st = gcn_amd.load_library().gcn_edge_softmax_heads_csr_f32(vp(adj.rowptr), g.m, g.nnz, H, vp(buf), vp(buf), vp(ws), ws.numel(),
                                                                   stream())
        assert st == 0
        torch.cuda.synchronize()
        assert torch.equal(buf, p1)


@pytest.mark.parametrize("name", ["boundaries", "hubs"])
def test_one_head_2d_forms_and_1d_forms_give_the_same_bits(name):
    """[nnz, 1] / [rows, 1] operands and 1-D operands: the 1-D forms are the H = 1 case of the 2-D forms, bit for bit, forward
    and backward, on a row either side of every threshold (boundaries) and on rows of 5 000 and 300 000 entries (hubs)"""
    g = Graph.get(name)
    madj = gcn_amd.CsrAdjacency(g.adj.rowptr, g.adj.col, torch.ones(g.nnz, device=DEV), (g.m, g.n), mutable_values=True)
    gout = torch.randn(g.nnz, 1, generator=torch.Generator().manual_seed(13)).to(DEV)

    def both(f2, f1, ops):
        """[output, gradients ...] of f2 on the 2-D operands and of f1 on their 1-D forms, under the same upstream gradient"""
        res = []
        for f, flat in ((f2, False), (f1, True)):
            leaves = [(o[:, 0].contiguous() if flat else o.clone()).requires_grad_(True) for o in ops]
            out = f(*leaves)
            out.backward(gout[:, 0].contiguous() if flat else gout)
            res.append([out.detach()] + [t.grad for t in leaves])
        return res

    def same(two, one, what):
        assert len(two) == len(one)
        for i, (a, b) in enumerate(zip(two, one)):
            assert a.shape == b.shape + (1,) and torch.equal(a[:, 0], b), (what, i)

    same(*both(lambda s: gcn_amd.edge_softmax(g.adj, s), lambda s: gcn_amd.edge_softmax(g.adj, s), [scores_for(g, 1, seed=3)]),
         "edge_softmax: p, ds")
    a_dst, a_src = gat_inputs(g, 1, seed=4)
    two, one = both(lambda d, s: gcn_amd.gat_edge_softmax(g.adj, d, s, 0.2), lambda d, s: gcn_amd.gat_edge_softmax(madj, d, s, 0.2),
                    [a_dst, a_src])
    same(two, one, "gat_edge_softmax: p, grad_a_dst, grad_a_src")
    ds2, gd2 = raw_gat_backward(g.adj, a_dst, a_src, 0.2, two[0], gout)
    ds1, gd1 = torch.empty(g.nnz, device=DEV), torch.empty(g.m, device=DEV)
    ws = raw_ws(g.m, g.nnz, 1, 1)
    st = gcn_amd.load_library().gcn_gat_edge_softmax_backward_csr_f32(
        vp(g.adj.rowptr), vp(g.adj.col), g.m, g.nnz, vp(a_dst[:, 0].contiguous()), vp(a_src[:, 0].contiguous()), 0.2, vp(one[0]),
        vp(gout[:, 0].contiguous()), vp(ds1), vp(gd1), vp(ws), ws.numel(), stream())
    torch.cuda.synchronize()
    assert st == 0
    same([ds2, gd2], [ds1, gd1], "fused backward: ds, grad_a_dst")
    assert torch.equal(gd1, one[1])
    x = torch.randn(g.nnz, 1, generator=torch.Generator().manual_seed(14)).to(DEV)
    perm = torch.randperm(g.nnz, generator=torch.Generator().manual_seed(15)).to(DEV, torch.int32)
    for pm in (None, perm):
        same([gcn_amd.segment_sum(g.adj.rowptr, x, perm=pm)], [gcn_amd.segment_sum(g.adj.rowptr, x[:, 0].contiguous(), perm=pm)],
             "segment_sum" + (" permuted" if pm is not None else ""))


def _dense_gat(x, mask, weight, att_dst, att_src, bias, heads, out_f, concat, slope):
    """dense fp64 GAT layer: masked softmax over the n x n score matrix"""
    h = x @ weight
    outs = []
    for k in range(heads):
        hk = h[:, k * out_f:(k + 1) * out_f]
        e = F_.leaky_relu((hk @ att_dst[k])[:, None] + (hk @ att_src[k])[None, :], slope)
        e = e.masked_fill(~mask, float("-inf"))
        outs.append(torch.softmax(e, dim=1) @ hk)
    out = torch.cat(outs, 1) if concat else torch.stack(outs).mean(0)
    return out + bias if bias is not None else out


def _cora_problem():
    g = Graph.get("cora")
    mask = torch.zeros(g.n, g.n, dtype=torch.bool)
    mask[torch.from_numpy(g.row), torch.from_numpy(g.col.astype(np.int64))] = True
    assert int(mask.sum()) == g.nnz                        # (no duplicate entries: the dense mask is the pattern)
    return g.adj, mask, g.n


def test_head_batched_forward_backward_captures_and_replays_bit_for_bit():
    adj, _mask, n = _cora_problem()
    torch.manual_seed(3)
    layer = gcn_amd.GraphAttention(24, 8, heads=4, head_batched=True).to(DEV)
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(n, 24, generator=gen).to(DEV).requires_grad_(True)
    gout = torch.randn(n, 32, generator=gen).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):                                 # the transposed pattern and the workspace now exist
            x.grad = None
            layer.zero_grad(set_to_none=True)
            layer(x, adj).backward(gout)
    torch.cuda.current_stream().wait_stream(side)
    x.grad = None
    layer.zero_grad(set_to_none=True)
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_):
        out = layer(x, adj)
        out.backward(gout)
    for _rep in range(2):
        with torch.no_grad():
            x.copy_(torch.randn(n, 24, generator=gen).to(DEV))
            gout.copy_(torch.randn(n, 32, generator=gen).to(DEV))
        graph_.replay()
        torch.cuda.synchronize()
        got = [out.clone(), x.grad.clone()] + [p.grad.clone() for p in layer.parameters()]
        xe = x.detach().clone().requires_grad_(True)
        saved = [p.grad for p in layer.parameters()]
        for p in layer.parameters():
            p.grad = None
        oe = layer(xe, adj)
        oe.backward(gout)
        torch.cuda.synchronize()
        want = [oe.detach(), xe.grad] + [p.grad for p in layer.parameters()]
        for p, gsaved in zip(layer.parameters(), saved):
            p.grad = gsaved                                # (the graph writes into these tensors)
        for u, v in zip(got, want):
            assert torch.equal(u, v)


# ---- 6. autograd against fp64 dense autograd -------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,F", [(4, 8), (3, 5)])
def test_spmm_heads_and_sddmm_heads_gradients_match_dense_fp64_autograd(H, F):
    g = Graph.get("cora")
    k = H * F
    gen = torch.Generator().manual_seed(H)
    x, a = torch.randn(g.n, k, generator=gen), torch.randn(g.m, k, generator=gen)
    vals, gv = torch.randn(g.nnz, H, generator=gen), torch.randn(g.nnz, H, generator=gen)
    row, col = torch.from_numpy(g.row), torch.from_numpy(g.col.astype(np.int64))
    # the kernels
    xd, vd = x.to(DEV).requires_grad_(True), vals.to(DEV).requires_grad_(True)
    out = gcn_amd.spmm_heads(g.adj, xd, vd)
    out.backward(a.to(DEV))
    ad, bd = a.to(DEV).requires_grad_(True), x.to(DEV).requires_grad_(True)
    sd = gcn_amd.sddmm_heads(g.adj, ad, bd, H)
    sd.backward(gv.to(DEV))
    # fp64 autograd through dense per-head matrices
    x64, v64 = x.double().requires_grad_(True), vals.double().requires_grad_(True)
    outs = []
    for h in range(H):
        D = torch.zeros(g.m, g.n, dtype=torch.float64).index_put((row, col), v64[:, h], accumulate=True)
        outs.append(D @ x64[:, h * F:(h + 1) * F])
    o64 = torch.cat(outs, 1)
    o64.backward(a.double())
    a64, b64 = a.double().requires_grad_(True), x.double().requires_grad_(True)
    s64 = torch.stack([(a64[:, h * F:(h + 1) * F] @ b64[:, h * F:(h + 1) * F].T)[row, col] for h in range(H)], 1)
    s64.backward(gv.double())
    for got, want, what in ((out.detach(), o64.detach(), "spmm_heads"), (xd.grad, x64.grad, "d spmm_heads / dx"),
                            (vd.grad, v64.grad, "d spmm_heads / dvalues"), (sd.detach(), s64.detach(), "sddmm_heads"),
                            (ad.grad, a64.grad, "d sddmm_heads / da"), (bd.grad, b64.grad, "d sddmm_heads / db")):
        err = rel_err(got.cpu().numpy(), want.numpy())
        print(f"[heads] {what} {H}x{F}: rel err {err:.2e}")
        assert err <= 1e-4, (what, err)


# ---- 7. the layer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("concat", [True, False])
def test_head_batched_graph_attention_matches_dense_fp64(concat):
    adj, mask, n = _cora_problem()
    torch.manual_seed(8 + concat)
    layer = gcn_amd.GraphAttention(24, 8, heads=4, concat=concat, head_batched=True).to(DEV)
    with torch.no_grad():
        layer.bias.normal_()
    x = torch.randn(n, 24)
    xd = x.to(DEV).requires_grad_(True)
    out = layer(xd, adj)
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(1))
    out.backward(gout.to(DEV))
    ref_p = {k: v.detach().cpu().double().requires_grad_(True) for k, v in layer.named_parameters()}
    x64 = x.double().requires_grad_(True)
    ref = _dense_gat(x64, mask, ref_p["weight"], ref_p["att_dst"], ref_p["att_src"], ref_p["bias"], 4, 8, concat, 0.2)
    ref.backward(gout.double())
    assert rel_err(out.detach().cpu().numpy(), ref.detach().numpy()) <= 1e-4
    assert rel_err(xd.grad.cpu().numpy(), x64.grad.numpy()) <= 1e-4
    for k, v in layer.named_parameters():
        err = rel_err(v.grad.cpu().numpy(), ref_p[k].grad.numpy())
        print(f"[heads] layer concat={concat}: grad {k} rel err {err:.2e}")
        assert err <= 1e-4, (k, err)


def test_head_batched_two_layer_model_trains_like_the_dense_fp64_model():
    adj, mask, n = _cora_problem()
    torch.manual_seed(0)
    l1 = gcn_amd.GraphAttention(32, 8, heads=4, head_batched=True).to(DEV)
    l2 = gcn_amd.GraphAttention(32, 7, heads=1, head_batched=True).to(DEV)
    x = torch.randn(n, 32)
    y = torch.randint(0, 7, (n,))
    params = list(l1.parameters()) + list(l2.parameters())
    ref = [p.detach().cpu().double().requires_grad_(True) for p in params]
    opt, ropt = torch.optim.Adam(params, lr=0.01), torch.optim.Adam(ref, lr=0.01)
    xd, yd, x64 = x.to(DEV), y.to(DEV), x.double()
    losses, rlosses = [], []
    for _ in range(20):
        opt.zero_grad()
        loss = F_.nll_loss(F_.log_softmax(l2(F_.elu(l1(xd, adj)), adj), dim=1), yd)
        loss.backward()
        opt.step()
        losses.append(loss.item())
        ropt.zero_grad()
        h = F_.elu(_dense_gat(x64, mask, ref[0], ref[1], ref[2], ref[3], 4, 8, True, 0.2))
        rloss = F_.nll_loss(F_.log_softmax(_dense_gat(h, mask, ref[4], ref[5], ref[6], ref[7], 1, 7, True, 0.2), dim=1), y)
        rloss.backward()
        ropt.step()
        rlosses.append(rloss.item())
    rel = max(abs(u - v) / abs(v) for u, v in zip(losses, rlosses))
    print(f"[heads] 20 Adam steps: loss {rlosses[0]:.4f} -> {rlosses[-1]:.4f}, max relative deviation {rel:.2e}")
    assert rlosses[-1] < rlosses[0]
    assert rel <= 1e-4, rel


@pytest.mark.parametrize("concat", [True, False])
def test_head_batched_and_loop_forms_agree(concat):
    g = Graph.get("cora")
    madj = gcn_amd.CsrAdjacency(g.adj.rowptr, g.adj.col, torch.ones(g.nnz, device=DEV), (g.m, g.n), mutable_values=True)
    torch.manual_seed(21)
    loop = gcn_amd.GraphAttention(24, 8, heads=4, concat=concat).to(DEV)
    batched = gcn_amd.GraphAttention(24, 8, heads=4, concat=concat, head_batched=True).to(DEV)
    batched.load_state_dict(loop.state_dict())
    x = torch.randn(g.n, 24).to(DEV)
    err = rel_err(batched(x, g.adj).detach().cpu().numpy(), loop(x, madj).detach().cpu().numpy())
    print(f"[heads] head-batched vs loop, concat={concat}: rel err {err:.2e}")
    assert err <= 1e-5, err


# ---- 8. seeded sweep -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(24))
def test_seeded_sweep_is_exact(seed):
    rng = np.random.default_rng(7000 + seed)
    m, n = int(rng.integers(1, 400)), int(rng.integers(40, 6000))
    deg = float(rng.choice([0.3, 3.0, 20.0, 100.0]))
    long_rows = ((int(rng.integers(0, m)), min(n, int(rng.choice([4096, 4097, 4500, 5999])))),) if seed % 3 == 0 else ()
    H = int(rng.choice([1, 2, 3, 4, 5, 8, 16, 32]))
    F = int(rng.choice([1, 2, 4, 5, 8, 12, 16, 32]))
    by = seed % 2
    what = f"seed {seed}: m={m} n={n} deg={deg} long={long_rows} H={H} F={F} shift={by}"
    try:
        rp, col, _v = random_csr(m, n, int(m * min(deg, n / 2)), seed=seed, empty_rows=float(rng.choice([0.0, 0.3])),
                                 long_rows=long_rows)
        RawProblem(rp, col, n, by).exact(H, F, seed, what)
    except AssertionError:
        print(f"[heads] sweep failed at {what}")
        raise
