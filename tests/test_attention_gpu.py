"""Attention aggregation on the GPU: edge softmax, its fused GAT form, their backwards and the segment sum against fp64
on every entry of graphs that cross every branch of the row-length dispatch; the edge cases of the softmax (shifts, equal
scores, -inf, NaN, aliasing, determinism); GraphAttention against a dense fp64 implementation, forward, gradients and a
20-step training trajectory; and one captured forward + backward replayed bit for bit.

Bounds, with eps = 2^-24, R the row's score range and A(len) the additions on the longest path of a row sum:
forward |p - p*| <= eps (4R + 2A + 8) p* + 1e-38; backward |ds - ds*| <= eps (A + 6) p (|g| + sum_row p|g|) + 1e-38 (times
max(1, slope) fused); per-node gradients and segment sums 1e-5 sum|terms| + 1e-30 (the SDDMM's figure)."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gcn_amd
from gcn_amd import graphgen
from gcn_amd.attention import _workspace
from util import random_csr, rel_err

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
DEV = "cuda:0"
CHUNK = 8192


def A_of(lens):
    """additions on the longest path of the kernel's row sum: one wave per row up to 8192 entries
    (ceil(len/64) per lane + 6 butterfly steps; 8 lanes x <= 4 entries + 3 steps for short rows is below that); longer
    rows: a 256-thread block per 8192-entry chunk (32 per thread + 6 + 3), then the row's chunk partials (ceil(nc/256) per
    thread + 6 + 3), nc <= ceil(len/8192) + 1"""
    lens = np.asarray(lens, np.float64)
    short = np.ceil(lens / 64) + 6
    nc = np.ceil(lens / CHUNK) + 1
    return np.where(lens <= CHUNK, short, 41 + np.ceil(nc / 256) + 9)


def _csr_from_lens(lens, n, seed):
    rng = np.random.default_rng(seed)
    rowptr = np.zeros(len(lens) + 1, np.int64)
    rowptr[1:] = np.cumsum(lens)
    col = rng.integers(0, n, rowptr[-1]).astype(np.int32)      # (duplicates allowed: each stored entry is its own)
    return rowptr.astype(np.int32), col, n


_cache = {}


def graph(name):
    """name -> (rowptr int32 [m+1], col int32 [nnz], n)"""
    if name in _cache:
        return _cache[name]
    if name == "cora":
        rp, col, _v, n = graphgen.make_graph("cora", device="cpu", seed=1)
        g = (rp.numpy(), col.numpy(), n)
    elif name == "hubs":                               # 30 % empty rows, hub rows of 5 000 and 300 000 entries
        rp, col, _v = random_csr(3000, 400000, 30000, seed=5, empty_rows=0.3, long_rows=((7, 5000), (1500, 300000)))
        g = (rp, col, 400000)
    elif name == "one_row":                            # 1 row, 2 M entries
        g = (np.array([0, 2_000_000], np.int32), np.arange(2_000_000, dtype=np.int32), 2_000_000)
    elif name == "empty_tail":                         # the last million rows are empty
        lens = np.concatenate([np.random.default_rng(3).poisson(40, 2000), np.zeros(1_000_000, np.int64)])
        g = _csr_from_lens(lens, 5000, 4)
    elif name == "reddit":
        rp, col, _v, n = graphgen.make_graph("reddit", device="cpu", seed=1, scale=0.02)
        g = (rp.numpy(), col.numpy(), n)
    elif name == "boundaries":                         # every branch of the dispatch, on both sides of each threshold
        lens = [1, 5, 0, 32, 33, 64, 0, 0, 256, 257, 300, 1024, 1025, 5000, 8192, 8193, 20000, 0, 3, 2, 1, 0, 0, 0, 0, 0, 7,
                16385, 31, 32, 1, 1, 1, 4, 0, 16384, 8191, 2]
        g = _csr_from_lens(np.array(lens, np.int64), 50000, 6)
    else:
        raise KeyError(name)
    _cache[name] = g
    return g


GRAPHS = ["cora", "hubs", "one_row", "empty_tail", "reddit", "boundaries"]


def make_adj(name, mutable=False):
    rp, col, n = graph(name)
    m = len(rp) - 1
    return gcn_amd.CsrAdjacency(torch.from_numpy(rp).to(DEV), torch.from_numpy(col).to(DEV),
                                torch.ones(len(col), device=DEV), (m, n), mutable_values=mutable)


class Rows:
    """per-entry row bookkeeping of a CSR on the host (fp64 references)"""

    def __init__(self, rowptr):
        self.rowptr = rowptr.astype(np.int64)
        self.m = len(rowptr) - 1
        self.lens = np.diff(self.rowptr)
        self.ne = self.lens > 0
        self.starts = self.rowptr[:-1][self.ne]
        self.seg = np.repeat(np.arange(int(self.ne.sum())), self.lens[self.ne])     # entry -> index of its non-empty row
        self.row = np.repeat(np.arange(self.m), self.lens)
        self.len_e = self.lens[self.ne][self.seg]
        self.A_e = A_of(self.len_e)

    def rsum(self, x):                                 # per non-empty row
        return np.add.reduceat(x, self.starts) if len(x) else np.zeros(0)

    def full(self, per_ne):                            # per non-empty row -> per row (empty: 0)
        out = np.zeros(self.m)
        out[self.ne] = per_ne
        return out

    def softmax(self, s):
        s = s.astype(np.float64)
        mx, mn = np.maximum.reduceat(s, self.starts), np.minimum.reduceat(s, self.starts)
        e = np.exp(s - mx[self.seg])
        return e / self.rsum(e)[self.seg], (mx - mn)[self.seg]


def check_forward(R, s32, p32, what):
    pref, rng_e = R.softmax(s32)
    assert float(rng_e.max()) <= 16.0 + 1e-3, "the bound is meaningful for R <= 16"
    bound = EPS * (4 * rng_e + 2 * R.A_e + 8) * pref + 1e-38
    ratio = float((np.abs(p32.astype(np.float64) - pref) / bound).max())
    print(f"[attention] forward {what}: max error / bound = {ratio:.4f} over {len(pref)} entries")
    assert ratio <= 1.0, (what, ratio)
    sums = R.rsum(p32.astype(np.float64))
    srat = float((np.abs(sums - 1.0) / (EPS * (A_of(R.lens[R.ne]) + 4))).max())
    print(f"[attention] row sums {what}: max |sum - 1| / bound = {srat:.4f}")
    assert srat <= 1.0, (what, srat)
    return ratio


def scores_for(name, seed=0):
    nnz = len(graph(name)[1])
    return (torch.rand(nnz, generator=torch.Generator().manual_seed(seed)) * 16 - 8).to(DEV)


# ---- 1. forward parity -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GRAPHS)
def test_edge_softmax_forward_matches_fp64(name):
    adj, R = make_adj(name), Rows(graph(name)[0])
    s = scores_for(name)
    p = gcn_amd.edge_softmax(adj, s)
    torch.cuda.synchronize()
    check_forward(R, s.cpu().numpy(), p.cpu().numpy(), name)


def _gat_inputs(name, seed=1):
    rp, col, n = graph(name)
    g = torch.Generator().manual_seed(seed)
    a_dst = (torch.rand(len(rp) - 1, generator=g) * 8 - 4).to(DEV)
    a_src = (torch.rand(n, generator=g) * 8 - 4).to(DEV)
    return a_dst, a_src


def _torch_scores(adj, R, a_dst, a_src, slope):
    row = torch.from_numpy(R.row).to(DEV)
    return F.leaky_relu(a_dst[row] + a_src[adj.col.long()], slope)


@pytest.mark.parametrize("name", GRAPHS)
def test_gat_edge_softmax_forward_matches_fp64_and_the_unfused_form(name):
    adj, R = make_adj(name, mutable=True), Rows(graph(name)[0])
    a_dst, a_src = _gat_inputs(name)
    p = gcn_amd.gat_edge_softmax(adj, a_dst, a_src, 0.2)
    s = _torch_scores(adj, R, a_dst, a_src, 0.2)
    p2 = gcn_amd.edge_softmax(adj, s)
    torch.cuda.synchronize()
    check_forward(R, s.cpu().numpy(), p.cpu().numpy(), name + " (fused)")
    # fused == unfused within the forward bound (both sit within it of the same fp64 softmax, so within twice it of
    # each other; in fact the same arithmetic on the same fp32 scores)
    pref, rng_e = R.softmax(s.cpu().numpy())
    bound = EPS * (4 * rng_e + 2 * R.A_e + 8) * pref + 1e-38
    assert float((np.abs(p.cpu().numpy().astype(np.float64) - p2.cpu().numpy()) / bound).max()) <= 1.0


# ---- 2. edge cases ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [1e4, -1e4])
@pytest.mark.parametrize("name", ["boundaries", "hubs"])
def test_shifted_scores_keep_the_bound(name, shift):
    adj, R = make_adj(name), Rows(graph(name)[0])
    s = scores_for(name, seed=2) + shift               # (rounded to fp32: the reference sees the same inputs)
    p = gcn_amd.edge_softmax(adj, s)
    check_forward(R, s.cpu().numpy(), p.cpu().numpy(), f"{name} shifted by {shift:+.0e}")


def test_equal_scores_give_one_over_len():
    adj, R = make_adj("boundaries"), Rows(graph("boundaries")[0])
    row_val = torch.from_numpy(np.random.default_rng(0).uniform(-50, 50, R.m).astype(np.float32))
    s = row_val[torch.from_numpy(R.row)].to(DEV)
    p = gcn_amd.edge_softmax(adj, s).cpu().numpy().astype(np.float64)
    want = 1.0 / R.len_e
    assert float((np.abs(p - want) / want).max()) <= 2 * EPS


def _masked_case():
    rp, _col, _n = graph("boundaries")
    R = Rows(rp)
    s = scores_for("boundaries", seed=3).cpu().numpy()
    rng = np.random.default_rng(1)
    mask = rng.random(len(s)) < 0.3                    # -inf entries beside finite ones
    dead_rows = [1, 8, 12, 15, 16]                     # whole rows of -inf: 5, 256, 1025, 8193 and 20000 entries
    for r in dead_rows:
        mask[R.rowptr[r]:R.rowptr[r + 1]] = True
    s[mask] = -np.inf
    return R, s, mask, dead_rows


def test_minus_inf_entries_give_exact_zeros_and_dead_rows_give_zeros():
    adj = make_adj("boundaries")
    R, s, mask, dead_rows = _masked_case()
    p = gcn_amd.edge_softmax(adj, torch.from_numpy(s).to(DEV)).cpu().numpy()
    assert not np.isnan(p).any()
    assert (p[mask] == 0.0).all()
    dead = np.isin(R.row, dead_rows)
    assert (p[dead] == 0.0).all()
    # the live entries are the softmax of the live entries of their row
    live = ~mask
    mx = np.maximum.reduceat(np.where(live, s, -1e30).astype(np.float64), R.starts)[R.seg]
    e = np.where(live, np.exp(np.where(live, s.astype(np.float64) - mx, 0.0)), 0.0)
    den = R.rsum(e)[R.seg]
    ok = live & ~dead
    pref = e[ok] / den[ok]
    bound = EPS * (4 * 16 + 2 * R.A_e[ok] + 8) * pref + 1e-38
    assert float((np.abs(p[ok] - pref) / bound).max()) <= 1.0


def test_a_nan_stays_in_its_row():
    adj, R = make_adj("boundaries"), Rows(graph("boundaries")[0])
    s = scores_for("boundaries", seed=4)
    clean = gcn_amd.edge_softmax(adj, s).cpu().numpy()
    bad_rows = [0, 3, 10, 13, 16, 27]                  # 1, 32, 300, 5000, 20000 and 16385 entries
    s2 = s.clone()
    for r in bad_rows:
        s2[int(R.rowptr[r]) + (int(R.lens[r]) * 2) // 3] = float("nan")
    p = gcn_amd.edge_softmax(adj, s2).cpu().numpy()
    bad = np.isin(R.row, bad_rows)
    assert np.isnan(p[bad]).all()
    assert np.array_equal(p[~bad], clean[~bad])


def test_p_may_alias_s_and_two_calls_are_bit_identical():
    for name in ("boundaries", "reddit"):
        adj = make_adj(name)
        s = scores_for(name, seed=5)
        p1 = gcn_amd.edge_softmax(adj, s)
        p2 = gcn_amd.edge_softmax(adj, s)
        assert torch.equal(p1, p2)
        buf = s.clone()
        ws = _workspace(adj, adj.nnz, buf.device)
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        st = gcn_amd.load_library().gcn_edge_softmax_csr_f32(vp(adj.rowptr), adj.m, adj.nnz, vp(buf), vp(buf), vp(ws), ws.numel(),
                                                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert st == 0
        torch.cuda.synchronize()
        assert torch.equal(buf, p1)


def test_non_fp32_scores_raise():
    adj = make_adj("cora")
    with pytest.raises(gcn_amd.GcnAmdError):
        gcn_amd.edge_softmax(adj, torch.ones(adj.nnz, dtype=torch.float64, device=DEV))


# ---- 3. backward parity ----------------------------------------------------------------------------------------------
def _ds_ref(R, p32, g32, d=None):
    p, g = p32.astype(np.float64), g32.astype(np.float64)
    t = R.rsum(p * g)[R.seg]
    ds = p * (g - t)
    bound = EPS * (R.A_e + 6) * p * (np.abs(g) + R.rsum(p * np.abs(g))[R.seg]) + 1e-38
    if d is not None:
        ds = ds * d
    return ds, bound


@pytest.mark.parametrize("name", GRAPHS)
def test_edge_softmax_backward_matches_fp64(name):
    adj, R = make_adj(name), Rows(graph(name)[0])
    s = scores_for(name, seed=6).requires_grad_(True)
    p = gcn_amd.edge_softmax(adj, s)
    g = torch.randn(adj.nnz, generator=torch.Generator().manual_seed(7)).to(DEV)
    p.backward(g)
    torch.cuda.synchronize()
    ds_ref, bound = _ds_ref(R, p.detach().cpu().numpy(), g.cpu().numpy())
    ratio = float((np.abs(s.grad.cpu().numpy() - ds_ref) / bound).max())
    print(f"[attention] backward {name}: max error / bound = {ratio:.4f}")
    assert ratio <= 1.0, (name, ratio)


def _gat_backward_raw(adj, a_dst, a_src, slope, p, g):
    ds, gd = torch.empty_like(p), torch.empty(adj.m, device=p.device)
    ws = _workspace(adj, adj.nnz, p.device)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    st = gcn_amd.load_library().gcn_gat_edge_softmax_backward_csr_f32(
        vp(adj.rowptr), vp(adj.col), adj.m, adj.nnz, vp(a_dst), vp(a_src), slope, vp(p), vp(g), vp(ds), vp(gd), vp(ws),
        ws.numel(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0
    return ds, gd


@pytest.mark.parametrize("slope", [0.2, 1.5])
@pytest.mark.parametrize("name", GRAPHS)
def test_gat_edge_softmax_backward_matches_fp64(name, slope):
    rp, col, n = graph(name)
    adj, R = make_adj(name, mutable=True), Rows(rp)
    a_dst, a_src = _gat_inputs(name, seed=8)
    if name == "boundaries":                           # pre-activations of exactly 0: the derivative there is the slope
        a_dst[4] = 0.0
        a_src[torch.from_numpy(col[R.rowptr[4]:R.rowptr[4] + 10].astype(np.int64)).to(DEV)] = 0.0
    a_dst.requires_grad_(True)
    a_src.requires_grad_(True)
    p = gcn_amd.gat_edge_softmax(adj, a_dst, a_src, slope)
    g = torch.randn(adj.nnz, generator=torch.Generator().manual_seed(9)).to(DEV)
    p.backward(g)
    gd1, gs1 = a_dst.grad.clone(), a_src.grad.clone()
    a_dst.grad = a_src.grad = None
    gcn_amd.gat_edge_softmax(adj, a_dst, a_src, slope).backward(g)
    assert torch.equal(a_src.grad, gs1) and torch.equal(a_dst.grad, gd1)          # bit-identical over two runs
    ds, gd_raw = _gat_backward_raw(adj, a_dst.detach(), a_src.detach(), slope, p.detach(), g)
    torch.cuda.synchronize()
    assert torch.equal(gd_raw, gd1)
    pre = a_dst.detach().cpu().numpy().astype(np.float64)[R.row] + a_src.detach().cpu().numpy().astype(np.float64)[col]
    d = np.where(pre > 0, 1.0, slope)
    ds_ref, bound = _ds_ref(R, p.detach().cpu().numpy(), g.cpu().numpy(), d)
    ratio = float((np.abs(ds.cpu().numpy() - ds_ref) / (bound * max(1.0, slope))).max())
    print(f"[attention] fused backward {name} slope {slope}: max error / bound = {ratio:.4f}")
    assert ratio <= 1.0, (name, ratio)
    gd_ref, gd_mag = R.full(R.rsum(ds_ref)), R.full(R.rsum(np.abs(ds_ref)))
    r_dst = float((np.abs(gd1.cpu().numpy() - gd_ref) / (1e-5 * gd_mag + 1e-30)).max())
    gs_ref = np.bincount(col, weights=ds_ref, minlength=n)
    gs_mag = np.bincount(col, weights=np.abs(ds_ref), minlength=n)
    r_src = float((np.abs(gs1.cpu().numpy() - gs_ref) / (1e-5 * gs_mag + 1e-30)).max())
    print(f"[attention] fused backward {name} slope {slope}: grad_a_dst {r_dst:.4f}, grad_a_src {r_src:.4f} of their bounds")
    assert r_dst <= 1.0 and r_src <= 1.0, (name, r_dst, r_src)


def _fwd_bound(R, s32):
    pref, rng_e = R.softmax(s32)
    return pref, EPS * (4 * rng_e + 2 * R.A_e + 8) * pref + 1e-38


@pytest.mark.parametrize("name", ["cora", "boundaries"])
def test_backwards_match_fp64_autograd(name):
    """An independent reference: torch autograd in fp64 on the CPU through softmax(leaky_relu(a_dst[row] + a_src[col]))
    built from index_add_ (no closed-form backward written here).  Autograd differentiates at the fp64 p*, the kernel at its
    own fp32 p, so the tolerance is the backward bound plus what the forward bound fb = |p - p*| allows:
    |ds(p) - ds(p*)| <= fb_e (|g_e| + sum_row p|g|) + p_e sum_row fb|g|   (first order in fb; d = 1 or slope multiplies all)."""
    rp, col, n = graph(name)
    adj, R = make_adj(name, mutable=True), Rows(rp)
    slope = 0.2
    a_dst, a_src = _gat_inputs(name, seed=12)
    g = torch.randn(adj.nnz, generator=torch.Generator().manual_seed(13))
    # fp64 autograd on the host
    seg = torch.from_numpy(R.row)
    ad64 = a_dst.cpu().double().requires_grad_(True)
    as64 = a_src.cpu().double().requires_grad_(True)
    s64 = F.leaky_relu(ad64[seg] + as64[torch.from_numpy(col.astype(np.int64))], slope)
    s64.retain_grad()
    mx = torch.full((R.m,), float("-inf"), dtype=torch.float64).scatter_reduce(0, seg, s64.detach(), "amax")
    e64 = torch.exp(s64 - mx[seg])
    p64 = e64 / torch.zeros(R.m, dtype=torch.float64).index_add_(0, seg, e64)[seg]
    p64.backward(g.double())
    # the kernels
    ad, asr = a_dst.clone().requires_grad_(True), a_src.clone().requires_grad_(True)
    gcn_amd.gat_edge_softmax(adj, ad, asr, slope).backward(g.to(DEV))
    s32 = F.leaky_relu(a_dst[seg.to(DEV)] + a_src[adj.col.long()], slope).requires_grad_(True)
    p32 = gcn_amd.edge_softmax(adj, s32)
    p32.backward(g.to(DEV))
    torch.cuda.synchronize()
    pn, gn = p32.detach().cpu().numpy().astype(np.float64), g.numpy().astype(np.float64)
    _pref, fb = _fwd_bound(R, s32.detach().cpu().numpy())
    T = R.rsum(pn * np.abs(gn))[R.seg]
    tol = EPS * (R.A_e + 6) * pn * (np.abs(gn) + T) + fb * (np.abs(gn) + T) + pn * R.rsum(fb * np.abs(gn))[R.seg] + 1e-38
    ratio = float((np.abs(s32.grad.cpu().numpy() - s64.grad.numpy()) / tol).max())
    print(f"[attention] backward vs fp64 autograd {name}: max error / tolerance = {ratio:.4f}")
    assert ratio <= 1.0, (name, ratio)
    # per-node gradients: sums of those ds, each within tol of autograd's -> 1e-5 sum|terms| plus the summed tolerances
    ds64 = s64.grad.numpy()
    pre = a_dst.cpu().numpy().astype(np.float64)[R.row] + a_src.cpu().numpy().astype(np.float64)[col]
    d = np.where(pre > 0, 1.0, slope)
    gd_tol = 1e-5 * R.full(R.rsum(np.abs(ds64) * d)) + R.full(R.rsum(tol * d)) + 1e-30
    gs_tol = 1e-5 * np.bincount(col, weights=np.abs(ds64) * d, minlength=n) + np.bincount(col, weights=tol * d, minlength=n) + 1e-30
    r_dst = float((np.abs(ad.grad.cpu().numpy() - ad64.grad.numpy()) / gd_tol).max())
    r_src = float((np.abs(asr.grad.cpu().numpy() - as64.grad.numpy()) / gs_tol).max())
    print(f"[attention] fused gradients vs fp64 autograd {name}: grad_a_dst {r_dst:.4f}, grad_a_src {r_src:.4f} of their tolerances")
    assert r_dst <= 1.0 and r_src <= 1.0, (name, r_dst, r_src)


# ---- 4. segment sum --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hubs", "empty_tail", "boundaries", "one_row"])
def test_segment_sum_matches_fp64(name):
    rp, col, _n = graph(name)
    R = Rows(rp)
    x = torch.randn(len(col), generator=torch.Generator().manual_seed(10))
    perm = torch.randperm(len(col), generator=torch.Generator().manual_seed(11))
    rpd = torch.from_numpy(rp).to(DEV)
    out = gcn_amd.segment_sum(rpd, x.to(DEV))
    outp = gcn_amd.segment_sum(rpd, x.to(DEV), perm=perm.to(DEV, torch.int32))
    assert torch.equal(out, gcn_amd.segment_sum(rpd, x.to(DEV)))
    x64 = x.numpy().astype(np.float64)
    for got, xs in ((out, x64), (outp, x64[perm.numpy()])):
        ref, mag = R.full(R.rsum(xs)), R.full(R.rsum(np.abs(xs)))
        ratio = float((np.abs(got.cpu().numpy() - ref) / (1e-5 * mag + 1e-30)).max())
        print(f"[attention] segment sum {name}: max error / bound = {ratio:.4f}")
        assert ratio <= 1.0, (name, ratio)


# ---- 5. the layer ----------------------------------------------------------------------------------------------------
def _dense_gat(x, mask, weight, att_dst, att_src, bias, heads, out_f, concat, slope):
    """dense fp64 GAT layer: masked softmax over the n x n score matrix"""
    h = x @ weight
    outs = []
    for k in range(heads):
        hk = h[:, k * out_f:(k + 1) * out_f]
        e = F.leaky_relu((hk @ att_dst[k])[:, None] + (hk @ att_src[k])[None, :], slope)
        e = e.masked_fill(~mask, float("-inf"))
        outs.append(torch.softmax(e, dim=1) @ hk)
    out = torch.cat(outs, 1) if concat else torch.stack(outs).mean(0)
    return out + bias if bias is not None else out


def _cora_problem():
    rp, col, n = graph("cora")
    R = Rows(rp)
    mask = torch.zeros(n, n, dtype=torch.bool)
    mask[torch.from_numpy(R.row), torch.from_numpy(col.astype(np.int64))] = True
    assert int(mask.sum()) == len(col)                 # (no duplicate entries: the dense mask is the pattern)
    return make_adj("cora", mutable=True), mask, n


@pytest.mark.parametrize("heads,concat", [(1, True), (4, True), (4, False)])
def test_graph_attention_matches_dense_fp64(heads, concat):
    adj, mask, n = _cora_problem()
    torch.manual_seed(heads * 2 + concat)
    layer = gcn_amd.GraphAttention(24, 8, heads=heads, concat=concat).to(DEV)
    with torch.no_grad():
        layer.bias.normal_()
    x = torch.randn(n, 24)
    xd = x.to(DEV).requires_grad_(True)
    out = layer(xd, adj)
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(1))
    out.backward(gout.to(DEV))
    ref_p = {k: v.detach().cpu().double().requires_grad_(True) for k, v in layer.named_parameters()}
    x64 = x.double().requires_grad_(True)
    ref = _dense_gat(x64, mask, ref_p["weight"], ref_p["att_dst"], ref_p["att_src"], ref_p["bias"], heads, 8, concat, 0.2)
    ref.backward(gout.double())
    assert rel_err(out.detach().cpu().numpy(), ref.detach().numpy()) <= 1e-4
    assert rel_err(xd.grad.cpu().numpy(), x64.grad.numpy()) <= 1e-4
    for k, v in layer.named_parameters():
        err = rel_err(v.grad.cpu().numpy(), ref_p[k].grad.numpy())
        print(f"[attention] layer heads={heads} concat={concat}: grad {k} rel err {err:.2e}")
        assert err <= 1e-4, (k, err)


def test_two_layer_model_trains_like_the_dense_fp64_model():
    adj, mask, n = _cora_problem()
    torch.manual_seed(0)
    l1 = gcn_amd.GraphAttention(32, 8, heads=4).to(DEV)
    l2 = gcn_amd.GraphAttention(32, 7, heads=1).to(DEV)
    x = torch.randn(n, 32)
    y = torch.randint(0, 7, (n,))
    params = list(l1.parameters()) + list(l2.parameters())
    ref = [p.detach().cpu().double().requires_grad_(True) for p in params]
    opt, ropt = torch.optim.Adam(params, lr=0.01), torch.optim.Adam(ref, lr=0.01)
    xd, yd, x64 = x.to(DEV), y.to(DEV), x.double()
    losses, rlosses = [], []
    for _ in range(20):
        opt.zero_grad()
        loss = F.nll_loss(F.log_softmax(l2(F.elu(l1(xd, adj)), adj), dim=1), yd)
        loss.backward()
        opt.step()
        losses.append(loss.item())
        ropt.zero_grad()
        h = F.elu(_dense_gat(x64, mask, ref[0], ref[1], ref[2], ref[3], 4, 8, True, 0.2))
        rloss = F.nll_loss(F.log_softmax(_dense_gat(h, mask, ref[4], ref[5], ref[6], ref[7], 1, 7, True, 0.2), dim=1), y)
        rloss.backward()
        ropt.step()
        rlosses.append(rloss.item())
    rel = max(abs(a - b) / abs(b) for a, b in zip(losses, rlosses))
    print(f"[attention] 20 Adam steps: loss {rlosses[0]:.4f} -> {rlosses[-1]:.4f}, max relative deviation {rel:.2e}")
    assert rlosses[-1] < rlosses[0]
    assert rel <= 1e-4, rel


def test_graph_attention_under_bf16_autocast_keeps_scores_and_softmax_fp32(monkeypatch):
    """Inside torch.autocast(bf16) only x·W runs in bf16: a_dst, a_src, p and the weighted SpMM's operand are fp32.  Against
    the fp32 run the difference is that of a bf16 matmul: x, W and h each rounded to 8 bits (3 * 2^-8 on h, relative to its
    largest entry), which moves a score by at most that times |a| and so p by about 2 * that * max|a| (both exponents);
    gradients pass one more bf16 matmul on the way back: twice the tolerance."""
    import gcn_amd.layers as layers_mod
    adj, _mask, n = _cora_problem()
    torch.manual_seed(11)
    layer = gcn_amd.GraphAttention(24, 8, heads=2).to(DEV)
    x = torch.randn(n, 24)
    gout = torch.randn(n, 16, generator=torch.Generator().manual_seed(2)).to(DEV)
    seen = []
    real_gat, real_spmm = layers_mod.gat_edge_softmax, layers_mod.spmm

    def spy_gat(adj_, a_dst, a_src, slope):
        p = real_gat(adj_, a_dst, a_src, slope)
        seen.append(("scores", a_dst.dtype, a_src.dtype, p.dtype, float(a_dst.abs().max() + a_src.abs().max())))
        return p

    def spy_spmm(adj_, dense, values=None):
        seen.append(("spmm", dense.dtype, values.dtype))
        return real_spmm(adj_, dense, values=values)

    monkeypatch.setattr(layers_mod, "gat_edge_softmax", spy_gat)
    monkeypatch.setattr(layers_mod, "spmm", spy_spmm)

    def run(autocast):
        xd = x.to(DEV).requires_grad_(True)
        layer.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            out = layer(xd, adj)
        out.backward(gout)
        return [out.detach().float(), xd.grad] + [p.grad.clone() for p in layer.parameters()], out.dtype

    ref, _ = run(False)
    amax = max(r[4] for r in seen if r[0] == "scores")
    seen.clear()
    got, out_dtype = run(True)
    assert out_dtype == torch.float32
    assert len(seen) == 4
    for r in seen:
        assert all(dt == torch.float32 for dt in r[1:] if isinstance(dt, torch.dtype)), r
    tol = 3 * 2.0 ** -8 * (1 + 2 * amax)
    names = ["out", "x.grad"] + [k for k, _ in layer.named_parameters()]
    for k, (a, b) in zip(names, zip(got, ref)):
        err = rel_err(a.cpu().numpy(), b.cpu().numpy())
        print(f"[attention] bf16 autocast vs fp32, {k}: rel err {err:.2e} (tolerance {tol if k == 'out' else 2 * tol:.2e})")
        assert err <= (tol if k == "out" else 2 * tol), (k, err)
        if k in ("out", "weight"):                     # (the bias gradient is a column sum of gout either way)
            assert err > 0, "x·W did not run in bf16 at all"


# ---- 6. capture ------------------------------------------------------------------------------------------------------
def test_forward_backward_captures_and_replays_bit_for_bit():
    adj, _mask, n = _cora_problem()
    torch.manual_seed(3)
    layer = gcn_amd.GraphAttention(24, 16, heads=1).to(DEV)
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(n, 24, generator=gen).to(DEV).requires_grad_(True)
    gout = torch.randn(n, 16, generator=gen).to(DEV)

    def step():
        layer(x, adj).backward(gout)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):                             # plans, the transpose, its permutation and the workspace now exist
            x.grad = None
            layer.zero_grad(set_to_none=True)
            step()
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
            gout.copy_(torch.randn(n, 16, generator=gen).to(DEV))
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
            p.grad = gsaved                            # (the graph writes into these tensors)
        for a, b in zip(got, want):
            assert torch.equal(a, b)


# ---- 9. the adjacency's scratch keeper and its one transposed pattern -----------------------------------------------------------
def _retire_rule(adj, kind, narrow, wide):
    """the rule of spmm.Scratch for one kind: a wider call replaces the buffer and keeps the one it replaces (a captured step
    recorded its address and goes on writing there), a narrow call after it neither shrinks nor retires.  Identity and sizes
    only: nothing is captured"""
    keeper = adj._scratch
    narrow()
    small = keeper.buffers[kind]
    wide()
    big = keeper.buffers[kind]
    assert big is not small and big.numel() > small.numel()
    assert any(w is small for w in keeper.retired)
    retired = len(keeper.retired)
    narrow()
    assert keeper.buffers[kind] is big and len(keeper.retired) == retired


def test_a_wider_heads_call_keeps_the_edge_scratch_a_capture_may_hold():
    adj = make_adj("boundaries")
    vals = torch.ones(adj.nnz, 2, device=DEV)
    x = torch.ones(adj.n, 64, device=DEV)
    _retire_rule(adj, "edge", lambda: gcn_amd.spmm_heads(adj, x[:, :4].contiguous(), vals), lambda: gcn_amd.spmm_heads(adj, x, vals))
    assert len(adj._scratch.retired) == 1 and set(adj._scratch.buffers) == {"edge"}


def test_a_wider_gatv2_call_keeps_the_gatv2_scratch_a_capture_may_hold():
    adj = make_adj("boundaries")
    hd, hs = torch.ones(adj.m, 64, device=DEV), torch.ones(adj.n, 64, device=DEV)
    call = lambda f: gcn_amd.gatv2_scores(adj, hd[:, :2 * f].contiguous(), hs[:, :2 * f].contiguous(), torch.ones(2, f, device=DEV))
    _retire_rule(adj, "gatv2", lambda: call(2), lambda: call(32))
    assert len(adj._scratch.retired) == 1 and set(adj._scratch.buffers) == {"gatv2"}


@pytest.mark.parametrize("mutable", [False, True])
def test_every_backward_walk_reads_the_adjacencys_one_transposed_pattern(mutable, monkeypatch):
    import sys
    agg_mod, att_mod = sys.modules["gcn_amd.aggregate"], sys.modules["gcn_amd.attention"]   # (the package's names are functions)
    adj = make_adj("boundaries", mutable=mutable)
    passed = {}                                        # entry point -> the (trowptr, trow, tperm) it was handed (None: not passed)
    where = {"gcn_aggregate_backward_csr": (0, 1, 2), "gcn_spmm_heads_csr_f32": (0, 1, 2), "gcn_segment_sum_heads_csr_f32": (0, None, 5)}

    def recording(real):
        def call(name, *args, **kw):
            if name in where and args[where[name][2]] is not None:             # (perm None: a walk of the pattern itself)
                passed[name] = tuple(args[i] if i is not None else None for i in where[name])
            return real(name, *args, **kw)
        return call

    monkeypatch.setattr(agg_mod, "call", recording(agg_mod.call))
    monkeypatch.setattr(att_mod, "call", recording(att_mod.call))
    gen = torch.Generator().manual_seed(21)
    x = torch.randn(adj.n, 4, generator=gen).to(DEV).requires_grad_(True)
    gcn_amd.aggregate(adj, x, "max").sum().backward()
    vals = torch.rand(adj.nnz, 2, generator=gen).to(DEV)
    gcn_amd.spmm_heads(adj, x, vals).sum().backward()
    a_dst = torch.randn(adj.m, 2, generator=gen).to(DEV).requires_grad_(True)
    a_src = torch.randn(adj.n, 2, generator=gen).to(DEV).requires_grad_(True)
    (gcn_amd.gat_edge_softmax(adj, a_dst, a_src) * vals).sum().backward()
    torch.cuda.synchronize()
    # exactly one pattern cache on the adjacency, and every unit was handed its arrays themselves
    caches = [k for k, v in vars(adj).items() if isinstance(v, (tuple, list)) and any(isinstance(t, torch.Tensor) for t in v)]
    assert caches == ["_tpattern"]
    tp = adj.tpattern()
    assert tp is adj._tpattern and len(tp) == 3
    assert set(passed) == set(where)
    for name, arrays in passed.items():
        for got, cached in zip(arrays, tp):
            assert got is None or got is cached, name
    for t, count in zip(tp, (adj.n + 1, adj.nnz, adj.nnz)):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == count
    assert torch.equal(tp[2].long(), adj._transposed_pattern()[2])
    if mutable:
        t = adj._mutable_transpose()
        assert torch.equal(t.rowptr, tp[0]) and torch.equal(t.col, tp[1])
        assert [k for k, v in vars(adj).items() if isinstance(v, (tuple, list))] == ["_tpattern"]
