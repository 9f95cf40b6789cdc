"""The GATv2 score kernel, its two backward walks and the GraphAttentionV2 layer on the GPU (gcn_amd/csrc/multihead.hip),
against the fp64 twin of tests/gatv2_ref.py.

* bit for bit on an exact grid: h_dst, h_src and att integers in [-2, 2], g eighths in [-7/8, 7/8], slope 0.5.  Every term of
  every sum is then a multiple of 1/16 — a forward term att * leaky_relu(t) of 1/2, a gradient term g * D of 1/16, an act_sums
  term g * t * D (at most 7/8 * 4 = 56 sixteenths) of 1/16 — and with rows of at most 12 289 entries and about 4 * 10^4 entries
  in all every partial sum stays below 2^24 sixteenths, so any correct order gives the same bits and a dropped, doubled or
  misrouted entry shows.  The fp64 reference is asserted to lie on the fp32 grid: the precondition is checked, not assumed.
* the project's standing |err| <= 1e-5 * sum|terms| + 1e-30 on random fp32 inputs, slopes 0.2 and 1.5, with
    forward:        sum|terms| = sum_j |att| max(1, |slope|) (|h_dst| + |h_src|)
    node gradients: sum|terms| = |att| sum_e |g| max(1, |slope|)
    act_sums:       sum|terms| = sum_e |g| max(1, |slope|) (|h_dst| + |h_src|)
  (t has the same sign in fp32 and in fp64 because the inputs are fp32, so D never disagrees with the reference).
* every operand shifted by one element (the element forms on aligned shapes) inside guarded buffers, head isolation under
  NaN and inf, determinism, one tensor on both sides, capture, fp64 autograd of torch formulations, a seeded sweep."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F_

import gatv2_ref
import gcn_amd
import heads_ref
from gcn_amd import graphgen
from util import guards_intact, offset_view, random_csr, rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# fast route, 16-byte form, 16 / 32 / 64 lanes a slot | slow route, element form | k > 256: two column tiles of the backward
SHAPES = [(1, 16), (2, 4), (8, 8), (16, 4), (4, 64), (3, 5), (8, 1), (8, 40)]
GRAPHS = ["cora", "boundary"]
BOUNDARY_LENS = [0, 1, 2, 63, 64, 65, 255, 257, 4095, 4096, 4097, 8193, 12289]


class Graph:
    """a host CSR pattern [m, n], its transposed pattern and (on demand) its device adjacency"""
    _cache = {}

    def __init__(self, rowptr, col, n):
        self.rowptr, self.col, self.n = np.asarray(rowptr, np.int32), np.asarray(col, np.int32), int(n)
        self.m, self.nnz = len(rowptr) - 1, len(col)
        self.row = heads_ref.entry_rows(self.rowptr)
        self.t = heads_ref.transpose_pattern(self.rowptr, self.col, self.n)
        self._adj = None

    @classmethod
    def get(cls, name):
        if name not in cls._cache:
            if name == "cora":
                rp, col, _v, n = graphgen.make_graph("cora", device="cpu", seed=1)
                cls._cache[name] = cls(rp.numpy(), col.numpy(), n)
            elif name == "boundary":
                # rectangular: a row on either side of every threshold of both walks (one batch of a slot, the 64 indices
                # of a fetch, the chunk of 4096 and its multiples), 200 ordinary rows, 3000 trailing empty rows; 3000
                # columns, repeats allowed, and 12 % of the entries name column 3: a long row of the transposed pattern
                rng = np.random.default_rng(11)
                lens = np.concatenate([BOUNDARY_LENS, rng.poisson(30, 200), np.zeros(3000, np.int64)]).astype(np.int64)
                rowptr = np.concatenate([[0], np.cumsum(lens)])
                col = rng.integers(0, 3000, rowptr[-1])
                col[rng.random(len(col)) < 0.12] = 3
                g = cls(rowptr, col, 3000)
                assert int((g.col == 3).sum()) >= 4097 and 35000 <= g.nnz <= 45000
                cls._cache[name] = g
            else:
                raise KeyError(name)
        return cls._cache[name]

    @property
    def adj(self):
        if self._adj is None:
            self._adj = gcn_amd.CsrAdjacency(torch.from_numpy(self.rowptr).to(DEV), torch.from_numpy(self.col).to(DEV),
                                             torch.ones(self.nnz, device=DEV), (self.m, self.n))
        return self._adj


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def on_grid(ref):
    """the fp32 form of an fp64 reference that must lie on the fp32 grid"""
    ref32 = ref.astype(np.float32)
    assert np.array_equal(ref32.astype(np.float64), ref), "the reference is not on the fp32 grid"
    return ref32


class Case:
    """inputs and the twin's results for one (pattern, H, F, slope); computed once and left alone"""

    def __init__(self, g, H, F, slope, seed, grid):
        rng = np.random.default_rng(seed)
        k = H * F
        if grid:
            self.hd, self.hs = (rng.integers(-2, 3, (rows, k)).astype(np.float32) for rows in (g.m, g.n))
            self.att = rng.integers(-2, 3, (H, F)).astype(np.float32)
            self.g = (rng.integers(-7, 8, (g.nnz, H)) / 8.0).astype(np.float32)
        else:
            self.hd, self.hs = (rng.standard_normal((rows, k)).astype(np.float32) for rows in (g.m, g.n))
            self.att = rng.standard_normal((H, F)).astype(np.float32)
            self.g = rng.standard_normal((g.nnz, H)).astype(np.float32)
        self.H, self.F, self.k, self.slope = H, F, k, slope
        args = (self.hd, self.hs, self.att, slope)
        self.s = gatv2_ref.scores(g.rowptr, g.col, *args)
        self.gd, self.gs, self.act, self.ga = gatv2_ref.backward(g.rowptr, g.col, g.n, *args, self.g)
        if not grid:
            self.s_mag = gatv2_ref.scores_magnitude(g.rowptr, g.col, *args)
            self.gd_mag, self.gs_mag, self.act_mag = gatv2_ref.backward_magnitudes(g.rowptr, g.col, g.n, *args, self.g)


@functools.lru_cache(maxsize=None)
def grid_case(name, H, F):
    return Case(Graph.get(name), H, F, 0.5, seed=100 * H + F, grid=True)


# ---- raw calls: operands and outputs `by` elements off a 16-byte boundary, sentinels around them -----------------------------------
def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Raw:
    def __init__(self, g, by):
        self.g, self.by, self.lib = g, by, gcn_amd.load_library()
        trp, trow, tperm = g.t
        self.held = []
        self.rowptr, self.col, self.trp, self.trow, self.tperm = (self.put(a, torch.int32) for a in (g.rowptr, g.col, trp, trow, tperm))

    def put(self, a, dtype=torch.float32):
        view, flat = offset_view(a, self.by, dtype, DEV)
        self.held.append((view, flat))
        return view

    def out(self, *shape):
        return offset_view(shape, self.by, torch.float32, DEV)

    def ws(self, H, k):
        need = ctypes.c_size_t(0)
        assert self.lib.gcn_gatv2_ws_bytes(max(self.g.m, self.g.n), self.g.nnz, H, k, ctypes.byref(need)) == 0
        return torch.empty(need.value, dtype=torch.uint8, device=DEV)

    def run(self, c):
        """(scores, grad_h_dst, act_sums, grad_h_src) of the three calls on the case's inputs; None where nothing is launched"""
        g, H, k = self.g, c.H, c.k
        hd, hs, att, gg = self.put(c.hd), self.put(c.hs), self.put(c.att), self.put(c.g)
        ws = self.ws(H, k)
        outs = [self.out(g.nnz, H), self.out(g.m, k), self.out(g.m, k), self.out(g.n, k)]
        (s, _), (gd, _), (act, _), (gs, _) = outs
        st = [self.lib.gcn_gatv2_scores_csr_f32(vp(self.rowptr), vp(self.col), g.m, g.nnz, H, k, vp(hd), vp(hs), vp(att), c.slope, vp(s),
                                                vp(ws), ws.numel(), stream()),
              self.lib.gcn_gatv2_scores_backward_csr_f32(vp(self.rowptr), vp(self.col), None, g.m, g.nnz, H, k, vp(hd), vp(hs), vp(att),
                                                         c.slope, vp(gg), vp(gd), vp(act), vp(ws), ws.numel(), stream()),
              self.lib.gcn_gatv2_scores_backward_csr_f32(vp(self.trp), vp(self.trow), vp(self.tperm), g.n, g.nnz, H, k, vp(hs), vp(hd),
                                                         vp(att), c.slope, vp(gg), vp(gs), None, vp(ws), ws.numel(), stream())]
        torch.cuda.synchronize()
        assert st == [0, 0, 0], st
        for view, flat in outs + self.held:
            assert guards_intact(flat, view), "a call wrote outside its arrays"
        if g.nnz == 0 or g.m == 0:
            return None                                    # (nothing is launched and nothing written: the caller zeroes)
        return s, gd, act, gs

    def exact(self, c, what):
        got = self.run(c)
        if got is None:
            return
        for t, ref, name in zip(got, (c.s, c.gd, c.act, c.gs), ("scores", "grad_h_dst", "act_sums", "grad_h_src")):
            assert torch.equal(t, dev(on_grid(ref))), f"{what}: {name} H={c.H} F={c.F} shifted by {self.by}"


# ---- 1. exact arithmetic through the public function and its autograd, act_sums through the C ABI --------------------------------
@pytest.mark.parametrize("H,F", SHAPES)
@pytest.mark.parametrize("name", GRAPHS)
def test_scores_and_all_gradients_are_exact_on_the_grid(name, H, F):
    g, c = Graph.get(name), grid_case(name, H, F)
    hd, hs, att = (dev(a).requires_grad_(True) for a in (c.hd, c.hs, c.att))
    s = gcn_amd.gatv2_scores(g.adj, hd, hs, att, c.slope)
    assert s.shape == (g.nnz, H)
    s.backward(dev(c.g))
    what = f"{name} {H}x{F}"
    assert torch.equal(s.detach(), dev(on_grid(c.s))), what + " scores"
    assert torch.equal(hd.grad, dev(on_grid(c.gd))), what + " grad_h_dst"
    assert torch.equal(hs.grad, dev(on_grid(c.gs))), what + " grad_h_src"
    assert torch.equal(att.grad, dev(on_grid(c.ga))), what + " grad_att"
    Raw(g, 0).exact(c, what)                               # the kernel's act_sums, and the same bits with the caller's buffers


# ---- 2. random fp32 inputs ---------------------------------------------------------------------------------------------------------
def ratio(got, ref, mag):
    return float((np.abs(got.cpu().numpy().astype(np.float64) - ref) / (1e-5 * mag + 1e-30)).max()) if ref.size else 0.0


@pytest.mark.parametrize("H,F", SHAPES)
@pytest.mark.parametrize("name", GRAPHS)
def test_random_inputs_keep_the_standing_bound(name, H, F):
    g = Graph.get(name)
    for slope in (0.2, 1.5):
        c = Case(g, H, F, slope, seed=7 * H + F, grid=False)
        hd, hs, att = (dev(a).requires_grad_(True) for a in (c.hd, c.hs, c.att))
        s = gcn_amd.gatv2_scores(g.adj, hd, hs, att, slope)
        s.backward(dev(c.g))
        _s, _gd, act, _gs = Raw(g, 0).run(c)
        for got, ref, mag, what in ((s.detach(), c.s, c.s_mag, "scores"), (hd.grad, c.gd, c.gd_mag, "grad_h_dst"),
                                    (hs.grad, c.gs, c.gs_mag, "grad_h_src"), (act, c.act, c.act_mag, "act_sums")):
            r = ratio(got, ref, mag)
            print(f"[gatv2] {what} {name} {H}x{F} slope={slope}: max error / bound = {r:.4f}")
            assert r <= 1.0, (what, r)
        # grad_att: the column sums of act_sums, a torch reduction over m rows of terms whose magnitudes are act_mag
        r = ratio(att.grad, c.ga, c.act_mag.sum(0).reshape(H, F))
        print(f"[gatv2] grad_att {name} {H}x{F} slope={slope}: max error / bound = {r:.4f}")
        assert r <= 1.0, ("grad_att", r)


# ---- 3. misaligned operands --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,F", SHAPES)
@pytest.mark.parametrize("name", GRAPHS)
def test_every_operand_shifted_by_one_element_is_exact(name, H, F):
    Raw(Graph.get(name), 1).exact(grid_case(name, H, F), name)


# ---- 4. head isolation, determinism, one tensor on both sides ---------------------------------------------------------------------
def _run(g, hd, hs, att, gout, slope=0.2):
    hd, hs, att = (t.clone().requires_grad_(True) for t in (hd, hs, att))
    s = gcn_amd.gatv2_scores(g.adj, hd, hs, att, slope)
    s.backward(gout)
    return [s.detach(), hd.grad, hs.grad, att.grad]


@pytest.mark.parametrize("H,F", [(4, 8), (3, 5), (16, 4)])
def test_nan_or_inf_in_one_head_leaves_the_other_heads_their_bits(H, F):
    g = Graph.get("boundary")
    gen = torch.Generator().manual_seed(H)
    hd, hs = torch.randn(g.m, H * F, generator=gen).to(DEV), torch.randn(g.n, H * F, generator=gen).to(DEV)
    att, gout = torch.randn(H, F, generator=gen).to(DEV), torch.randn(g.nnz, H, generator=gen).to(DEV)
    clean = _run(g, hd, hs, att, gout)
    others = [h for h in range(H) if h != 1]
    cols = torch.tensor([h * F + j for h in others for j in range(F)], device=DEV)
    for bad in (float("nan"), float("inf"), float("-inf")):
        hs2 = hs.clone()
        hs2[:, F:2 * F] = bad                              # head 1 of every source row
        s, gd, gs, ga = _run(g, hd, hs2, att, gout)
        assert torch.equal(s[:, others], clean[0][:, others]), bad
        assert torch.equal(gd[:, cols], clean[1][:, cols]) and torch.equal(gs[:, cols], clean[2][:, cols]), bad
        assert torch.equal(ga[others], clean[3][others]), bad
        assert not bool(torch.isfinite(s[:, 1]).any()), bad
        if bad != bad:
            assert bool(torch.isnan(s[:, 1]).all())
    # one NaN element of h_src poisons the (entry, head)s that gather it and nothing else
    hs3 = hs.clone()
    hs3[3, F + 1] = float("nan")                           # column 3: more than 4096 entries name it
    s3 = _run(g, hd, hs3, att, gout)[0]
    hit = torch.zeros(g.nnz, H, dtype=torch.bool, device=DEV)
    hit[dev(g.col == 3, torch.bool), 1] = True
    assert bool(torch.isnan(s3[hit]).all()) and torch.equal(s3[~hit], clean[0][~hit])


def test_two_calls_are_bit_identical():
    for name, H, F in (("boundary", 8, 8), ("boundary", 3, 5), ("cora", 8, 40)):
        g = Graph.get(name)
        gen = torch.Generator().manual_seed(F)
        hd, hs = torch.randn(g.m, H * F, generator=gen).to(DEV), torch.randn(g.n, H * F, generator=gen).to(DEV)
        att, gout = torch.randn(H, F, generator=gen).to(DEV), torch.randn(g.nnz, H, generator=gen).to(DEV)
        for u, v in zip(_run(g, hd, hs, att, gout), _run(g, hd, hs, att, gout)):
            assert torch.equal(u, v), (name, H, F)


@pytest.mark.parametrize("H,F", [(8, 8), (3, 5)])
def test_one_tensor_on_both_sides_gets_the_sum_of_the_two_gradients(H, F):
    g = Graph.get("cora")
    gen = torch.Generator().manual_seed(2)
    h, att = torch.randn(g.n, H * F, generator=gen).to(DEV), torch.randn(H, F, generator=gen).to(DEV)
    gout = torch.randn(g.nnz, H, generator=gen).to(DEV)
    hh = h.clone().requires_grad_(True)
    s = gcn_amd.gatv2_scores(g.adj, hh, hh, att)
    s.backward(gout)
    s2, gd, gs, _ga = _run(g, h, h, att, gout)
    assert torch.equal(s.detach(), s2) and torch.equal(hh.grad, gd + gs)


# ---- 5. capture --------------------------------------------------------------------------------------------------------------------
def test_layer_forward_backward_captures_and_replays_bit_for_bit():
    g = Graph.get("cora")
    adj, n = g.adj, g.n
    torch.manual_seed(3)
    layer = gcn_amd.GraphAttentionV2(24, 8, heads=4).to(DEV)
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(n, 24, generator=gen).to(DEV).requires_grad_(True)
    gout = torch.randn(n, 32, generator=gen).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):                                 # the transposed pattern and the workspaces now exist
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


# ---- 6. against fp64 autograd of torch formulations ---------------------------------------------------------------------------------
@pytest.mark.parametrize("H,F", [(4, 8), (3, 5)])
def test_gradients_match_fp64_autograd_of_the_torch_formulation(H, F):
    g = Graph.get("cora")
    gen = torch.Generator().manual_seed(H)
    hd, hs = torch.randn(g.m, H * F, generator=gen), torch.randn(g.n, H * F, generator=gen)
    att, gout = torch.randn(H, F, generator=gen), torch.randn(g.nnz, H, generator=gen)
    got = _run(g, hd.to(DEV), hs.to(DEV), att.to(DEV), gout.to(DEV))
    a, b, w = (t.double().requires_grad_(True) for t in (hd, hs, att))
    row, col = torch.from_numpy(g.row), torch.from_numpy(g.col.astype(np.int64))
    s = (F_.leaky_relu(a[row] + b[col], 0.2).view(g.nnz, H, F) * w).sum(-1)
    s.backward(gout.double())
    for u, v, what in zip(got, (s.detach(), a.grad, b.grad, w.grad), ("scores", "d / dh_dst", "d / dh_src", "d / datt")):
        err = rel_err(u.cpu().numpy(), v.numpy())
        print(f"[gatv2] {what} {H}x{F}: rel err {err:.2e}")
        assert err <= 1e-4, (what, err)


def _dense_gatv2(x_src, x_dst, row, col, m, n, w_src, w_dst, att, bias, heads, out_f, concat, slope):
    """fp64 GATv2 layer: the scores per entry by the torch formulation, then a masked softmax over the dense m x n matrix
    (the pattern has no repeated entry) and a dense product per head"""
    h_src, h_dst = x_src @ w_src, x_dst @ w_dst
    s = (F_.leaky_relu(h_dst[row] + h_src[col], slope).view(len(row), heads, out_f) * att).sum(-1)
    has = torch.zeros(m, dtype=torch.bool).index_fill_(0, row, True)[:, None]
    outs = []
    for k in range(heads):
        e = torch.full((m, n), float("-inf"), dtype=torch.float64).index_put((row, col), s[:, k])
        p = torch.softmax(torch.where(has, e, torch.zeros_like(e)), dim=1) * has     # (a row without entries: zeros)
        outs.append(p @ h_src[:, k * out_f:(k + 1) * out_f])
    out = torch.cat(outs, 1) if concat else torch.stack(outs).mean(0)
    return out + bias if bias is not None else out


def _check_layer(layer, adj, row, col, x_src, x_dst, what):
    """forward and every gradient of `layer` against _dense_gatv2 in fp64; x_dst None: one feature matrix for both sides"""
    xs = x_src.to(DEV).requires_grad_(True)
    xd = x_dst.to(DEV).requires_grad_(True) if x_dst is not None else None
    out = layer(xs if xd is None else (xs, xd), adj)
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(1))
    out.backward(gout.to(DEV))
    ref_p = {k: v.detach().cpu().double().requires_grad_(True) for k, v in layer.named_parameters()}
    xs64 = x_src.double().requires_grad_(True)
    xd64 = x_dst.double().requires_grad_(True) if x_dst is not None else xs64
    ref = _dense_gatv2(xs64, xd64, row, col, adj.m, adj.n, ref_p["weight_src"], ref_p.get("weight_dst", ref_p["weight_src"]),
                       ref_p["att"], ref_p.get("bias"), layer.heads, layer.out_features, layer.concat, layer.negative_slope)
    ref.backward(gout.double())
    checks = [("out", out.detach(), ref.detach()), ("grad x_src", xs.grad, xs64.grad)]
    if xd is not None:
        checks.append(("grad x_dst", xd.grad, xd64.grad))
    checks += [("grad " + k, v.grad, ref_p[k].grad) for k, v in layer.named_parameters()]
    for name, got, want in checks:
        err = rel_err(got.cpu().numpy(), want.numpy())
        print(f"[gatv2] layer {what}: {name} rel err {err:.2e}")
        assert err <= 1e-4, (what, name, err)


@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("concat", [True, False])
def test_layer_matches_dense_fp64(concat, share):
    g = Graph.get("cora")
    torch.manual_seed(8 + 2 * concat + share)
    layer = gcn_amd.GraphAttentionV2(24, 8, heads=4, concat=concat, share_weights=share).to(DEV)
    with torch.no_grad():
        layer.bias.normal_()
    row, col = torch.from_numpy(g.row), torch.from_numpy(g.col.astype(np.int64))
    _check_layer(layer, g.adj, row, col, torch.randn(g.n, 24), None, f"concat={concat} share_weights={share}")


def test_layer_on_a_rectangular_block_matches_dense_fp64():
    m, n = 300, 500
    rp, col, _v = random_csr(m, n, 8 * m, seed=5, empty_rows=0.1)          # (no repeated entries; some rows are empty)
    g = Graph(rp, col, n)
    torch.manual_seed(12)
    layer = gcn_amd.GraphAttentionV2(20, 5, heads=3, negative_slope=0.3).to(DEV)
    with torch.no_grad():
        layer.bias.normal_()
    _check_layer(layer, g.adj, torch.from_numpy(g.row), torch.from_numpy(g.col.astype(np.int64)), torch.randn(n, 20),
                 torch.randn(m, 20), "bipartite 300 x 500")


# ---- 7. seeded sweep -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(24))
def test_seeded_sweep_is_exact(seed):
    rng = np.random.default_rng(9000 + seed)
    m, n = int(rng.integers(1, 400)), int(rng.integers(40, 6000))
    deg = float(rng.choice([0.3, 3.0, 20.0, 100.0]))
    long_rows = ((int(rng.integers(0, m)), min(n, int(rng.choice([4096, 4097, 4500])))),) if seed % 3 == 0 else ()
    H = int(rng.choice([1, 2, 3, 4, 5, 8, 16, 32]))
    F = int(rng.choice([1, 2, 4, 5, 8, 12, 16, 32]))
    by = seed % 2
    what = f"seed {seed}: m={m} n={n} deg={deg} long={long_rows} H={H} F={F} shift={by}"
    try:
        rp, col, _v = random_csr(m, n, int(m * min(deg, n / 2)), seed=seed, empty_rows=float(rng.choice([0.0, 0.3])),
                                 long_rows=long_rows)
        g = Graph(rp, col, n)
        Raw(g, by).exact(Case(g, H, F, 0.5, seed, grid=True), what)
    except AssertionError:
        print(f"[gatv2] sweep failed at {what}")
        raise
