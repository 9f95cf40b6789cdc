"""gcn_amd.edge_aggregate, its gradients and the GIN layers on the GPU, against the numpy twins of tests/edge_aggregate_ref.py.

Graphs (the four kinds of tests/test_heads_gpu.py, rebuilt here): Cora-shaped; "boundaries" (a row on either side of every
length at which the kernels take another path: the 64-entry batch, the 4096-entry chunk and its multiples); "hubs" (30 %
empty rows, rows of 5 000 and 300 000 entries, 5 % of the entries in one column: a long row of the transposed pattern);
"empty_tail" (a million empty rows behind 2 000 live ones).  "boundaries" and "hubs" repeat (row, column) pairs a thousand
times and more (5 % of every row names one column): under op = add the terms of the gradient in x are then copies of one
g[r, j], the input on which an uncompensated chain of additions drifts past the standing bound.  Widths: both sides of 16 / 32 / 64 lanes a slot and of the
column tile on the 16-byte route (4, 64, 68, 128, 132, 256, 260) and on the element route (1, 3, 5, 17, 33, 65, and 64 with
one operand off its 16-byte boundary).

1. Exact grid: x and g integers in [-3, 3], edge_feat eighths in [-1, 1].  Every message and gradient term is a multiple of
   1/8 of magnitude at most 4, and the longest sum (300 000 terms) stays below 2^24 eighths, so every order of every sum
   gives the twin's bits and any dropped, doubled or misrouted entry shows.  The grid is full of ties: arg is compared
   exactly.
2. Random fp32 inputs: max / min and arg stay bit-identical (a selection of identically rounded messages); sums and both
   gradients keep the standing bound 1e-5 * sum |terms| + 1e-30 per element.
3. Non-finite inputs, 4. the call contract (same bits twice, frozen operands, views, repeated backward, capture),
5. autograd against the fp64 torch formulation, 6. the layers against a dense fp64 restatement."""
import numpy as np
import pytest
import torch

import edge_aggregate_ref as ref
import gcn_amd
from gcn_amd import _lib, edgefeat, graphgen
from gcn_amd._lib import call
from util import guards_intact, offset_view

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OPS = [("add", None), ("add", "relu"), ("mul", None), ("mul", "relu")]
TWO = [("add", "relu"), ("mul", None)]                     # GINE's message, and the one whose gradients read both operands
VEC4 = [4, 64, 68, 128, 132, 256, 260]
VEC1 = [1, 3, 5, 17, 33, 65]
BOUNDARY_LENS = [0, 1, 2, 63, 64, 65, 0, 0, 3, 4095, 4096, 4097, 8192, 8193, 0, 12289, 16385, 20000, 5, 31, 32, 33, 0, 127, 128, 129,
                 7, 0, 0, 0, 0, 0, 0, 0, 0, 1, 255, 256, 257, 0]


# ---- graphs ----------------------------------------------------------------------------------------------------------------
def _csr_from_lens(lens, n, seed, popular=None):
    rng = np.random.default_rng(seed)
    rowptr = np.zeros(len(lens) + 1, np.int64)
    rowptr[1:] = np.cumsum(lens)
    col = rng.integers(0, n, rowptr[-1]).astype(np.int32)      # (duplicates allowed: each stored entry is its own)
    if popular is not None:                                     # a long row of the transposed pattern too
        col[rng.random(len(col)) < 0.05] = popular
    return rowptr, col, n


class Graph:
    _cache = {}

    def __init__(self, rowptr, col, n, live=None):
        self.rowptr, self.col, self.n = np.asarray(rowptr, np.int64), np.asarray(col, np.int64), int(n)
        self.m, self.nnz = len(rowptr) - 1, len(col)
        self.live = self.m if live is None else live           # rows from `live` on are empty
        self.rp = self.rowptr[:self.live + 1]                  # the twin's CSR: the live rows
        self._adj = None

    @classmethod
    def get(cls, name):
        if name in cls._cache:
            return cls._cache[name]
        if name == "cora":
            rp, col, _v, n = graphgen.make_graph("cora", device="cpu", seed=1)
            g = cls(rp.numpy(), col.numpy(), n)
        elif name == "boundaries":
            g = cls(*_csr_from_lens(np.array(BOUNDARY_LENS, np.int64), 3000, 6, popular=11))
        elif name == "hubs":
            rng = np.random.default_rng(5)
            lens = rng.poisson(10, 3000)
            lens[rng.random(3000) < 0.3] = 0
            lens[7], lens[1500] = 5000, 300000
            g = cls(*_csr_from_lens(lens, 20000, 6, popular=3))
        elif name == "empty_tail":
            lens = np.concatenate([np.random.default_rng(3).poisson(40, 2000), np.zeros(1_000_000, np.int64)])
            g = cls(*_csr_from_lens(lens, 5000, 4), live=2000)
        elif name == "small":                                  # the non-finite and contract cases: two long rows, empty rows
            rng = np.random.default_rng(8)
            lens = rng.poisson(5, 300)
            lens[rng.random(300) < 0.2] = 0
            lens[4], lens[250] = 4100, 70
            g = cls(*_csr_from_lens(lens, 200, 9, popular=2))
        else:
            raise KeyError(name)
        cls._cache[name] = g
        return g

    @property
    def adj(self):
        if self._adj is None:
            self._adj = gcn_amd.CsrAdjacency(dev(self.rowptr, torch.int32), dev(self.col, torch.int32),
                                             torch.ones(self.nnz, device=DEV), (self.m, self.n))
        return self._adj


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def g_rows(g, live_rows):
    """a [g.m, k] device tensor whose first g.live rows are `live_rows` (rows past that have no entry)"""
    if g.live == g.m:
        return dev(live_rows)
    out = torch.zeros(g.m, live_rows.shape[1], device=DEV)
    out[:g.live] = dev(live_rows)
    return out


def grid_inputs(g, k, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, (g.n, k)).astype(np.float32)
    w = (rng.integers(-8, 9, (g.nnz, k)) / 8.0).astype(np.float32)
    gout = rng.integers(-3, 4, (g.live, k)).astype(np.float32)
    # the bound that makes every sum exact in fp32 in any order: terms are multiples of 1/8, |t| <= 4, and the longest
    # row (of the pattern or of its transpose) has fewer than 2^24 / 32 of them
    assert np.abs(x).max() <= 3 and np.abs(w).max() <= 1 and np.array_equal(w * 8, np.round(w * 8)) and np.abs(gout).max() <= 3
    longest = max(int(np.diff(g.rp).max()), int(np.bincount(g.col, minlength=g.n).max()))
    assert longest * 4 * 8 < 2 ** 24
    return x, w, gout


def random_inputs(g, k, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((g.n, k)).astype(np.float32), rng.standard_normal((g.nnz, k)).astype(np.float32),
            rng.standard_normal((g.live, k)).astype(np.float32))


def run(g, x, w, gout, op, act, reduce, x_grad=True, w_grad=True):
    """(out, arg or None, gx or None, ge or None) through the public function and its autograd"""
    xt, wt = dev(x).requires_grad_(x_grad), dev(w).requires_grad_(w_grad)
    res = gcn_amd.edge_aggregate(g.adj, xt, wt, op, act, reduce, return_arg=reduce in ("max", "min"))
    out, arg = res if isinstance(res, tuple) else (res, None)
    if x_grad or w_grad:
        out.backward(g_rows(g, gout))
    return out.detach(), arg, xt.grad, wt.grad


def assert_exact(g, got, want_live, what):
    want32 = np.asarray(want_live).astype(np.float32)
    assert np.array_equal(want32.astype(np.float64), np.asarray(want_live, np.float64)), "the reference is not on the fp32 grid"
    assert torch.equal(got[:len(want32)], dev(want32)), what
    assert int(torch.count_nonzero(got[len(want32):])) == 0, what + " (rows past the live ones)"


def assert_close(got, want, mag, what):
    err = np.abs(got.cpu().numpy().astype(np.float64)[:len(want)] - want)
    ratio = float((err / (1e-5 * mag + 1e-30)).max()) if err.size else 0.0
    print(f"[edge_aggregate] {what}: max error / bound = {ratio:.4f}")
    assert ratio <= 1.0, (what, ratio)
    assert int(torch.count_nonzero(got[len(want):])) == 0, what + " (rows past the live ones)"


def check_case(g, k, op, act, reduce, inputs, exact):
    x, w, gout = inputs
    what = f"{op}/{act}/{reduce} k={k}"
    out, arg, gx, ge = run(g, x, w, gout, op, act, reduce)
    if reduce in ("max", "min"):
        want, want_arg = ref.forward(g.rp, g.col, x, w, op, act, reduce)
        assert torch.equal(arg[:g.live], dev(want_arg, torch.int32)), what + " arg"
        assert bool((arg[g.live:] == -1).all()), what + " arg (rows past the live ones)"
        assert_exact(g, out, want, what + " out")              # a selection: exact on any inputs
        want_gx, mag_gx, want_ge = ref.backward_select(g.rp, g.col, g.n, x, w, gout, want_arg, op, act)
    else:
        want, mag = ref.forward(g.rp, g.col, x, w, op, act, "sum")
        if exact:
            assert_exact(g, out, want, what + " out")
        else:
            assert_close(out, want, mag, what + " out")
        want_gx, mag_gx, want_ge = ref.backward_sum(g.rp, g.col, g.n, x, w, gout, op, act)
    assert torch.equal(ge, dev(want_ge)), what + " ge"          # one product rounded once: the twin's bits on any inputs
    if exact:
        assert_exact(g, gx, want_gx, what + " gx")
    else:
        assert_close(gx, want_gx, mag_gx, what + " gx")


# ---- 1. the exact grid ---------------------------------------------------------------------------------------------------------
# (the twin takes about a second per million elements of edge_feat and message kind: the wide cases on the large graphs
# carry one kind each, the narrow ones all four)
GRID = ([("cora", k, OPS) for k in VEC4 + VEC1] +
        [("boundaries", k, OPS) for k in (4, 17, 1)] + [("boundaries", 64, TWO), ("boundaries", 68, TWO), ("boundaries", 128, [("add", None)]),
                                                        ("boundaries", 132, [("mul", None)]), ("boundaries", 256, [("mul", "relu")]),
                                                        ("boundaries", 260, [("add", "relu")]), ("boundaries", 65, [("mul", "relu")]),
                                                        ("boundaries", 33, [("add", "relu")])] +
        [("hubs", k, OPS) for k in (4, 5)] + [("hubs", 64, [("add", "relu")]), ("hubs", 33, [("mul", None)]), ("hubs", 17, [("add", None)])] +
        [("empty_tail", 4, OPS), ("empty_tail", 64, [("add", "relu")]), ("empty_tail", 3, TWO)])


@pytest.mark.parametrize("name,k,ops", GRID, ids=[f"{n}-k{k}-" + "+".join(f"{a}_{b}" for a, b in o) for n, k, o in GRID])
def test_exact_on_the_grid(name, k, ops):
    g = Graph.get(name)
    inputs = grid_inputs(g, k, seed=k)
    for op, act in ops:
        for reduce in ("sum", "max", "min"):
            check_case(g, k, op, act, reduce, inputs, exact=True)


@pytest.mark.parametrize("name,k", [("cora", 64), ("boundaries", 5), ("empty_tail", 4)])
def test_mean_is_the_sum_divided_once_by_the_row_length(name, k):
    g = Graph.get(name)
    x, w, gout = grid_inputs(g, k, seed=1)
    lens = np.maximum(np.diff(g.rp), 1)[:, None].astype(np.float32)
    cnt = torch.clamp(dev(np.diff(g.rowptr)), min=1)[:, None]
    for op, act in OPS:
        total, _, sgx, sge = run(g, x, w, gout / lens, op, act, "sum")
        mean, _, mgx, mge = run(g, x, w, gout, op, act, "mean")
        assert torch.equal(mean, total / cnt)                  # one fp32 IEEE division; an empty row: 0 / 1
        want = ref.forward(g.rp, g.col, x, w, op, act, "sum")[0].astype(np.float32) / lens      # (the sum is exact in fp32)
        assert torch.equal(mean[:g.live], dev(want)) and int(torch.count_nonzero(mean[g.live:])) == 0
        assert torch.equal(mgx, sgx) and torch.equal(mge, sge)  # the sum's kernels on g / len


# ---- 2. random inputs ----------------------------------------------------------------------------------------------------------
RANDOM = [("cora", 64), ("cora", 260), ("cora", 33), ("boundaries", 68), ("boundaries", 5), ("hubs", 16), ("empty_tail", 68)]


@pytest.mark.parametrize("name,k", RANDOM)
def test_random_inputs_selection_exact_and_sums_within_the_standing_bound(name, k):
    g = Graph.get(name)
    inputs = random_inputs(g, k, seed=100 + k)
    for op, act in (OPS if name == "cora" else TWO):
        for reduce in ("sum", "max", "min"):
            check_case(g, k, op, act, reduce, inputs, exact=False)


# ---- the element route by alignment: k = 64 with each operand in turn one element off a 16-byte boundary ---------------------------
def _raw(g, x, w, gout, op, act, reduce, shift):
    """the three kernels through the C ABI with the operand named `shift` one element past a 16-byte boundary; every
    tensor sits between guards"""
    adj, k = g.adj, x.shape[1]
    t = {}
    for name, src in (("x", x), ("w", w), ("g", gout), ("out", (g.m, k)), ("gx", (g.n, k)), ("ge", (g.nnz, k))):
        t[name] = offset_view(src, 1 if name == shift else 0, torch.float32, DEV)
    arg = torch.empty((g.m, k), dtype=torch.int32, device=DEV)
    ws = edgefeat._scratch(adj, k, torch.device(DEV))
    o = _lib.EDGE_OP_MUL if op == "mul" else _lib.EDGE_OP_ADD
    a = _lib.EDGE_ACT_RELU if act == "relu" else _lib.EDGE_ACT_NONE
    red = {"sum": _lib.REDUCE_SUM, "max": _lib.REDUCE_MAX, "min": _lib.REDUCE_MIN}[reduce]
    call("gcn_edge_aggregate_csr_f32", adj.rowptr, adj.col, g.m, g.n, g.nnz, t["x"][0], t["w"][0], k, o, a, red, t["out"][0], arg,
         ws, ws.numel(), device=torch.device(DEV))
    trowptr, trow, tperm = adj.tpattern()
    call("gcn_edge_aggregate_backward_x_csr_f32", trowptr, trow, tperm, g.n, g.m, g.nnz, t["g"][0], t["x"][0], t["w"][0], k, o, a,
         t["gx"][0], ws, ws.numel(), device=torch.device(DEV))
    call("gcn_edge_aggregate_backward_e_csr_f32", adj.rowptr, adj.col, g.m, g.n, g.nnz, t["g"][0], t["x"][0], t["w"][0], k, o, a,
         t["ge"][0], ws, ws.numel(), device=torch.device(DEV))
    torch.cuda.synchronize()
    for name, (view, flat) in t.items():
        assert guards_intact(flat, view), f"{name} guards with {shift} shifted"
    return t["out"][0], arg, t["gx"][0], t["ge"][0]


@pytest.mark.parametrize("shift", ["x", "w", "g", "out", "gx", "ge"])
@pytest.mark.parametrize("name", ["cora", "boundaries"])
def test_k64_with_one_operand_shifted_by_one_element_is_exact(name, shift):
    g = Graph.get(name)
    x, w, gout = grid_inputs(g, 64, seed=7)
    assert edgefeat.route(64, offset_view((4,), 1, torch.float32, DEV)[0]) == (1, 64, 1)
    for op, act in TWO:
        out, _arg, gx, ge = _raw(g, x, w, gout, op, act, "sum", shift)
        want, _ = ref.forward(g.rp, g.col, x, w, op, act, "sum")
        want_gx, _, want_ge = ref.backward_sum(g.rp, g.col, g.n, x, w, gout, op, act)
        assert_exact(g, out, want, f"out, {shift} shifted")
        assert_exact(g, gx, want_gx, f"gx, {shift} shifted")
        assert torch.equal(ge, dev(want_ge)), f"ge, {shift} shifted"
    if shift in ("x", "w", "out"):
        out, arg, _gx, _ge = _raw(g, x, w, gout, "mul", "relu", "max", shift)
        want, want_arg = ref.forward(g.rp, g.col, x, w, "mul", "relu", "max")
        assert torch.equal(out, dev(want)) and torch.equal(arg, dev(want_arg, torch.int32))


# ---- 3. non-finite inputs ----------------------------------------------------------------------------------------------------------
def _same_bits_up_to_nan(got, want):
    got, want = got.cpu().numpy(), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.int32), want[~nan].view(np.int32))


@pytest.mark.parametrize("k", [8, 5])
def test_non_finite_inputs_follow_the_twin(k):
    g = Graph.get("small")
    x, w, _ = grid_inputs(g, k, seed=2)
    rng = np.random.default_rng(12)
    for a in (x, w):
        hit = rng.random(a.shape)
        a[hit < 0.004] = np.nan
        a[(hit >= 0.004) & (hit < 0.008)] = np.inf
        a[(hit >= 0.008) & (hit < 0.012)] = -np.inf
        a[(hit >= 0.012) & (hit < 0.03)] = -0.0
    xt, wt = dev(x), dev(w)
    for op, act in OPS:
        msg = ref.messages(g.col, x, w, op, act)
        assert np.isnan(msg).any() and np.isinf(msg).any() and (np.signbit(msg) & (msg == 0)).any()
        for reduce in ("max", "min"):
            out, arg = gcn_amd.edge_aggregate(g.adj, xt, wt, op, act, reduce, return_arg=True)
            want, want_arg = ref.forward(g.rp, g.col, x, w, op, act, reduce)
            assert torch.equal(arg, dev(want_arg, torch.int32)), (op, act, reduce)     # the first NaN of a (row, column) wins
            assert _same_bits_up_to_nan(out, want), (op, act, reduce)
            assert np.isnan(want).sum() >= 10
        out = gcn_amd.edge_aggregate(g.adj, xt, wt, op, act, "sum")
        want, _ = ref.forward(g.rp, g.col, x, w, op, act, "sum")
        got, nan = out.cpu().numpy(), np.isnan(want)            # NaN where the twin has one (a NaN message, or +Inf meeting
        assert np.array_equal(np.isnan(got), nan), (op, act)    # -Inf), +-Inf where it has one, the exact sum elsewhere (a
        assert np.array_equal(got[~nan].astype(np.float64), want[~nan]), (op, act)     # zero sum's sign is the chain's, not compared)
        assert np.isinf(want).any() and nan.any()


def test_relu_keeps_nan_and_plus_inf_and_maps_minus_inf_to_zero():
    rowptr = np.arange(7, dtype=np.int64)                      # six rows of one entry: out is the message itself
    g = Graph(rowptr, np.arange(6), 6)
    x = np.array([[np.nan], [np.inf], [-np.inf], [-0.0], [-2.0], [3.0]], np.float32)
    for op, w in (("add", np.zeros((6, 1), np.float32)), ("mul", np.ones((6, 1), np.float32))):
        for reduce in ("sum", "max", "min"):
            out = gcn_amd.edge_aggregate(g.adj, dev(x), dev(w), op, "relu", reduce).cpu().numpy()[:, 0]
            assert np.isnan(out[0]) and out[1] == np.inf and out[2] == 0 and not np.signbit(out[2]), (op, reduce, out)
            assert out[4] == 0 and not np.signbit(out[4]) and out[5] == 3
            if op == "mul":                                    # (-0.0 + 0.0 is +0.0 before the relu sees it)
                assert out[3] == 0 and np.signbit(out[3]) == (reduce != "sum"), (reduce, out)     # a sum starts from +0
    # the derivative: a NaN passes the gradient, t <= 0 blocks it (and selects: an infinite g gives a zero, not a NaN)
    xt, wt = dev(x).requires_grad_(), dev(np.zeros((6, 1), np.float32)).requires_grad_()
    gcn_amd.edge_aggregate(g.adj, xt, wt, "add", "relu", "sum").backward(dev(np.full((6, 1), np.inf, np.float32)))
    for grad in (xt.grad.cpu().numpy()[:, 0], wt.grad.cpu().numpy()[:, 0]):
        assert list(grad) == [np.inf, np.inf, 0, 0, 0, np.inf]


@pytest.mark.parametrize("k", [64, 5])
def test_a_nan_message_poisons_only_its_own_row_and_column(k):
    g = Graph.get("small")
    x, w, _ = grid_inputs(g, k, seed=3)
    rows = ref.entry_rows(g.rp)
    for e, j, side in ((int(g.rp[4]) + 2000, k - 1, "w"), (int(g.rp[250]) + 3, 0, "w"), (int(g.rp[4]) + 5, 1, "x")):
        for op, act in TWO:
            clean = gcn_amd.edge_aggregate(g.adj, dev(x), dev(w), op, act, "sum")
            x2, w2 = x.copy(), w.copy()
            if side == "w":
                w2[e, j] = np.nan
                hit = np.zeros((g.m, k), bool)
                hit[rows[e], j] = True
            else:                                              # a NaN in x reaches every row that stores the column
                x2[g.col[e], j] = np.nan
                hit = np.zeros((g.m, k), bool)
                hit[rows[g.col == g.col[e]], j] = True
            for reduce in ("sum", "max", "min"):
                base = gcn_amd.edge_aggregate(g.adj, dev(x), dev(w), op, act, reduce)
                out = gcn_amd.edge_aggregate(g.adj, dev(x2), dev(w2), op, act, reduce)
                assert np.array_equal(torch.isnan(out).cpu().numpy(), hit), (side, op, act, reduce)
                assert torch.equal(out[~dev(hit, torch.bool)], base[~dev(hit, torch.bool)])
            assert not bool(torch.isnan(clean).any())


# ---- 4. the contract -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduce", ["sum", "mean", "max", "min"])
def test_two_calls_same_bits_frozen_operands_views_and_repeated_backward(reduce):
    g = Graph.get("hubs")
    k = 68
    x, w, gout = random_inputs(g, k, seed=5)
    for op, act in TWO:
        out, arg, gx, ge = run(g, x, w, gout, op, act, reduce)
        out2, arg2, gx2, ge2 = run(g, x, w, gout, op, act, reduce)
        assert torch.equal(out, out2) and torch.equal(gx, gx2) and torch.equal(ge, ge2)
        assert arg is None or torch.equal(arg, arg2)
        # out and a gradient do not depend on whether the other operand asks for one
        ox, _, gx3, none_e = run(g, x, w, gout, op, act, reduce, w_grad=False)
        oe, _, none_x, ge3 = run(g, x, w, gout, op, act, reduce, x_grad=False)
        o0 = run(g, x, w, gout, op, act, reduce, x_grad=False, w_grad=False)[0]
        assert none_e is None and none_x is None
        assert torch.equal(ox, out) and torch.equal(oe, out) and torch.equal(o0, out)
        assert torch.equal(gx3, gx) and torch.equal(ge3, ge)
        # non-contiguous views of x and edge_feat
        xw = torch.zeros(g.n, 2 * k, device=DEV)
        xw[:, ::2] = dev(x)
        xv = xw[:, ::2].requires_grad_()
        wv = dev(w).t().contiguous().t().requires_grad_()
        assert not xv.is_contiguous() and not wv.is_contiguous()
        ov = gcn_amd.edge_aggregate(g.adj, xv, wv, op, act, reduce)
        # backward twice with retain_graph: the second adds the same gradient again
        ov.backward(g_rows(g, gout), retain_graph=True)
        assert torch.equal(ov.detach(), out) and torch.equal(xv.grad, gx) and torch.equal(wv.grad, ge)
        ov.backward(g_rows(g, gout))
        assert torch.equal(xv.grad, gx + gx) and torch.equal(wv.grad, ge + ge)


def test_rows_past_the_live_ones_are_zero_and_take_no_gradient():
    g = Graph.get("empty_tail")
    x, w, _ = random_inputs(g, 16, seed=6)
    gout = torch.ones(g.m, 16, device=DEV)                     # a gradient on the empty rows too
    for reduce in ("sum", "mean", "max", "min"):
        xt, wt = dev(x).requires_grad_(), dev(w).requires_grad_()
        res = gcn_amd.edge_aggregate(g.adj, xt, wt, "add", "relu", reduce, return_arg=reduce in ("max", "min"))
        out, arg = res if isinstance(res, tuple) else (res, None)
        assert int(torch.count_nonzero(out[g.live:])) == 0 and (arg is None or bool((arg[g.live:] == -1).all()))
        out.backward(gout)
        lone = torch.ones(g.live, 16, device=DEV)
        xl, wl = dev(x).requires_grad_(), dev(w).requires_grad_()
        live_adj = gcn_amd.CsrAdjacency(dev(g.rp, torch.int32), dev(g.col, torch.int32), torch.ones(g.nnz, device=DEV), (g.live, g.n))
        gcn_amd.edge_aggregate(live_adj, xl, wl, "add", "relu", reduce).backward(lone)
        assert torch.equal(xt.grad, xl.grad) and torch.equal(wt.grad, wl.grad)


@pytest.mark.parametrize("op,act,reduce", [("add", "relu", "sum"), ("mul", None, "max"), ("mul", "relu", "mean")])
def test_forward_and_backward_capture_and_replay_bit_for_bit(op, act, reduce):
    g = Graph.get("boundaries")
    k = 64
    gen = np.random.default_rng(9)
    x = dev(gen.standard_normal((g.n, k)).astype(np.float32)).requires_grad_()
    w = dev(gen.standard_normal((g.nnz, k)).astype(np.float32)).requires_grad_()
    gout = dev(gen.standard_normal((g.m, k)).astype(np.float32))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):                                     # the transposed pattern, the row counts and the workspaces now exist
            x.grad = w.grad = None
            gcn_amd.edge_aggregate(g.adj, x, w, op, act, reduce).backward(gout)
    torch.cuda.current_stream().wait_stream(side)
    x.grad = w.grad = None
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_):
        out = gcn_amd.edge_aggregate(g.adj, x, w, op, act, reduce)
        out.backward(gout)
    for _rep in range(2):
        with torch.no_grad():
            x.copy_(dev(gen.standard_normal((g.n, k)).astype(np.float32)))
            w.copy_(dev(gen.standard_normal((g.nnz, k)).astype(np.float32)))
            gout.copy_(dev(gen.standard_normal((g.m, k)).astype(np.float32)))
        graph_.replay()
        torch.cuda.synchronize()
        got = [out.clone(), x.grad.clone(), w.grad.clone()]
        xe, we = x.detach().clone().requires_grad_(), w.detach().clone().requires_grad_()
        oe = gcn_amd.edge_aggregate(g.adj, xe, we, op, act, reduce)
        oe.backward(gout)
        torch.cuda.synchronize()
        for u, v in zip(got, [oe.detach(), xe.grad, we.grad]):
            assert torch.equal(u, v)


# ---- 5. autograd against the fp64 torch formulation -------------------------------------------------------------------------------
def _torch_formulation(g, x, w, gout, op, act, reduce):
    """(out, gx, ge, sums of |terms| of out and gx) in fp64 on the device: (x[col] op w).relu() reduced with index_add_ /
    scatter_reduce"""
    rows = dev(ref.entry_rows(g.rowptr), torch.int64)
    col = dev(g.col, torch.int64)
    xt, wt = dev(x, torch.float64).requires_grad_(), dev(w, torch.float64).requires_grad_()
    msg = xt[col] * wt if op == "mul" else xt[col] + wt
    if act == "relu":
        msg = msg.relu()
    k = x.shape[1]
    if reduce in ("sum", "mean"):
        out = torch.zeros(g.m, k, dtype=torch.float64, device=DEV).index_add_(0, rows, msg)
        if reduce == "mean":
            out = out / torch.clamp(dev(np.diff(g.rowptr), torch.float64), min=1)[:, None]
    else:
        out = torch.zeros(g.m, k, dtype=torch.float64, device=DEV).scatter_reduce(
            0, rows[:, None].expand(-1, k), msg, "amax" if reduce == "max" else "amin", include_self=False)
    out.backward(g_rows(g, gout).double())
    return out.detach(), xt.grad, wt.grad


@pytest.mark.parametrize("reduce", ["sum", "mean", "max", "min"])
@pytest.mark.parametrize("op,act", OPS)
@pytest.mark.parametrize("name", ["cora", "boundaries"])
def test_autograd_matches_the_fp64_torch_formulation(name, op, act, reduce):
    g = Graph.get(name)
    k = 12
    x, w, gout = random_inputs(g, k, seed=21)
    out, _arg, gx, ge = run(g, x, w, gout, op, act, reduce)
    want, want_gx, want_ge = _torch_formulation(g, x, w, gout, op, act, reduce)
    # the scale of a row's (a column's) terms: what the standing bound 1e-5 * sum |terms| is taken of
    rows, col = dev(ref.entry_rows(g.rowptr), torch.int64), dev(g.col, torch.int64)
    amsg = (dev(x, torch.float64)[col] * dev(w, torch.float64)).abs() if op == "mul" else dev(x, torch.float64)[col].abs() + dev(w, torch.float64).abs()
    mag = torch.zeros(g.m, k, dtype=torch.float64, device=DEV).index_add_(0, rows, amsg)
    if reduce in ("max", "min"):                           # the gradient goes to the selected entries: their terms alone
        _, want_arg = ref.forward(g.rp, g.col, x, w, op, act, reduce)
        mag_gx = dev(ref.backward_select(g.rp, g.col, g.n, x, w, gout, want_arg, op, act)[1], torch.float64)
    else:
        gterm = g_rows(g, gout).double().abs()[rows] * (dev(w, torch.float64).abs() if op == "mul" else 1.0)
        if reduce == "mean":
            cnt = torch.clamp(dev(np.diff(g.rowptr), torch.float64), min=1)[:, None]
            mag, gterm = mag / cnt, gterm / cnt[rows]
        mag_gx = torch.zeros(g.n, k, dtype=torch.float64, device=DEV).index_add_(0, col, gterm)
    # (an element of ge is one product, or two operations under the mean: its own magnitude is its sum of |terms|)
    for got, ref64, scale, what in ((out, want, mag, "out"), (gx, want_gx, mag_gx, "gx"), (ge, want_ge, want_ge.abs(), "ge")):
        ratio = float(((got.double() - ref64).abs() / (1e-5 * scale + 1e-30)).max())
        print(f"[edge_aggregate] {name} {op}/{act}/{reduce} {what} against fp64 autograd: max error / bound = {ratio:.4f}")
        assert ratio <= 1.0, (what, ratio)


# ---- 6. the layers -----------------------------------------------------------------------------------------------------------------
def _net(i, h, o, seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(i, h), torch.nn.ReLU(), torch.nn.Linear(h, o))


def _dense_gine(layer64, x, x_dst, rowptr, col, edge_attr):
    """PyG's formula in fp64: nn((1 + eps) * x_dst + sum_j relu(x_j + e_ji))"""
    rows = dev(ref.entry_rows(rowptr), torch.int64)
    e = layer64.lin(edge_attr) if layer64.lin is not None else edge_attr
    msg = (x[dev(col, torch.int64)] + e).relu()
    agg = torch.zeros(len(rowptr) - 1, x.shape[1], dtype=torch.float64, device=DEV).index_add_(0, rows, msg)
    return layer64.nn((1.0 + layer64.eps) * x_dst + agg)


@pytest.mark.parametrize("edge_dim", [None, 5])
def test_gine_conv_matches_the_dense_fp64_restatement(edge_dim):
    import copy
    g = Graph.get("cora")
    layer = gcn_amd.GINEConv(_net(16, 24, 7, seed=1), eps=0.3, train_eps=True, edge_dim=edge_dim).to(DEV)
    layer64 = copy.deepcopy(layer).double()
    gen = np.random.default_rng(2)
    x = gen.standard_normal((g.n, 16)).astype(np.float32)
    ea = gen.standard_normal((g.nnz, edge_dim or 16)).astype(np.float32)
    gout = gen.standard_normal((g.m, 7)).astype(np.float32)
    xt, et = dev(x).requires_grad_(), dev(ea).requires_grad_()
    out = layer(xt, g.adj, et)
    out.backward(dev(gout))
    x64, e64 = dev(x, torch.float64).requires_grad_(), dev(ea, torch.float64).requires_grad_()
    want = _dense_gine(layer64, x64, x64, g.rowptr, g.col, e64)
    want.backward(dev(gout, torch.float64))
    pairs = [(out, want, "out"), (xt.grad, x64.grad, "grad x"), (et.grad, e64.grad, "grad edge_attr")]
    pairs += [(p.grad, q.grad, "grad " + n) for (n, p), (_, q) in zip(layer.named_parameters(), layer64.named_parameters())]
    assert {n for n, _ in layer.named_parameters()} >= {"eps", "nn.0.weight", "nn.2.bias"}
    for got, ref64, what in pairs:
        err = float((got.double() - ref64).abs().max()) / max(float(ref64.abs().max()), 1e-30)
        print(f"[edge_aggregate] GINEConv edge_dim={edge_dim} {what}: rel. error {err:.2e}")
        assert err <= 1e-5, (what, err)


def test_gine_conv_on_sampled_blocks_with_the_parents_edge_attributes():
    import copy
    g = Graph.get("cora")
    layer = gcn_amd.GINEConv(_net(8, 12, 4, seed=3), eps=0.1).to(DEV)
    layer64 = copy.deepcopy(layer).double()
    gen = np.random.default_rng(4)
    x, ea = gen.standard_normal((g.n, 8)).astype(np.float32), gen.standard_normal((g.nnz, 8)).astype(np.float32)
    seeds = dev(np.arange(0, g.n, 9), torch.int64)
    blocks, input_ids = gcn_amd.sample_blocks(g.adj, seeds, [4, -1], seed=11)
    edge_attr = dev(ea)
    for block in blocks:
        src = dev(x)[block.src_ids]
        out = layer((src, src[:block.num_dst]), block.adj, edge_attr[block.eid.long()])
        rp, col = block.adj.rowptr.cpu().numpy().astype(np.int64), block.adj.col.cpu().numpy().astype(np.int64)
        src64 = src.double()
        want = _dense_gine(layer64, src64, src64[:block.num_dst], rp, col, edge_attr.double()[block.eid.long()])
        assert out.shape == (block.num_dst, 4) and block.adj.nnz > 0
        assert float((out.double() - want).abs().max()) <= 1e-5 * max(float(want.abs().max()), 1.0)
    assert torch.equal(input_ids, blocks[0].src_ids)


def test_gine_conv_with_zero_edge_attr_and_no_negative_x_equals_gin_conv():
    g = Graph.get("cora")
    net = _net(16, 16, 16, seed=5).to(DEV)
    gine, gin = gcn_amd.GINEConv(net, eps=0.2).to(DEV), gcn_amd.GINConv(net, eps=0.2).to(DEV)
    x = dev(np.random.default_rng(6).integers(0, 4, (g.n, 16)).astype(np.float32))     # small integers: both sums are exact
    a, b = gine(x, g.adj, torch.zeros(g.nnz, 16, device=DEV)), gin(x, g.adj)
    assert torch.equal(a, b)
