"""Max / min / sum / mean neighbourhood aggregation on the GPU (gcn_amd/csrc/aggregate.hip, gcn_amd.aggregate, SAGEConv).

References are numpy: per row, np.argmax / np.argmin over the gathered slab x[col[b:e]] — the first of equal values
(-0.0 == +0.0) and the first NaN, exactly the kernel's rule — so `out` is compared BY BITS and `arg` for equality; the
backward is np.add.at on col[arg] with small-integer gradients, whose fp32 sums are exact in any order.  Most features
are integers in [-2, 2], so nearly every element is a tie.  The graphs put rows on both sides of every threshold of the
dispatch (a slot of 4 entries, a batch of 64, the 4096-entry long-row threshold and chunk), start a long row on a chunk
boundary and inside a chunk, and end with empty rows.

Autograd (continuous features, no ties) is compared with fp64 torch on dense tensors: max / min over the neighbourhoods
padded to the longest row, a dense [n, longest, k] tensor (the n x n x k one does not fit; the Cora-shaped graph's longest
row has 14 entries), sum / mean through the dense m x n count matrix.  Tolerances: selected values exact; products and
gradients 1e-5 * sum|terms| + 1e-30 (the SDDMM's figure); a 20-step Adam loss trajectory 1e-4 relative."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gcn_amd
from gcn_amd import _lib, graphgen
from util import (BF16_EPS, assert_elementwise, guards_intact, offset_view, oracle_spmm, random_csr, with_duplicate_entries,
                  with_duplicates)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CHUNK = 4096
WIDTHS = [1, 3, 16, 33, 64, 65, 128, 200]
_cache = {}


def _csr_from_lens(lens, n, seed):
    rng = np.random.default_rng(seed)
    rowptr = np.zeros(len(lens) + 1, np.int64)
    rowptr[1:] = np.cumsum(lens)
    col = rng.integers(0, n, rowptr[-1]).astype(np.int32)      # (duplicates allowed: each stored entry is its own)
    return rowptr.astype(np.int32), col, n


def graph(name):
    """name -> (rowptr int32 [m+1], col int32 [nnz], n)"""
    if name in _cache:
        return _cache[name]
    if name == "boundaries":
        # 4096 entries first, so the 4097-entry row starts ON a chunk boundary; the later long rows start inside chunks
        lens = [4096, 4097, 0, 1, 3, 4, 5, 0, 0, 63, 64, 65, 0, 127, 128, 129, 4095, 0, 4096, 4097, 8192, 0, 8193, 12289, 2, 0,
                0, 0, 0, 0, 0, 0, 0, 0, 0, 16, 17, 0, 1] + [0] * 21
        g = _csr_from_lens(np.array(lens, np.int64), 3000, 6)
    elif name == "hubs":                               # 30 % empty rows, hub rows of about 5 000 and 300 000 entries
        rng = np.random.default_rng(5)
        lens = rng.poisson(10, 3000)
        lens[rng.random(3000) < 0.3] = 0
        lens[7], lens[1500] = 5000, 300000
        g = _csr_from_lens(lens, 20000, 7)
    elif name == "one_row":                            # a single row holding every entry
        g = _csr_from_lens(np.array([50000], np.int64), 7000, 8)
    elif name == "cora":
        rp, col, _v, n = graphgen.make_graph("cora", device="cpu", seed=1)
        g = (rp.numpy(), col.numpy(), n)
    elif name == "rect":                               # m != n, not symmetric, empty rows, hub rows, duplicated entries
        rp, col, va = random_csr(700, 1300, 30000, seed=5, empty_rows=0.1, long_rows=((3, 400), (10, 900)))
        rp, col, _v = with_duplicate_entries(rp, col, va)
        g = (rp, col, 1300)
    elif name.endswith("_T"):                          # the transpose: the long ROWS of the base graph become hub COLUMNS
        rp0, col0, n0 = graph(name[:-2])
        m0 = len(rp0) - 1
        order = np.argsort(col0, kind="stable")
        rp = np.zeros(n0 + 1, np.int64)
        rp[1:] = np.cumsum(np.bincount(col0, minlength=n0))
        g = (rp.astype(np.int32), np.repeat(np.arange(m0, dtype=np.int32), np.diff(rp0))[order], m0)
        assert np.array_equal(np.bincount(g[1], minlength=m0), np.diff(rp0))
    else:
        raise KeyError(name)
    _cache[name] = g
    return g


GRAPHS = ["boundaries", "hubs", "one_row", "cora"]
# The backward walks the TRANSPOSED pattern, whose row lengths are the column counts — at most 42 in the graphs above,
# whose columns are drawn uniformly.  The transposes turn that round: their columns are listed by exactly the base
# graph's row lengths, so the backward's walk meets every length of "boundaries" (both sides of 4, 64 and 4096, 8192,
# 8193, 12289, one long column starting on a chunk boundary of the transpose and the others inside chunks), the 5 000-
# and 300 000-entry hubs, and one column holding every entry (all of them duplicates of one (row, column) pair per row).
HUB_COLUMN_GRAPHS = ["boundaries_T", "hubs_T", "one_row_T"]


def make_adj(name, mutable=False):
    rp, col, n = graph(name)
    return gcn_amd.CsrAdjacency(torch.from_numpy(rp).to(DEV), torch.from_numpy(col).to(DEV), torch.ones(len(col), device=DEV),
                                (len(rp) - 1, n), mutable_values=mutable)


def level_features(n, k, seed, dtype=np.float32):
    """integers in [-2, 2]: five levels, so nearly every element of a row of more than a few entries is a tie"""
    return np.random.default_rng(seed).integers(-2, 3, (n, k)).astype(dtype)


def ref_select(rp, col, x, op):
    """(out, arg) by numpy: first maximum / minimum (first NaN) of every column of each row's slab; empty rows 0 and -1"""
    m, k = len(rp) - 1, x.shape[1]
    out = np.zeros((m, k), x.dtype)
    arg = np.full((m, k), -1, np.int32)
    pick = np.argmax if op == "max" else np.argmin
    jj = np.arange(k)
    for r in range(m):
        b, e = int(rp[r]), int(rp[r + 1])
        if e > b:
            slab = x[col[b:e]]
            a = pick(slab, axis=0)
            out[r] = slab[a, jj]
            arg[r] = b + a
    return out, arg


def ref_select_cached(name, k, op):
    key = ("ref", name, k, op)
    if key not in _cache:
        rp, col, n = graph(name)
        _cache[key] = ref_select(rp, col, level_features(n, k, seed=k), op)
    return _cache[key]


def bits(a):
    a = a.detach().cpu() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return a.contiguous().view(torch.int16 if a.element_size() == 2 else torch.int32).numpy()


def assert_select(out, arg, ref_out, ref_arg, what):
    got_arg = arg.cpu().numpy()
    bad = np.argwhere(got_arg != ref_arg)
    assert len(bad) == 0, f"{what}: arg differs at {len(bad)} elements, first {tuple(bad[0])}: {got_arg[tuple(bad[0])]} != {ref_arg[tuple(bad[0])]}"
    assert np.array_equal(bits(out), bits(ref_out)), f"{what}: out differs by bits"


def ref_backward(col, n, arg, g):
    """gx[col[arg[r, j]], j] += g[r, j] in fp64"""
    gx = np.zeros((n, g.shape[1]), np.float64)
    rr, jj = np.nonzero(arg >= 0)
    np.add.at(gx, (col[arg[rr, jj]], jj), g[rr, jj].astype(np.float64))
    return gx


def int_grad(m, k, seed, top=8):
    return np.random.default_rng(seed).integers(-top, top + 1, (m, k)).astype(np.float32)


# ---- 1. forward: bit-exact out, equal arg ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k", WIDTHS)
@pytest.mark.parametrize("name", GRAPHS)
def test_forward_is_numpy_argmax_bit_for_bit(name, k):
    adj = make_adj(name)
    x = torch.from_numpy(level_features(adj.n, k, seed=k)).to(DEV)
    for op in ("max", "min"):
        out, arg = gcn_amd.aggregate(adj, x, op, return_arg=True)
        assert out.dtype == torch.float32 and arg.dtype == torch.int32 and out.shape == arg.shape == (adj.m, k)
        assert not arg.requires_grad
        assert_select(out, arg, *ref_select_cached(name, k, op), f"{name} k={k} {op}")
        assert torch.equal(gcn_amd.aggregate(adj, x, op), out)


# ---- 2. special values ----------------------------------------------------------------------------------------------------
def _special(name, k, edit, seed):
    rp, col, n = graph(name)
    x = level_features(n, k, seed)
    edit(x, rp, col)
    adj = make_adj(name)
    for op in ("max", "min"):
        out, arg = gcn_amd.aggregate(adj, torch.from_numpy(x).to(DEV), op, return_arg=True)
        ref_out, ref_arg = ref_select(rp, col, x, op)
        assert_select(out, arg, ref_out, ref_arg, f"{name} {op}")
        yield op, x, out.cpu().numpy(), arg.cpu().numpy(), rp, col


def test_a_nan_poisons_exactly_the_rows_that_list_it():
    src = int(graph("boundaries")[1][4096 + 2000])      # a column the chunk-aligned long row lists (and others do)

    def edit(x, rp, col):
        x[src, :] = np.nan
    for _op, x, out, arg, rp, col in _special("boundaries", 33, edit, seed=1):
        rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
        listed = np.zeros(len(rp) - 1, bool)
        listed[rows[col == src]] = True
        assert listed.sum() >= 3 and (~listed).sum() >= 3
        assert np.array_equal(np.isnan(out).all(axis=1), listed) and np.array_equal(np.isnan(out).any(axis=1), listed)
        first = {r: int(np.flatnonzero(col[rp[r]:rp[r + 1]] == src)[0]) + int(rp[r]) for r in np.flatnonzero(listed)}
        for r, e in first.items():
            assert (arg[r] == e).all(), (r, e)


def test_infinities_are_ordinary_values():
    def edit(x, rp, col):
        x[:, 0] = -np.inf                               # column 0: every row is all -inf
        x[:, 1] = np.inf                                # column 1: all +inf
        x[::3, 2] = np.inf                              # +inf and -inf beside finite values
        x[1::3, 3] = -np.inf
    for op, x, out, arg, rp, col in _special("boundaries", 5, edit, seed=2):
        ne = np.diff(rp) > 0
        assert (out[ne, 0] == -np.inf).all() and (arg[ne, 0] == rp[:-1][ne]).all()   # the first entry of the row
        assert (out[ne, 1] == np.inf).all() and (arg[ne, 1] == rp[:-1][ne]).all()
        assert (out[~ne] == 0).all() and (arg[~ne] == -1).all()


def test_signed_zeros_tie_and_the_first_ones_bits_are_returned():
    def edit(x, rp, col):
        rng = np.random.default_rng(3)
        x[:] = np.where(rng.random(x.shape) < 0.5, np.float32(-0.0), np.float32(0.0))
    seen = set()
    for _op, x, out, arg, rp, col in _special("boundaries", 16, edit, seed=3):
        ne = np.diff(rp) > 0
        assert (arg[ne] == rp[:-1][ne, None]).all()     # everything ties: the first entry, whatever its sign
        first = x[col[rp[:-1][ne]]]
        assert np.array_equal(bits(out[ne]), bits(first))
        seen |= set(np.unique(bits(out[ne])).tolist())
    assert seen == {0, -2 ** 31}                        # both zeros came back


def test_no_rows_and_no_entries():
    x = torch.from_numpy(level_features(9, 5, seed=4)).to(DEV).requires_grad_(True)
    empty_i = torch.zeros(0, dtype=torch.int32, device=DEV)
    empty_f = torch.zeros(0, device=DEV)
    for op in ("max", "min"):
        a0 = gcn_amd.CsrAdjacency(torch.zeros(1, dtype=torch.int32, device=DEV), empty_i, empty_f, (0, 9))
        out, arg = gcn_amd.aggregate(a0, x, op, return_arg=True)
        assert out.shape == (0, 5) and arg.shape == (0, 5)
        out.sum().backward()
        assert torch.equal(x.grad, torch.zeros_like(x))
        x.grad = None
        a1 = gcn_amd.CsrAdjacency(torch.zeros(7, dtype=torch.int32, device=DEV), empty_i, empty_f, (6, 9))
        out, arg = gcn_amd.aggregate(a1, x, op, return_arg=True)
        assert (bits(out) == 0).all() and (arg == -1).all() and out.shape == (6, 5)
        out.backward(torch.ones_like(out))
        assert torch.equal(x.grad, torch.zeros_like(x))
        x.grad = None
    for reduce in ("sum", "mean"):
        assert torch.equal(gcn_amd.aggregate(a1, x.detach(), reduce), torch.zeros(6, 5, device=DEV))


# ---- 3. duplicated columns ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 64])
def test_duplicates_first_copy_wins_and_gets_the_gradient_once(k):
    rp0, col0, n = graph("cora")
    rp, col, _v = with_duplicates(rp0, col0, np.ones(len(col0), np.float32), seed=9)
    assert len(col) > len(col0)
    m = len(rp) - 1
    dup_of_prev = np.zeros(len(col), bool)
    dup_of_prev[1:] = (col[1:] == col[:-1]) & (np.repeat(np.arange(m), np.diff(rp))[1:] == np.repeat(np.arange(m), np.diff(rp))[:-1])
    for mutable in (False, True):
        adj = gcn_amd.CsrAdjacency(torch.from_numpy(rp).to(DEV), torch.from_numpy(col).to(DEV), torch.ones(len(col), device=DEV),
                                   (m, n), mutable_values=mutable)
        x = level_features(n, k, seed=10)
        g = int_grad(m, k, seed=11)
        for op in ("max", "min"):
            xd = torch.from_numpy(x).to(DEV).requires_grad_(True)
            out, arg = gcn_amd.aggregate(adj, xd, op, return_arg=True)
            ref_out, ref_arg = ref_select(rp, col, x, op)
            assert_select(out, arg, ref_out, ref_arg, f"duplicates {op}")
            assert not dup_of_prev[ref_arg[ref_arg >= 0]].any()         # never a later copy
            out.backward(torch.from_numpy(g).to(DEV))
            assert np.array_equal(xd.grad.cpu().numpy().astype(np.float64), ref_backward(col, n, ref_arg, g))


# ---- 4. backward, bit-exact -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 33, 64, 200])
@pytest.mark.parametrize("name", GRAPHS + ["rect"])
def test_backward_is_exact_and_repeats_bit_for_bit(name, k):
    # the mutable adjacency's own transpose and permutation
    _check_backward(name, k, mutable=name in ("rect", "cora") and k in (33, 64))


@pytest.mark.parametrize("k", [3, 64])                 # one element per lane, and 16-byte loads
@pytest.mark.parametrize("name", HUB_COLUMN_GRAPHS)
def test_backward_over_hub_columns_is_exact_and_repeats_bit_for_bit(name, k):
    rp, col, n = graph(name)
    assert np.bincount(col, minlength=n).max() > 2 * CHUNK              # the long-row kernels of the backward run
    _check_backward(name, k, mutable=name == "boundaries_T" and k == 64)


def _check_backward(name, k, mutable):
    rp, col, n = graph(name)
    adj = make_adj(name, mutable=mutable)
    x = level_features(n, k, seed=k)
    g = int_grad(adj.m, k, seed=k + 1)
    gd = torch.from_numpy(g).to(DEV)
    for op in ("max", "min"):
        xd = torch.from_numpy(x).to(DEV).requires_grad_(True)
        out, arg = gcn_amd.aggregate(adj, xd, op, return_arg=True)
        ref_arg = (ref_select_cached(name, k, op) if name != "rect" else ref_select(rp, col, x, op))[1]
        assert np.array_equal(arg.cpu().numpy(), ref_arg)
        (gx1,) = torch.autograd.grad(out, xd, gd, retain_graph=True)
        (gx2,) = torch.autograd.grad(out, xd, gd)
        ref = ref_backward(col, n, ref_arg, g)
        assert np.abs(ref).max() < 2 ** 24
        assert gx1.shape == (n, k) and gx1.dtype == torch.float32
        assert np.array_equal(gx1.cpu().numpy().astype(np.float64), ref), f"{name} k={k} {op}"
        assert np.array_equal(bits(gx1), bits(gx2))


# ---- 5. bf16 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 64, 128, 200])
@pytest.mark.parametrize("name", ["boundaries", "cora"])
def test_bf16_forward_and_backward(name, k):
    rp, col, n = graph(name)
    adj = make_adj(name)
    gen = torch.Generator().manual_seed(k)
    xb = torch.randn(n, k, generator=gen).to(torch.bfloat16)
    xb[::2] = torch.from_numpy(level_features(n, k, seed=k))[::2].to(torch.bfloat16)      # half of the rows: ties
    x32 = xb.float().numpy()
    lens_in = np.bincount(col, minlength=n)
    for op in ("max", "min"):
        xd = xb.to(DEV).requires_grad_(True)
        out, arg = gcn_amd.aggregate(adj, xd, op, return_arg=True)
        assert out.dtype == torch.bfloat16
        ref_out, ref_arg = ref_select(rp, col, x32, op)
        assert np.array_equal(arg.cpu().numpy(), ref_arg)
        assert np.array_equal(bits(out), bits(torch.from_numpy(ref_out).to(torch.bfloat16)))
        assert np.array_equal(out.detach().float().cpu().numpy(), ref_out)
        # integer gradients in {-1, 0, 1}: sums the bf16 format holds exactly (asserted) -> exact
        gi = int_grad(adj.m, k, seed=k + 2, top=1)
        ref = ref_backward(col, n, ref_arg, gi)
        mag = ref_backward(col, n, ref_arg, np.abs(gi))
        assert mag.max() <= 256
        (gx,) = torch.autograd.grad(out, xd, torch.from_numpy(gi).to(torch.bfloat16).to(DEV), retain_graph=True)
        assert gx.dtype == torch.bfloat16
        assert np.array_equal(gx.float().cpu().numpy().astype(np.float64), ref)
        # any gradients: fp32 sums in some fixed order (|v - ref| <= L u32 mag, L the column's entries), one bf16 rounding
        gr = torch.randn(adj.m, k, generator=gen).to(torch.bfloat16)
        ref = ref_backward(col, n, ref_arg, gr.float().numpy())
        mag = ref_backward(col, n, ref_arg, gr.float().abs().numpy())
        (gx,) = torch.autograd.grad(out, xd, gr.to(DEV))
        acc = lens_in[:, None] * 2.0 ** -24 * mag
        excess = np.abs(gx.float().cpu().numpy() - ref) - (BF16_EPS * (np.abs(ref) + acc) + acc + 1e-38)
        assert excess.max() <= 0, f"{name} k={k} {op}: bound exceeded by {excess.max():.3e}"


@pytest.mark.parametrize("k", [5, 8])                  # one element per lane, and 16-byte loads (8 bf16)
@pytest.mark.parametrize("name", ["boundaries_T", "hubs_T"])
def test_bf16_backward_over_hub_columns(name, k):
    """columns listed by thousands of entries: the chunk partials are summed in fp32 and rounded to bf16 ONCE, at the store"""
    rp, col, n = graph(name)
    adj = make_adj(name)
    gen = torch.Generator().manual_seed(k)
    xb = torch.randn(n, k, generator=gen).to(torch.bfloat16)
    xb[::2] = torch.from_numpy(level_features(n, k, seed=k))[::2].to(torch.bfloat16)
    lens_in = np.bincount(col, minlength=n)
    for op in ("max", "min"):
        xd = xb.to(DEV).requires_grad_(True)
        out, arg = gcn_amd.aggregate(adj, xd, op, return_arg=True)
        ref_out, ref_arg = ref_select(rp, col, xb.float().numpy(), op)
        assert np.array_equal(arg.cpu().numpy(), ref_arg)
        assert np.array_equal(bits(out), bits(torch.from_numpy(ref_out).to(torch.bfloat16)))
        # integer gradients: every fp32 sum is an exact integer (< 2^24, asserted) in any order, so the result is that
        # integer rounded to bf16 once, to nearest even — torch's conversion — bit for bit; equal to it where bf16 holds it
        gi = int_grad(adj.m, k, seed=k + 2, top=8)
        ref = ref_backward(col, n, ref_arg, gi)
        assert ref_backward(col, n, ref_arg, np.abs(gi)).max() < 2 ** 24 and np.abs(ref).max() > 256
        (gx,) = torch.autograd.grad(out, xd, torch.from_numpy(gi).to(torch.bfloat16).to(DEV), retain_graph=True)
        assert gx.dtype == torch.bfloat16
        assert np.array_equal(bits(gx), bits(torch.from_numpy(ref).to(torch.bfloat16))), f"{name} k={k} {op}"
        # any gradients: |fp32 sum - ref| <= L u32 mag (L the column's entries, any order), then one bf16 rounding; twice
        gr = torch.randn(adj.m, k, generator=gen).to(torch.bfloat16)
        ref = ref_backward(col, n, ref_arg, gr.float().numpy())
        mag = ref_backward(col, n, ref_arg, gr.float().abs().numpy())
        (gx,) = torch.autograd.grad(out, xd, gr.to(DEV), retain_graph=True)
        (gx2,) = torch.autograd.grad(out, xd, gr.to(DEV))
        assert np.array_equal(bits(gx), bits(gx2))
        acc = lens_in[:, None] * 2.0 ** -24 * mag
        excess = np.abs(gx.float().cpu().numpy() - ref) - (BF16_EPS * (np.abs(ref) + acc) + acc + 1e-38)
        assert excess.max() <= 0, f"{name} k={k} {op}: bound exceeded by {excess.max():.3e}"


# ---- 6. misaligned operands, through the C ABI -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("k", [5, 8, 64])
def test_operands_one_element_off_the_grid(k, dtype):
    rp, col, n = graph("rect")
    adj = make_adj("rect")
    m, code = adj.m, _lib.DTYPE_BF16 if dtype == torch.bfloat16 else _lib.DTYPE_F32
    lib = gcn_amd.load_library()
    agg = __import__("importlib").import_module("gcn_amd.aggregate")
    ws = agg._scratch(adj, k, torch.device(DEV))
    trp, trow, tperm = adj.tpattern()
    x = torch.from_numpy(level_features(n, k, seed=k)).to(dtype)
    g = torch.from_numpy(int_grad(m, k, seed=k + 1, top=1)).to(dtype)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(off):
        xv, xf = offset_view(x, off, dtype, DEV)
        gv, gf = offset_view(g, off, dtype, DEV)
        ov, of = offset_view((m, k), off, dtype, DEV)
        gxv, gxf = offset_view((n, k), off, dtype, DEV)
        av, af = offset_view((m, k), 0, torch.int32, DEV)
        res = []
        for op in (_lib.REDUCE_MAX, _lib.REDUCE_MIN):
            _lib.check(lib.gcn_aggregate_csr(p(adj.rowptr), p(adj.col), m, n, adj.nnz, p(xv), code, k, op, p(ov), p(av), p(ws),
                                             ws.numel(), st), "gcn_aggregate_csr")
            _lib.check(lib.gcn_aggregate_backward_csr(p(trp), p(trow), p(tperm), n, m, adj.nnz, p(gv), code, p(av), k, p(gxv),
                                                      p(ws), ws.numel(), st), "gcn_aggregate_backward_csr")
            torch.cuda.synchronize()
            for v, f in ((xv, xf), (gv, gf), (ov, of), (gxv, gxf), (av, af)):
                assert guards_intact(f, v), off
            res.append((ov.clone(), av.clone(), gxv.clone()))
        return res

    aligned, shifted = run(0), run(1)
    for (o0, a0, g0), (o1, a1, g1), op in zip(aligned, shifted, ("max", "min")):
        assert torch.equal(a0, a1) and np.array_equal(bits(o0), bits(o1)) and np.array_equal(bits(g0), bits(g1))
        ref_out, ref_arg = ref_select(rp, col, x.float().numpy(), op)
        assert np.array_equal(a1.cpu().numpy(), ref_arg) and np.array_equal(o1.float().cpu().numpy(), ref_out)
        assert np.array_equal(g1.float().cpu().numpy(), ref_backward(col, n, ref_arg, g.float().numpy()))


# ---- 7. sum and mean ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [33, 128])
@pytest.mark.parametrize("name", ["boundaries", "rect"])
def test_sum_and_mean_match_fp64(name, k):
    rp, col, n = graph(name)
    adj = make_adj(name)
    x = np.random.default_rng(k).standard_normal((n, k)).astype(np.float32)
    lens = np.diff(rp)
    for reduce in ("sum", "mean"):
        val = np.ones(len(col), np.float32) if reduce == "sum" else \
            np.repeat(np.float32(1.0) / np.maximum(lens, 1).astype(np.float32), lens)
        out = gcn_amd.aggregate(adj, torch.from_numpy(x).to(DEV), reduce)
        ref = oracle_spmm(rp, col, val, x).astype(np.float64)
        mag = oracle_spmm(rp, col, val, np.abs(x)).astype(np.float64)
        assert_elementwise(out.cpu().numpy(), ref, mag, rp, what=f"{name} k={k} {reduce}")
        assert (out[torch.from_numpy(lens == 0).to(DEV)] == 0).all()
    assert set(adj._agg_twins) == {"sum", "mean"}       # built once, kept on the adjacency
    twin = adj._agg_twins["mean"]
    gcn_amd.aggregate(adj, torch.from_numpy(x).to(DEV), "mean")
    assert adj._agg_twins["mean"] is twin


# ---- 8. autograd through aggregate and SAGEConv ------------------------------------------------------------------------------
def _padded(rp, col):
    """neighbour table [m, longest] (int64) and its mask: the dense form of the neighbourhoods"""
    lens = np.diff(rp)
    m, width = len(lens), int(lens.max())
    idx = np.zeros((m, width), np.int64)
    mask = np.arange(width)[None, :] < lens[:, None]
    idx[mask] = col
    return torch.from_numpy(idx), torch.from_numpy(mask)


def dense_aggregate(x, idx, mask, aggr):
    """fp64 torch on dense tensors; rows without entries give 0"""
    slab = x[idx]                                       # [m, longest, k]
    has = mask.any(1, keepdim=True)
    if aggr in ("max", "min"):
        fill = float("-inf") if aggr == "max" else float("inf")
        slab = slab.masked_fill(~mask[:, :, None], fill)
        red = slab.amax(1) if aggr == "max" else slab.amin(1)
        return torch.where(has, red, torch.zeros_like(red))
    s = (slab * mask[:, :, None]).sum(1)
    return s / mask.sum(1, keepdim=True).clamp(min=1) if aggr == "mean" else s


def dense_sage(x, idx, mask, wn, wr, b, aggr):
    out = dense_aggregate(x, idx, mask, aggr) @ wn
    if wr is not None:
        out = out + x @ wr
    return out + b if b is not None else out


def assert_terms(got, ref, mag, what):
    excess = np.abs(got.detach().double().cpu().numpy() - ref.detach().numpy()) - (1e-5 * mag.detach().numpy() + 1e-30)
    print(f"[aggregate] {what}: max |err| - bound = {excess.max():.3e}")
    assert excess.max() <= 0, (what, float(excess.max()))


@pytest.mark.parametrize("aggr", ["max", "min", "mean", "sum"])
@pytest.mark.parametrize("fin,fout", [(24, 8), (8, 24)])
def test_sage_conv_and_aggregate_match_dense_fp64(aggr, fin, fout):
    rp, col, n = graph("cora")
    adj = make_adj("cora")
    idx, mask = _padded(rp, col)
    torch.manual_seed(fin + len(aggr))
    layer = gcn_amd.SAGEConv(fin, fout, aggr=aggr).to(DEV)
    x = torch.randn(n, fin)
    gout = torch.randn(n, fout)
    xd = x.to(DEV).requires_grad_(True)
    # aggregate alone: selected values are exact, sums within the bound; the gradient is a sum of |g| terms
    h = gcn_amd.aggregate(adj, xd, aggr)
    x64 = x.double().requires_grad_(True)
    h64 = dense_aggregate(x64, idx, mask, aggr)
    gh = torch.randn(n, fin)
    (gx,) = torch.autograd.grad(h, xd, gh.to(DEV))
    (gx64,) = torch.autograd.grad(h64, x64, gh.double())
    ones = torch.ones(n, fin, dtype=torch.float64, requires_grad=True)
    if aggr in ("max", "min"):
        assert np.array_equal(h.detach().cpu().numpy().astype(np.float64), h64.detach().numpy())
        # |terms| of the gradient: the same selection applied to |g| (a selection is linear in g)
        (gmag,) = torch.autograd.grad(dense_aggregate(x64, idx, mask, aggr), x64, gh.double().abs())
    else:
        assert_terms(h, h64, dense_aggregate(x64.abs(), idx, mask, aggr), f"{aggr} forward")
        (gmag,) = torch.autograd.grad(dense_aggregate(ones, idx, mask, aggr), ones, gh.double().abs())
    assert_terms(gx, gx64, gmag, f"{aggr} grad x")
    # the layer: out and every gradient against the dense fp64 layer; |terms| from the same graph on absolute values
    out = layer(xd, adj)
    out.backward(gout.to(DEV))
    P = {k_: v.detach().cpu().double().requires_grad_(True) for k_, v in layer.named_parameters()}
    ref = dense_sage(x64, idx, mask, P["weight_neigh"], P["weight_root"], P["bias"], aggr)
    x64.grad = None
    ref.backward(gout.double())
    # magnitudes: the selection (or the averaging) is fixed, everything else is bilinear -> evaluate with absolute values
    hsel = dense_aggregate(x64, idx, mask, aggr).detach()
    habs = hsel.abs() if aggr in ("max", "min") else dense_aggregate(x64.detach().abs(), idx, mask, aggr)
    wn, wr, g64 = P["weight_neigh"].detach().abs(), P["weight_root"].detach().abs(), gout.double().abs()
    assert_terms(out, ref, habs @ wn + x64.detach().abs() @ wr + P["bias"].detach().abs(), f"{aggr} layer out")
    assert_terms(layer.weight_neigh.grad, P["weight_neigh"].grad, habs.t() @ g64, f"{aggr} grad weight_neigh")
    assert_terms(layer.weight_root.grad, P["weight_root"].grad, x64.detach().abs().t() @ g64, f"{aggr} grad weight_root")
    assert_terms(layer.bias.grad, P["bias"].grad, g64.sum(0), f"{aggr} grad bias")
    src = x64 if aggr in ("max", "min") else ones
    (through,) = torch.autograd.grad(dense_aggregate(src, idx, mask, aggr), src, g64 @ wn.t())
    assert_terms(xd.grad, x64.grad, through + g64 @ wr.t(), f"{aggr} layer grad x")


def test_two_layer_max_model_trains_like_the_dense_fp64_model():
    rp, col, n = graph("cora")
    adj = make_adj("cora")
    idx, mask = _padded(rp, col)
    torch.manual_seed(0)
    l1 = gcn_amd.SAGEConv(32, 16, aggr="max").to(DEV)
    l2 = gcn_amd.SAGEConv(16, 7, aggr="max").to(DEV)
    x = torch.randn(n, 32)
    y = torch.randint(0, 7, (n,))
    params = list(l1.parameters()) + list(l2.parameters())
    ref = [p.detach().cpu().double().requires_grad_(True) for p in params]
    opt, ropt = torch.optim.Adam(params, lr=0.01), torch.optim.Adam(ref, lr=0.01)
    xd, yd, x64 = x.to(DEV), y.to(DEV), x.double()
    losses, rlosses = [], []
    for _ in range(20):
        opt.zero_grad()
        loss = F.nll_loss(F.log_softmax(l2(F.relu(l1(xd, adj)), adj), dim=1), yd)
        loss.backward()
        opt.step()
        losses.append(loss.item())
        ropt.zero_grad()
        h = F.relu(dense_sage(x64, idx, mask, ref[0], ref[1], ref[2], "max"))
        rloss = F.nll_loss(F.log_softmax(dense_sage(h, idx, mask, ref[3], ref[4], ref[5], "max"), dim=1), y)
        rloss.backward()
        ropt.step()
        rlosses.append(rloss.item())
    rel = max(abs(a - b) / abs(b) for a, b in zip(losses, rlosses))
    print(f"[aggregate] 20 Adam steps: loss {rlosses[0]:.4f} -> {rlosses[-1]:.4f}, max relative deviation {rel:.2e}")
    assert rlosses[-1] < rlosses[0]
    assert rel <= 1e-4, rel


def test_sage_conv_under_bf16_autocast_aggregates_in_bf16(monkeypatch):
    import gcn_amd.layers as layers_mod
    adj = make_adj("cora")
    seen = []
    real = layers_mod.aggregate
    monkeypatch.setattr(layers_mod, "aggregate", lambda a, t, r: (seen.append(t.dtype), real(a, t, r))[1])
    torch.manual_seed(1)
    layer = gcn_amd.SAGEConv(16, 8, aggr="max").to(DEV)
    x = torch.randn(adj.n, 16, device=DEV, requires_grad=True)
    ref = layer(x, adj)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = layer(x, adj)
    out.float().sum().backward()
    assert seen == [torch.float32, torch.bfloat16]
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())
    # out = h Wn + x Wr + b with u = 2^-8: h = max of bf16(x) = bf16(max x) (rounding is monotone) and x, Wn, Wr each carry one
    # rounding (2u per product term), each product is rounded once (u) and their bf16 sum once more (u): 4u on the terms'
    # magnitudes, 5u with the second-order parts
    with torch.no_grad():
        h = gcn_amd.aggregate(adj, x.detach(), "max")
        mag = h.abs() @ layer.weight_neigh.abs() + x.abs() @ layer.weight_root.abs() + layer.bias.abs()
        excess = (out.float() - ref).abs() - 5 * BF16_EPS * mag
    assert float(excess.max()) <= 0, float(excess.max())
    assert float((out.float() - ref).abs().max()) > 0   # (it did run in bf16)


# ---- 9. capture -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", [("cora", 64), ("boundaries", 33), ("boundaries_T", 64)])   # (_T: hub columns)
def test_forward_backward_captures_and_replays_bit_for_bit(name, k):
    adj = make_adj(name)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(adj.n, k, generator=gen).to(DEV).requires_grad_(True)
    gout = torch.randn(adj.m, k, generator=gen).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # one eager call: the workspace, the transpose and its permutation exist
        gcn_amd.aggregate(adj, x, "max").backward(gout)
    torch.cuda.current_stream().wait_stream(side)
    x.grad = None
    graph_ = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph_):
        out, arg = gcn_amd.aggregate(adj, x, "max", return_arg=True)
        out.backward(gout)
    for _rep in range(2):
        with torch.no_grad():
            x.copy_(torch.randn(adj.n, k, generator=gen).to(DEV))
            gout.copy_(torch.randn(adj.m, k, generator=gen).to(DEV))
        graph_.replay()
        torch.cuda.synchronize()
        got = [out.clone(), arg.clone(), x.grad.clone()]
        xe = x.detach().clone().requires_grad_(True)
        oe, ae = gcn_amd.aggregate(adj, xe, "max", return_arg=True)
        oe.backward(gout)
        for a, b in zip(got, (oe, ae, xe.grad)):
            assert np.array_equal(bits(a), bits(b))


def test_a_wider_call_keeps_the_workspace_a_capture_may_hold():
    adj = make_adj("boundaries")
    x = torch.ones(adj.n, 64, device=DEV)
    gcn_amd.aggregate(adj, x[:, :4].contiguous(), "max")
    keeper = adj._scratch
    small = keeper.buffers["aggregate"]
    gcn_amd.aggregate(adj, x, "max")
    wide = keeper.buffers["aggregate"]
    assert wide is not small and wide.numel() > small.numel()
    assert any(w is small for w in keeper.retired)         # still allocated: a captured step would go on writing there
    gcn_amd.aggregate(adj, x[:, :4].contiguous(), "max")
    assert keeper.buffers["aggregate"] is wide and len(keeper.retired) == 1           # (never shrinks)


# ---- 10. errors -------------------------------------------------------------------------------------------------------------
def test_errors():
    adj = make_adj("cora")
    x = torch.ones(adj.n, 4, device=DEV)
    with pytest.raises(gcn_amd.GcnAmdError):
        gcn_amd.aggregate(adj, x.cpu(), "max")
    for dt in (torch.float64, torch.float16, torch.int32):
        with pytest.raises(gcn_amd.GcnAmdError):
            gcn_amd.aggregate(adj, x.to(dt), "max")
    for bad in (torch.ones(adj.n + 1, 4, device=DEV), torch.ones(adj.n, device=DEV), torch.ones(adj.n, 0, device=DEV)):
        with pytest.raises(ValueError):
            gcn_amd.aggregate(adj, bad, "min")
    with pytest.raises(ValueError):
        gcn_amd.aggregate(adj, x, "median")
    with pytest.raises(ValueError):
        gcn_amd.aggregate(adj, x, "mean", return_arg=True)
    with pytest.raises(TypeError):
        gcn_amd.aggregate(torch.eye(4, device=DEV).to_sparse(), torch.ones(4, 4, device=DEV))
    with pytest.raises(ValueError):
        gcn_amd.SAGEConv(4, 4).to(DEV)(torch.ones(adj.n + 1, 4, device=DEV), adj)
