"""Non-finite feature values on every SpMM route, against the class twin of tests/nonfinite_ref.py.

Every case runs ONE plan twice — on B_clean (finite integers) and on B_poison (the same with about a dozen single elements
replaced by NaN, +Inf, -Inf and a signalling NaN: nonfinite_ref.poison says where and why) — into outputs that start as the
NaN sentinel of util.SENTINEL, and asserts (nonfinite_ref.assert_contained):
  * an element no poisoned B[c, j] reaches through a stored entry has the same BITS in both results (runs are deterministic, so
    there is no tolerance): nothing leaks through a padding lane, a marker, a masked product, a dense tile's zeros, the scaled
    copy, the slice reduction, the fix-up or a bf16 conversion;
  * a touched element has the class the twin counts — NaN, +Inf, -Inf, or exactly 0 where a ReLU met -Inf or the mask dropped
    it; a fused ReLU keeps NaN, as torch.relu does;
  * the clean result is finite everywhere and the poisoned one holds no sentinel: both were written in full; empty rows are
    0, or dropout(act(bias)).
The plans are those of tests/exact_plans.py (shared with tests/test_exact_gpu.py), and every case asserts the kernel name it
claims to run.  tests/test_nonfinite_cpu.py proves the twin, that these assertions refuse three modelled defects, and that the
inputs of every case here meet the preconditions.  Every case prints one `ran:` line (route, kernel, width, dtypes, epilogue)."""
import numpy as np
import pytest
import torch

import gcn_amd
import nonfinite_ref as nr
from exact_plans import (DEV, EPI_CASES, GROUP_WIDTHS, UNSLICED, UNSLICED_NAMES, _adj, _assert_group_kernel, _epilogue_plan, _group_adj,
                         _special_adj, _t, _unsliced_adj, epilogue_slices, smallest_epilogue_cases)
from gcn_amd import dropin
from gcn_amd.layers import GraphConvolution
from util import EPILOGUE_DROPOUT, EPILOGUES, SENTINEL, epilogue_reference, int_features, random_csr

pytestmark = pytest.mark.gpu
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


def _sentinel_out(m, k, dtype=torch.float32):
    out = torch.empty((m, k), dtype=dtype, device=DEV)
    out.view(_INT[dtype]).fill_(SENTINEL[out.element_size()])
    return out


def _host(C):
    """(values as fp32, bits) of a result"""
    C = C.detach()
    bits = C.contiguous().view(_INT[C.dtype]).cpu().numpy()
    return C.float().cpu().numpy(), bits


def _sentinel_of(bits):
    return SENTINEL[bits.dtype.itemsize]


def _ran(route, kernel, k, b_dtype, c_dtype, epilogue="none"):
    short = {torch.float32: "fp32", torch.bfloat16: "bf16"}
    print(f"ran: {route} | {kernel} | k={k} | B {short[b_dtype]} C {short[c_dtype]} | {epilogue}")


def _epi_name(e):
    return "+".join(x for x in ("bias", "relu", "dropout") if e.get(x)) or "none"


def _check_pair(run, d, what, cls=None, c_dtype=torch.float32, b_dtype=torch.float32, empty_want=None):
    """run(B on the device, out) on the clean and on the poisoned features; the module's assertions"""
    ops, k = d["ops"], d["B"].shape[1]
    res = []
    for B in (d["B"], d["Bp"]):
        out = _sentinel_out(ops["m"], k, c_dtype)
        got = run(_t(B, b_dtype if b_dtype != torch.float32 else None), out)
        assert got.data_ptr() == out.data_ptr() and got.dtype == c_dtype
        res.append(_host(got))
    (Cp, bp), (Cc, bc) = res[1], res[0]
    nr.assert_contained(Cp, Cc, d["cls"] if cls is None else cls, d["touched"], what, bits=(bp, bc), sentinel=_sentinel_of(bp))
    empty = np.diff(ops["rp"]) == 0
    if empty.any():
        want = np.zeros((int(empty.sum()), k), np.float32) if empty_want is None else empty_want[empty]
        assert np.array_equal(Cc[empty], want) and np.array_equal(Cp[empty], want), what
    return Cp


def _plain(adj, **kw):
    return lambda B, out: adj.matmul_raw(B, out=out, **kw)


# ---------------------------------------------------------------------------------------------------------------
# every route, no epilogue
@pytest.mark.parametrize("family,k,gather", UNSLICED, ids=[f"{f}-k{k}" for f, k, _g in UNSLICED])
def test_unsliced_families(family, k, gather):
    """narrow4 / 8 / 16_dpp, quad4 / 16, chunk1 / 2 / 4: ragged last blocks whose lanes gather row 0, the hub row's pieces in
    the partial slab, the masked-on-the-product branch of the quad kernel, the padded tail of odd k"""
    adj, ops = _unsliced_adj(family, gather, "int")
    name = adj.main_kernel(k)
    assert UNSLICED_NAMES[family] in name, name
    _check_pair(_plain(adj), nr.nonfinite_inputs("unsliced", "int", k, 0), (family, k, name))
    _ran(f"unsliced {family}", name, k, torch.float32, torch.float32)


@pytest.mark.parametrize("weighted", [False, True], ids=["value_free", "weighted"])
@pytest.mark.parametrize("k", GROUP_WIDTHS)
def test_group_kernels(k, weighted):
    """slices=3: the zero row behind every slice that padding entries gather, the scaled copy u_col * B (value-free), the
    slice reduction with its cut pieces; the first and the last row of every slice are poisoned"""
    kind = "int" if weighted else "pow2"
    adj, ops = _group_adj("group_dup", kind)
    name = _assert_group_kernel(adj, k, weighted)
    _check_pair(_plain(adj), nr.nonfinite_inputs("group_dup", kind, k, 3), (k, kind, name))
    _ran(f"group S=3 {'weighted' if weighted else 'value-free, factors handed over'}", name, k, torch.float32, torch.float32)


@pytest.mark.parametrize("k", [16, 41, 128])
def test_group_value_factors_found_by_the_plan(k):
    """a stored diagonal in every row, single-entry rows: one of them references a poisoned column"""
    adj, ops = _group_adj("group_diag_dup", "pow2", hand_over=False)
    assert adj.has_value_factors
    name = _assert_group_kernel(adj, k, weighted=False)
    d = nr.nonfinite_inputs("group_diag_dup", "pow2", k, 3)
    assert d["report"]["rows"]["single_entry"]
    _check_pair(_plain(adj), d, ("group_diag_dup", k, name))
    _ran("group S=3 value-free, factors found by the plan", name, k, torch.float32, torch.float32)


@pytest.mark.parametrize("kind", ["pow2", "int"], ids=["value_free", "weighted"])
@pytest.mark.parametrize("k", [16, 64, 128])
def test_nine_slices(k, kind):
    """the wide reduction's unrolled group of eight slices and its tail of one; eighteen slice edges poisoned"""
    adj, ops = _group_adj("group_dup", kind, slices=9)
    name = _assert_group_kernel(adj, k, kind == "int")
    _check_pair(_plain(adj), nr.nonfinite_inputs("group_dup", kind, k, 9), (k, kind, name))
    _ran(f"group S=9 {'weighted' if kind == 'int' else 'value-free'}", name, k, torch.float32, torch.float32)


def _special_name(adj, pattern, k, d):
    name = adj.main_kernel(k)
    if pattern == "vcsr":
        assert name.startswith("gcn::spmm_quad_kernel<16, false, false,"), name
    elif pattern == "col16":
        assert name == "gcn::spmm_quad_kernel<16, false, true, true>", name
    else:
        assert name == "gcn::spmm_panel_in_kernel", name
        assert adj.dense_panels == d["dense"], (adj.dense_panels, d["dense"])       # the twin's windows are the plan's
        if pattern == "mfma":
            name += " + spmm_panel_dense_mfma_kernel"
    return name


_SPECIAL = [("vcsr", "int", 64, 4), ("col16", "pow2", 64, 2), ("lds", "int", 64, 0), ("lds", "int", 100, 0), ("lds_all", "int", 64, 0),
            ("lds_all", "int", 100, 0), ("mfma", "int", 36, 0), ("mfma", "int", 64, 0), ("mfma", "int", 128, 0)]


@pytest.mark.parametrize("pattern,kind,k,slices", _SPECIAL, ids=[f"{p}-k{k}" for p, _kd, k, _s in _SPECIAL])
def test_sliced_quad_routes_and_panels(pattern, kind, k, slices):
    """vcsr: the sliced virtual CSR with values; col16: the 0xFFFF markers of the 16-bit column stream and the scaled copy;
    lds / lds_all: windows staged in LDS (+ the accumulate pass); mfma: the dense tiles' non-finite scan and their entry-by-entry
    pass — a poisoned column in the middle of a dense window, one reached from outside a window.  A dense tile holds the SUM of
    the repeated entries of one (row, column), and the twin counts over the merged entries there (nonfinite_ref.in_dense_tile)."""
    adj, ops = _special_adj(pattern)
    d = nr.nonfinite_inputs(pattern, kind, k, slices)
    name = _special_name(adj, pattern, k, d)
    _check_pair(_plain(adj), d, (pattern, k, name))
    _ran(pattern, name, k, torch.float32, torch.float32)


# ---------------------------------------------------------------------------------------------------------------
# bf16
@pytest.mark.parametrize("kind", ["pow2", "int"], ids=["value_free", "weighted"])
@pytest.mark.parametrize("k", [64, 72, 100, 128])
def test_bf16_group_plans(k, kind):
    """bf16 B into an fp32 and into a bf16 result: the bf16 table (bits copied, or bf16(u_col * b) rounded once), the bf16 walk
    and the one rounding of the bf16 store; k = 100 is no multiple of 8 and takes the upcast route through the fp32 kernels"""
    adj, ops = _group_adj("group_dup", kind)
    d = nr.nonfinite_inputs("group_dup", kind, k, 3)
    for c_dtype in (torch.float32, torch.bfloat16):
        _check_pair(_plain(adj), d, (k, kind, c_dtype), c_dtype=c_dtype, b_dtype=torch.bfloat16)
        name = adj.main_kernel(k, dtype=torch.bfloat16)           # (after the call: k = 64 builds its slice set at first use)
        assert name.startswith("gcn::spmm_group"), name
        hot = name.startswith("gcn::spmm_group_bf16_weighted_kernel<" if kind == "int" else "gcn::spmm_group_bf16_kernel<")
        assert hot == (k % 8 == 0), (k, name)
        _ran(f"group S=3 bf16 {'hot path' if hot else 'upcast'}", name, k, torch.bfloat16, c_dtype)


def test_bf16_unsliced_family():
    """an unsliced plan widens, runs the fp32 entry and narrows"""
    adj, ops = _unsliced_adj("quad16", 4, "int")
    k = 64
    name = adj.main_kernel(k, dtype=torch.bfloat16)
    assert not name.startswith("gcn::spmm_group_bf16") and UNSLICED_NAMES["quad16"] in name, name
    d = nr.nonfinite_inputs("unsliced", "int", k, 0)
    for c_dtype in (torch.float32, torch.bfloat16):
        _check_pair(_plain(adj), d, ("bf16 unsliced", c_dtype), c_dtype=c_dtype, b_dtype=torch.bfloat16)
        _ran("unsliced quad16 bf16 upcast", name, k, torch.bfloat16, c_dtype)


# ---------------------------------------------------------------------------------------------------------------
# the fused epilogue on every route that carries it, at the smallest width of each family (and beyond 256 columns, where the
# reduction is another kernel)
_EPI_IDS = [c[0] for c in smallest_epilogue_cases()]
_EPI_BY_ID = {c[0]: c for c in EPI_CASES}


@pytest.mark.parametrize("cid", _EPI_IDS)
def test_epilogue_classes(cid):
    """all five util.EPILOGUES with the bias and the mask of util.epilogue_inputs: a finite bias changes no class, a ReLU maps
    -Inf to 0 and KEEPS NaN, a dropped element is exactly 0; the bf16 cases into a bf16 result too"""
    _cid, carrier, pattern, kind, k, opt = _EPI_BY_ID[cid]
    adj, ops = _epilogue_plan(carrier, pattern, kind, k, opt)
    d = nr.nonfinite_inputs(pattern, kind, k, epilogue_slices(pattern, opt))
    bf16 = carrier.startswith("bf16")
    bias, keep = d["bias"], nr.keep_mask(ops["m"], k)
    bias_d = _t(bias)
    if opt.get("bias_off"):                                  # one float off the 16-byte grid: slice_reduce_kernel<1>
        flat = torch.zeros(k + 8, device=DEV)
        bias_d = flat[opt["bias_off"]:opt["bias_off"] + k].copy_(_t(bias))
        assert bias_d.data_ptr() % 16 == 4 * opt["bias_off"]
    p, seed, offset = EPILOGUE_DROPOUT
    name = adj.main_kernel(k, True, dtype=torch.bfloat16 if bf16 else torch.float32)
    for e in EPILOGUES:
        b, r, kp = (bias if e.get("bias") else None), bool(e.get("relu")), (keep if e.get("dropout") else None)
        cls = nr.apply_epilogue(d["cls"], b, r, kp)
        empty_want = epilogue_reference(np.zeros((ops["m"], k)), b, r, kp, 2.0).astype(np.float32)
        kw = dict(bias=bias_d if e.get("bias") else None, relu=r, dropout=(p, seed, offset) if e.get("dropout") else None)
        for c_dtype in ((torch.float32, torch.bfloat16) if bf16 else (torch.float32,)):
            Cp = _check_pair(_plain(adj, **kw), d, (cid, e, c_dtype), cls=cls, c_dtype=c_dtype,
                             b_dtype=torch.bfloat16 if bf16 else torch.float32, empty_want=empty_want)
            if r:
                assert np.isnan(Cp[d["touched"] & (cls == nr.NAN)]).all() and (d["touched"] & (cls == nr.NAN)).any()
            _ran(f"epilogue {cid}", name if not bf16 else adj.main_kernel(k, True, dtype=torch.bfloat16), k,
                 torch.bfloat16 if bf16 else torch.float32, c_dtype, _epi_name(e))


# ---------------------------------------------------------------------------------------------------------------
# transpose, backward, pre-laid, drop-in, heads
@pytest.mark.parametrize("pattern,kind,k,slices", nr.TRANSPOSED_CASES, ids=[c[0] for c in nr.TRANSPOSED_CASES])
def test_transposed_plan(pattern, kind, k, slices):
    """adj.transpose().matmul_raw: the device-built transpose keeps repeated entries apart, as the twin's does"""
    adj, ops = _unsliced_adj("quad16", 4, kind) if pattern == "unsliced" else _group_adj(pattern, kind)
    d = nr.nonfinite_inputs(pattern, kind, k, slices, transpose=True)
    at = adj.transpose()
    assert at is not adj and (at.m, at.n) == (ops["n"], ops["m"])
    name = at.main_kernel(k)
    assert name.startswith("gcn::spmm_"), name
    _check_pair(_plain(at), d, ("transpose", pattern, name))
    _ran(f"transpose of {pattern}", name, k, torch.float32, torch.float32)


def test_backward_with_a_poisoned_upstream_gradient():
    """gcn_amd.spmm(adj, X): X.grad = A^T . g has the twin's classes of the transposed matrix for a poisoned g, and the bits of
    the clean gradient everywhere else"""
    pattern, kind, k, slices = nr.TRANSPOSED_CASES[0]
    adj, ops = _unsliced_adj("quad16", 4, kind)
    d = nr.nonfinite_inputs(pattern, kind, k, slices, transpose=True)
    X = _t(int_features(ops["n"], k, seed=1))
    grads = []
    for G in (d["B"], d["Bp"]):
        x = X.clone().requires_grad_(True)
        gcn_amd.spmm(adj, x).backward(_t(G))
        grads.append(_host(x.grad))
    nr.assert_contained(grads[1][0], grads[0][0], d["cls"], d["touched"], "X.grad", bits=(grads[1][1], grads[0][1]))
    _ran("backward of spmm (transpose of unsliced)", adj.transpose().main_kernel(k), k, torch.float32, torch.float32)


def test_prelaid_table():
    """to_prelaid + matmul_prelaid on the value-free group plan: the caller's own B' (u_col * B in torch arithmetic)"""
    adj, ops = _group_adj("group", "pow2")
    k = 64
    name = _assert_group_kernel(adj, k, weighted=False)
    lay = adj.prelaid_layout(k)
    assert lay is not None and "status" not in lay and lay["slices"] == 3 and lay["ld"] == k
    d = nr.nonfinite_inputs("group", "pow2", k, 3)
    u = _t(ops["u_col"])
    _check_pair(lambda B, out: adj.matmul_prelaid(adj.to_prelaid(B, u), out), d, ("prelaid", name))
    _ran("pre-laid table, group S=3 value-free", name, k, torch.float32, torch.float32)


def test_dropin_pair():
    """csr2tile -> flexspmm in the group format (tests/stress_dropin.py, seed 20): group_fixup_kernel adds the head pieces of
    the rows that chunk ends cut, the hub row's poisoned ones among them"""
    d = nr.dropin_inputs()
    ops = d["ops"]
    m, n, nnz, k = ops["m"], ops["n"], len(ops["ci"]), nr.DROPIN_K
    out = dropin.csr2tile(torch.from_numpy(ops["rp"].copy()), torch.from_numpy(ops["ci"].copy()), torch.from_numpy(ops["va"].copy()),
                          m, n, nnz, torch.arange(n, dtype=torch.int32))
    seg_rowPtr, segNzCV, segVoMap, tail, nxt, n_segs = out
    hdr = seg_rowPtr.numpy()[:9]
    assert int(n_segs[0]) > 0 and hdr[0] == 0x47434E47 and hdr[6] == 0 and hdr[8] == nnz, hdr      # the group format, weighted
    dev = [t.to(DEV) for t in (seg_rowPtr, segNzCV, segVoMap, tail, nxt)]
    res = [_host(dropin.flexspmm.apply(dev[0], dev[1], dev[2], m, n, int(n_segs[0]), dev[3], dev[4], _t(B))) for B in (d["B"], d["Bp"])]
    nr.assert_contained(res[1][0], res[0][0], d["cls"], d["touched"], "flexspmm", bits=(res[1][1], res[0][1]))
    assert np.all(res[0][0][np.diff(ops["rp"]) == 0] == 0) and np.all(res[1][0][np.diff(ops["rp"]) == 0] == 0)
    _ran("drop-in csr2tile -> flexspmm, group format S=2 weighted", "spmm_group_weighted_kernel + group_fixup_kernel", k,
         torch.float32, torch.float32)


def test_heads():
    """spmm_heads, H = 4: one poisoned (B row, head, column); every other head and column keeps its bits"""
    h = nr.heads_inputs()
    ops = h["ops"]
    adj = _adj(ops, symmetric=False)
    vals = _t(h["values"])
    res = [_host(gcn_amd.spmm_heads(adj, _t(X), vals)) for X in (h["X"], h["Xp"])]
    nr.assert_contained(res[1][0], res[0][0], h["cls"], h["touched"], "spmm_heads", bits=(res[1][1], res[0][1]))
    j = h["at"][1]
    other = np.ones(res[0][0].shape[1], bool)
    other[j] = False
    assert np.array_equal(res[1][1][:, other], res[0][1][:, other])
    _ran("spmm_heads H=4", "spmm_heads_kernel", nr.HEADS * nr.HEAD_F, torch.float32, torch.float32)


# ---------------------------------------------------------------------------------------------------------------
# the layer: the fused epilogue stands for bias + F.relu
def test_fused_layer_matches_the_unfused_one_on_non_finite_input():
    """GraphConvolution(fuse_epilogue=True) against fuse_epilogue=False on a 600-vertex graph with a NaN and a -Inf in the
    input: the classes of the output, of weight.grad and of the input gradient agree element for element, and so do the finite
    values (powers of two in A, small integers everywhere else: every sum is exact in either path)"""
    m = n = 600
    rowptr, col, val = random_csr(m, n, 6003, seed=11)
    val = (2.0 ** -np.random.default_rng(1).integers(0, 3, len(col))).astype(np.float32)
    adj = gcn_amd.CsrAdjacency(_t(rowptr), _t(col), _t(val), (m, n), symmetric=False)
    torch.manual_seed(0)
    layer = GraphConvolution(24, 16).to(DEV)
    with torch.no_grad():
        layer.weight.copy_(torch.randint(-2, 3, layer.weight.shape, device=DEV).float())
        layer.bias.copy_(torch.randint(-2, 3, layer.bias.shape, device=DEV).float())
    X = np.random.default_rng(2).integers(-3, 4, (n, 24)).astype(np.float32)
    X[17, 5], X[311, 20] = np.nan, -np.inf
    G = _t(np.random.default_rng(3).integers(1, 4, (m, 16)).astype(np.float32))
    got = {}
    for fused in (True, False):
        x = _t(X).requires_grad_(True)
        layer.zero_grad()
        out = layer(x, adj, relu=True, fuse_epilogue=fused)
        out.backward(G)
        got[fused] = [t.detach().cpu().numpy().copy() for t in (out, layer.weight.grad, x.grad)]
    for what, f, u in zip(("output", "weight.grad", "input gradient"), got[True], got[False]):
        a, b = nr.class_of(f), nr.class_of(u)
        a, b = np.where(a == nr.ZERO, nr.FINITE, a), np.where(b == nr.ZERO, nr.FINITE, b)
        if not np.array_equal(a, b):
            i = tuple(np.argwhere(a != b)[0])
            raise AssertionError(f"{what}: {int((a != b).sum())} elements differ in class between the fused and the unfused layer, "
                                 f"first at {i}: fused {f[i]!r}, unfused {u[i]!r}")
        fin = a == nr.FINITE
        assert np.array_equal(f[fin], u[fin]), f"{what}: {int((f[fin] != u[fin]).sum())} finite elements differ, fused against unfused"
    assert np.isnan(got[False][0]).any() and np.isnan(got[False][1]).any()        # the unfused layer reports the NaN
    _ran("GraphConvolution fused vs unfused", adj.main_kernel(16, True), 16, torch.float32, torch.float32, "bias+relu")
