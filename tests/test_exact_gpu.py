"""Exact-arithmetic and element-wise checks of the fp32 / bf16 SpMM on the GPU, through every kernel family.

The rest of the suite compares with max|C - C*| / max|C*| <= 1e-5 on unit-scale data: one number for the whole matrix,
an element is only tested against the LARGEST entry of C (tests/test_exact_cpu.py holds the demonstration).  Two legs:

Leg 1, no tolerance.  Operands whose every fp32 partial sum is exact in any order and any grouping: integer features in
[-8, 8]; non-zero integer values in [-4, 4] (they do not factor), or u[r]*u[c] with u = 2^-e, e in {0..3} (value-free
plans: u_col*B and the u_row scaling are power-of-two scalings, and the bf16 table holds them in 8 bits).  Every test
asserts the precondition on its own inputs (util.assert_exact_inputs: max |A|.|B| * 2^6 < 2^24, rows < 32768 entries) and
then VALUE EQUALITY with the fp64 oracle on every element; empty rows equal 0, or act(bias).

Leg 2, element-wise.  Features standard_normal * 2^(p_c + q_j), values N(0, 0.5) * 2^s_r or factors (0.5 + rand) * 2^a
(exponents +-12 / +-10: everything stays in the normal fp32 range; subnormals are out of scope), and for every element
    |C - C*|_ij <= 1.01 * (L_i + 16) * 2^-24 * mag_ij + 1e-37,      mag = oracle(|A|, |B|)  (+ |bias|, see below)
L_i the stored length of row i.  The 16 is derived, not measured (u = 2^-24): the value-factor check admits 4.8e-7
relative per term (8u), the roundings of u_col*b and of the u_row scaling (1u each), the bias add (1u), the oracle's own
rounding of C* to fp32 (1u), and L_i - 1 additions in any order (<= L_i u; adding a stored, padded or tile zero is exact) —
L_i + 12, rounded up; 1.01 covers the second-order terms.  With a bias, mag_ij is |A|.|B| + |bias_j|: the bias is one
more term of the row ([A 1].[B; bias]) and its addition rounds relative to a sum that holds it — without that term no
correct kernel could meet the bound where |bias| exceeds |A|.|B|.  The bf16 cases keep util.bf16_assert_bound.

Every case holds empty rows and a hub row (util.exact_pattern; the two cases whose value factors the plan or csr2tile
must find by itself need a stored diagonal in every row and have single-entry rows in place of the empty ones; lds_all, whose
entries all lie inside their panels' windows, has empty rows and no hub row), and asserts the kernel name it claims to run.
test_exact_epilogue runs leg 1 with the fused epilogue on every route and every piece of code that carries it.  The recipes that force a family are those of tests/test_contract_gpu.py;
the plans and the epilogue case list live in tests/exact_plans.py, which tests/test_nonfinite_gpu.py shares."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gcn_amd
from gcn_amd import _lib, dropin
from exact_plans import (DEV, EPI_CASES, GROUP_WIDTHS, UNSLICED, UNSLICED_NAMES, _adj, _assert_group_kernel, _epilogue_plan, _group_adj,
                         _special_adj, _t, _unsliced_adj)
from util import (EPILOGUE_DROPOUT, EPILOGUES, assert_elementwise, assert_exact, assert_exact_inputs, bf16_assert_bound, bf16_reference,
                  epilogue_inputs, epilogue_reference, exact_operands, guards_intact, int_features, offset_view, oracle_spmm,
                  spmm_references, wide_features)

pytestmark = pytest.mark.gpu


def _exact(adj, ops, k, what):
    """leg 1 on one plan and width: precondition, value equality on every element (C starts as NaN), empty rows zero"""
    B = int_features(ops["n"], k, seed=1000 + k)
    assert_exact_inputs(ops["rp"], ops["ci"], ops["va"], B)
    Cref = oracle_spmm(ops["rp"], ops["ci"], ops["va"], B)
    out = torch.full((ops["m"], k), float("nan"), device=DEV)        # whatever was there must be overwritten
    C = adj.matmul_raw(_t(B), out=out).cpu().numpy()
    assert_exact(C, Cref, what)
    assert np.all(C[np.diff(ops["rp"]) == 0] == 0.0), what
    return B, Cref


def _elementwise(adj, ops, k, what, epilogue=True):
    """leg 2 on one plan and width, without and with the bias + ReLU epilogue -> the larger ratio to the bound"""
    rng = np.random.default_rng(2000 + k)
    B = wide_features(ops["n"], k, seed=2000 + k)
    Cref, mag = spmm_references(ops["rp"], ops["ci"], ops["va"], B)
    C = adj.matmul_raw(_t(B)).cpu().numpy()
    ratio = assert_elementwise(C, Cref, mag, ops["rp"], f"{what} k={k}")
    empty = np.diff(ops["rp"]) == 0
    assert np.all(C[empty] == 0.0), what
    if epilogue:
        bias = (rng.standard_normal(k) * 2.0 ** rng.integers(-12, 13, k)).astype(np.float32)
        Eref, emag = spmm_references(ops["rp"], ops["ci"], ops["va"], B, bias=bias, relu=True)
        Ce = adj.matmul_raw(_t(B), bias=_t(bias), relu=True).cpu().numpy()
        ratio = max(ratio, assert_elementwise(Ce, Eref, emag, ops["rp"], f"{what} k={k} bias+relu"))
        assert np.all(Ce[empty] == np.maximum(bias, 0)[None, :]), what
    return ratio


# ---------------------------------------------------------------------------------------------------------------
# leg 1: exact arithmetic
@pytest.mark.parametrize("family,k,gather", UNSLICED, ids=[f"{f}-k{k}" for f, k, _g in UNSLICED])
def test_exact_unsliced_families(family, k, gather):
    """spmm_narrow_kernel / spmm_narrow16_dpp_kernel / spmm_quad_kernel<4|16> / spmm_chunk_kernel<1|2|4> on a 2500 x 3000
    matrix: 10 % empty rows, a 2000-entry row across 15 chunks, duplicate entries; integer values"""
    adj, ops = _unsliced_adj(family, gather, "int")
    name = adj.main_kernel(k)
    assert UNSLICED_NAMES[family] in name, name
    _exact(adj, ops, k, (family, k, name))


@pytest.mark.parametrize("dup", [False, True], ids=["plain", "duplicates"])
@pytest.mark.parametrize("weighted", [False, True], ids=["value_free", "weighted"])
@pytest.mark.parametrize("k", GROUP_WIDTHS)
def test_exact_group_kernels(k, weighted, dup):
    """the 8-, 12- and 16-lane engines of spmm_group.hip, value-free (factors handed over) and weighted, slice reduction
    with its cut lists; 41 and 100 on the padded copies"""
    adj, ops = _group_adj("group_dup" if dup else "group", "int" if weighted else "pow2")
    name = _assert_group_kernel(adj, k, weighted)
    _exact(adj, ops, k, (k, weighted, dup, name))


@pytest.mark.parametrize("pattern,kind", [("group_diag", "pow2"), ("group", "pow2_row")], ids=["stored_diagonal", "row_constant"])
def test_exact_value_factors_found_by_the_plan(pattern, kind):
    """no hand-over: enable_slicing finds u = sqrt(A[r, r]) from the stored diagonal u^2 (every row holds one: this case
    has single-entry rows, not empty ones), or the row-constant values 2^-e_r, and runs value-free"""
    adj, ops = _group_adj(pattern, kind, hand_over=False)
    assert adj.has_value_factors
    for k in (16, 41, 128):
        name = _assert_group_kernel(adj, k, weighted=False)
        _exact(adj, ops, k, (pattern, kind, k, name))


def test_exact_sliced_virtual_csr_with_values():
    """slices of 35 000 columns cannot use the 15-bit stream: the four-per-gather kernel on the slice-major virtual CSR"""
    adj, ops = _special_adj("vcsr")
    name = adj.main_kernel(64)
    assert adj.num_slices == 4 and not adj.has_value_factors
    assert name.startswith("gcn::spmm_quad_kernel<16,"), name
    _exact(adj, ops, 64, name)


def test_exact_sliced_virtual_csr_value_free_on_the_16_bit_column_stream():
    """... and value-free (build_col16_stream): 20 000 x 70 000, two slices, 49 entries per column so the scaled copy pays"""
    adj, ops = _special_adj("col16")
    assert adj.num_slices == 2 and adj.has_value_factors
    assert adj.main_kernel(64) == "gcn::spmm_quad_kernel<16, false, true, true>", adj.main_kernel(64)
    _exact(adj, ops, 64, "col16")


def test_exact_lds_panels():
    """spmm_panel_in_quad_kernel (window entries staged in LDS) and the accumulate pass over the rest"""
    adj, ops = _special_adj("lds")
    assert adj.panel_rows > 0 and adj.dense_panels == 0
    for k in (64, 100):
        assert adj.main_kernel(k) == "gcn::spmm_panel_in_kernel"
        _exact(adj, ops, k, ("lds", k))


@pytest.mark.parametrize("k", [36, 64, 128])
def test_exact_dense_mfma_panels(k):
    """spmm_panel_dense_mfma_kernel: duplicates ADD in the tile, the tile's zeros add exactly"""
    adj, ops = _special_adj("mfma")
    assert adj.dense_panels >= 10 and adj.main_kernel(k) == "gcn::spmm_panel_in_kernel"
    _exact(adj, ops, k, ("mfma", k))


# ---------------------------------------------------------------------------------------------------------------
# leg 1, the fused epilogue: every route x every piece of code that carries it
_EPI_INPUTS = {}


def _epilogue_inputs(ops, pattern, kind, k):
    """(B, bias, keep, C* as fp32) of one (matrix, width), computed once: the 3- and 9-slice plans and the bf16 cases share it"""
    key = (pattern, kind, k)
    if key not in _EPI_INPUTS:
        B, bias, keep = epilogue_inputs(ops["m"], ops["n"], k)
        assert_exact_inputs(ops["rp"], ops["ci"], ops["va"], B, extra=bias, scale=2.0)
        _EPI_INPUTS[key] = (B, bias, keep, oracle_spmm(ops["rp"], ops["ci"], ops["va"], B))
    return _EPI_INPUTS[key]


@pytest.mark.parametrize("case", EPI_CASES, ids=[c[0] for c in EPI_CASES])
def test_exact_epilogue(case):
    """C = dropout(act(A.B + bias)) EQUALS util.epilogue_reference on every element, empty rows (dropout(act(bias))) included,
    for all five EPILOGUES on every route and every piece of code that carries the epilogue: integer bias in [-8, 8], p = 0.5
    (scale 2 exactly), offset 11, the mask of util.dropout_keep; C starts as NaN.  tests/test_exact_cpu.py proves on these very
    inputs that a result with one step missing or out of order is refused.  A bf16 result equals the reference converted once.
    An explicit slice count builds no narrow slice set, so the k <= 32 cases run on the plan's own slices (asserted).
    OFF32 = false in the wide reduction (a plane of partial rows of 4 GiB) runs in tests/test_large_operands_gpu.py, with and
    without this epilogue.  Out of scope: the pre-laid entry (it has no bias, ReLU or mask argument) and
    GCN_AMD_GROUP_FUSED_FIXUP=0 (read once per process)."""
    cid, carrier, pattern, kind, k, opt = case
    adj, ops = _epilogue_plan(carrier, pattern, kind, k, opt)
    m = ops["m"]
    B, bias, keep, Cref = _epilogue_inputs(ops, pattern, kind, k)
    bf16 = carrier.startswith("bf16")
    Bd = _t(B, torch.bfloat16 if bf16 else None)
    if bf16:
        assert torch.equal(Bd.float(), _t(B))
    bias_d, flat = offset_view(bias, opt["bias_off"], torch.float32, DEV) if opt.get("bias_off") else (_t(bias), None)
    assert bias_d.data_ptr() % 16 == 4 * opt.get("bias_off", 0)
    p, seed, offset = EPILOGUE_DROPOUT
    empty = np.diff(ops["rp"]) == 0
    assert empty.sum() >= 2
    for e in EPILOGUES:
        ref64 = epilogue_reference(Cref, bias if e.get("bias") else None, bool(e.get("relu")), keep if e.get("dropout") else None, 2.0)
        ref = ref64.astype(np.float32)
        assert np.array_equal(ref.astype(np.float64), ref64)      # an fp32 number: a bf16 result is rounded once, from it
        kw = dict(bias=bias_d if e.get("bias") else None, relu=bool(e.get("relu")), dropout=(p, seed, offset) if e.get("dropout") else None)
        C = adj.matmul_raw(Bd, out=torch.full((m, k), float("nan"), device=DEV), **kw).cpu().numpy()
        assert_exact(C, ref, (cid, e))
        want = np.broadcast_to(epilogue_reference(np.zeros((1, k)), bias if e.get("bias") else None, bool(e.get("relu")), None, 2.0), (m, k))
        want = np.where(keep, 2.0 * want, 0.0) if e.get("dropout") else want
        assert np.array_equal(C[empty], want[empty].astype(np.float32)), (cid, e)
        if bf16:
            C16 = adj.matmul_raw(Bd, out=torch.full((m, k), float("nan"), device=DEV, dtype=torch.bfloat16), **kw)
            assert C16.dtype == torch.bfloat16
            assert_exact(C16.float().cpu().numpy(), torch.from_numpy(ref).to(torch.bfloat16).float().numpy(), (cid, e, "bf16 result"))
    if flat is not None:
        assert guards_intact(flat, bias_d), cid
    if carrier == "bf16":
        want = "gcn::spmm_group_bf16_weighted_kernel<" if kind == "int" else "gcn::spmm_group_bf16_kernel<"
        name = adj.main_kernel(k, True, dtype=torch.bfloat16)
        assert name.startswith(want), (cid, name)
    if pattern == "group_dup":
        assert adj.narrow_slices_for(k) == 0, cid                 # the plan's own slice set at every width


@pytest.mark.parametrize("weighted", [False, True], ids=["value_free", "weighted"])
def test_exact_bf16_hot_path(weighted):
    """spmm_group_bf16.hip: integers in [-8, 8] and their power-of-two scalings fit bf16's 8 bits, every sum is fp32: the
    fp32 result equals the oracle, the bf16 result is that value converted once"""
    adj, ops = _group_adj("group_dup", "int" if weighted else "pow2")
    want = "gcn::spmm_group_bf16_weighted_kernel<" if weighted else "gcn::spmm_group_bf16_kernel<"
    for k in (64, 128, 136):
        B = int_features(ops["n"], k, seed=4000 + k)
        B16 = _t(B, torch.bfloat16)
        assert torch.equal(B16.float(), _t(B))
        assert_exact_inputs(ops["rp"], ops["ci"], ops["va"], B)
        Cref = oracle_spmm(ops["rp"], ops["ci"], ops["va"], B)
        C32 = adj.matmul_raw(B16, out=torch.full((ops["m"], k), float("nan"), device=DEV))
        name = adj.main_kernel(k, dtype=torch.bfloat16)              # (after the call: k = 64 builds its slice set at first use)
        assert name.startswith(want), (k, name)
        assert_exact(C32.cpu().numpy(), Cref, (weighted, k, "fp32 result"))
        C16 = adj.matmul_raw(B16)
        assert C16.dtype == torch.bfloat16
        assert_exact(C16.float().cpu().numpy(), torch.from_numpy(Cref).to(torch.bfloat16).float().numpy(), (weighted, k, "bf16 result"))
        assert bool((C16[_t(np.diff(ops["rp"]) == 0)] == 0).all())


def test_exact_bf16_fallback_plan():
    """an unsliced plan widens, runs the fp32 entry and narrows"""
    adj, ops = _unsliced_adj("quad16", 4, "int")
    k = 64
    name = adj.main_kernel(k, dtype=torch.bfloat16)
    assert not name.startswith("gcn::spmm_group_bf16") and UNSLICED_NAMES["quad16"] in name, name
    B = int_features(ops["n"], k, seed=4500)
    assert_exact_inputs(ops["rp"], ops["ci"], ops["va"], B)
    Cref = oracle_spmm(ops["rp"], ops["ci"], ops["va"], B)
    B16 = _t(B, torch.bfloat16)
    assert_exact(adj.matmul_raw(B16, out=torch.empty((ops["m"], k), device=DEV)).cpu().numpy(), Cref, "fallback fp32 result")
    assert_exact(adj.matmul_raw(B16).float().cpu().numpy(), torch.from_numpy(Cref).to(torch.bfloat16).float().numpy(), "fallback bf16 result")


def test_exact_prelaid_two_layer_chain():
    """gcn_spmm_csr_f32_prelaid: layer 1 reads B' and writes layer 2's B' (out_gap = the slice width, out_scale = the
    power-of-two column factor), layer 2 reads it: both results equal the oracle's.  Features in [-2, 2] here: the second
    layer's sums are multiples of 2^-12 and must still fit 24 bits on the hub row (asserted)."""
    adj, ops = _group_adj("group", "pow2")
    k = 64
    _assert_group_kernel(adj, k, weighted=False)
    lay = adj.prelaid_layout(k)
    assert lay is not None and lay["slices"] == 3 and lay["ld"] == k
    w, m = lay["slice_cols"], ops["m"]
    u = _t(ops["u_col"])
    B = int_features(ops["n"], k, seed=5000, top=2)
    assert_exact_inputs(ops["rp"], ops["ci"], ops["va"], B)
    ref1 = oracle_spmm(ops["rp"], ops["ci"], ops["va"], B)
    assert_exact_inputs(ops["rp"], ops["ci"], ops["va"], ref1)
    ref2 = oracle_spmm(ops["rp"], ops["ci"], ops["va"], ref1)
    Bp = adj.to_prelaid(_t(B), u)
    C1 = adj.matmul_prelaid(Bp, torch.full((m, k), 5.0, device=DEV))
    assert_exact(C1.cpu().numpy(), ref1, "plain result from a pre-laid input")
    Bp2 = torch.zeros_like(Bp)
    adj.matmul_prelaid(Bp, Bp2, out_scale=u, out_gap=w)
    assert w > 0 and float(Bp2[w::w + 1].abs().max()) == 0.0          # the zero row behind every slice
    r = torch.arange(m, device=DEV)
    assert_exact(Bp2[r + r // w].cpu().numpy(), ops["u_col"][:, None] * ref1, "layer 1 into layer 2's B'")
    C2 = adj.matmul_prelaid(Bp2, torch.full((m, k), 5.0, device=DEV))
    assert_exact(C2.cpu().numpy(), ref2, "layer 2")
    assert np.all(C2.cpu().numpy()[np.diff(ops["rp"]) == 0] == 0.0)


@pytest.mark.parametrize("pattern,kind,k", [("unsliced", "int", 64), ("unsliced", "int", 41), ("group", "int", 128)])
def test_exact_oneshot(pattern, kind, k):
    """gcn_spmm_csr_f32_oneshot (the body of cuspmm): the schedule rebuilt on the device at every call"""
    ops = exact_operands(pattern, kind)
    B = int_features(ops["n"], k, seed=6000 + k)
    assert_exact_inputs(ops["rp"], ops["ci"], ops["va"], B)
    rp, ci, va, Bd = _t(ops["rp"]), _t(ops["ci"]), _t(ops["va"]), _t(B)
    C = torch.full((ops["m"], k), float("nan"), device=DEV)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    st = _lib.load().gcn_spmm_csr_f32_oneshot(vp(rp), vp(ci), vp(va), vp(Bd), vp(C), ops["m"], ops["n"], len(ops["ci"]), k,
                                              ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    _lib.check(st, "gcn_spmm_csr_f32_oneshot")
    torch.cuda.synchronize()
    C = C.cpu().numpy()
    assert_exact(C, oracle_spmm(ops["rp"], ops["ci"], ops["va"], B), (pattern, k))
    assert np.all(C[np.diff(ops["rp"]) == 0] == 0.0)


@pytest.mark.parametrize("pattern,kind", [("dropin_csr", "int"), ("dropin_group", "int"), ("dropin_group_diag", "pow2")],
                         ids=["csr", "group_weighted", "group_value_free"])
def test_exact_dropin_pair(pattern, kind):
    """csr2tile -> flexspmm: the plain-CSR packing, and the group packing weighted and value-free (csr2tile finds the
    factors itself from the stored diagonal)"""
    ops = exact_operands(pattern, kind)
    m, n, nnz = ops["m"], ops["n"], len(ops["ci"])
    out = dropin.csr2tile(torch.from_numpy(ops["rp"].copy()), torch.from_numpy(ops["ci"].copy()), torch.from_numpy(ops["va"].copy()),
                          m, n, nnz, torch.arange(n, dtype=torch.int32))
    seg_rowPtr, segNzCV, segVoMap, tail, nxt, n_segs = out
    assert int(n_segs[0]) > 0
    hdr = seg_rowPtr.numpy()[:9]
    if pattern == "dropin_csr":
        assert hdr[0] != 0x47434E47
    else:                                                            # the group format's header; [6]: value-free
        assert hdr[0] == 0x47434E47 and hdr[6] == (1 if kind == "pow2" else 0) and hdr[8] == nnz, hdr
    dev = [t.to(DEV) for t in (seg_rowPtr, segNzCV, segVoMap, tail, nxt)]
    for k in (16, 41, 128):
        X = int_features(n, k, seed=7000 + k)
        assert_exact_inputs(ops["rp"], ops["ci"], ops["va"], X)
        C = dropin.flexspmm.apply(dev[0], dev[1], dev[2], m, n, int(n_segs[0]), dev[3], dev[4], _t(X)).cpu().numpy()
        assert_exact(C, oracle_spmm(ops["rp"], ops["ci"], ops["va"], X), (pattern, k))
        assert np.all(C[np.diff(ops["rp"]) == 0] == 0.0)


def test_exact_backward():
    """gcn_amd.spmm: B.grad = A^T . g exactly for an integer g (the transpose sums duplicate entries: still integers)"""
    ops = exact_operands("unsliced", "int")
    m, n, k = ops["m"], ops["n"], 64
    adj = _adj(ops, symmetric=False)
    B = _t(int_features(n, k, seed=8000)).requires_grad_(True)
    G = int_features(m, k, seed=8001)
    At = sp.csr_matrix((ops["va"].astype(np.float64), ops["ci"], ops["rp"]), shape=(m, n)).T.tocsr()
    At.sum_duplicates()
    At.sort_indices()
    trp, tci, tva = At.indptr.astype(np.int32), At.indices.astype(np.int32), At.data.astype(np.float32)
    assert_exact_inputs(trp, tci, tva, G)
    C = gcn_amd.spmm(adj, B)
    assert adj.transpose().main_kernel(k).startswith("gcn::spmm_"), adj.transpose().main_kernel(k)
    assert_exact(C.detach().cpu().numpy(), oracle_spmm(ops["rp"], ops["ci"], ops["va"], B.detach().cpu().numpy()), "forward")
    C.backward(_t(G))
    assert_exact(B.grad.cpu().numpy(), oracle_spmm(trp, tci, tva, G), "B.grad")


# ---------------------------------------------------------------------------------------------------------------
# leg 2: element-wise bound on wide-range operands
@pytest.mark.parametrize("family,k,gather", [c for c in UNSLICED if c[1] != 128 or c[0] == "chunk2"],
                         ids=[f"{f}-k{k}" for f, k, _g in UNSLICED if k != 128 or f == "chunk2"])
def test_elementwise_unsliced_families(family, k, gather):
    adj, ops = _unsliced_adj(family, gather, "wide")
    assert UNSLICED_NAMES[family] in adj.main_kernel(k), adj.main_kernel(k)
    _elementwise(adj, ops, k, f"unsliced {family}")


@pytest.mark.parametrize("weighted", [False, True], ids=["value_free", "weighted"])
@pytest.mark.parametrize("k", [16, 41, 128])
def test_elementwise_group_kernels(k, weighted):
    """value-free: u_col * b and the u_row scaling each round once; the stored value is the fp32 product u_row * u_col"""
    adj, ops = _group_adj("group" if weighted else "group_dup", "wide" if weighted else "wide_factored")
    _assert_group_kernel(adj, k, weighted)
    _elementwise(adj, ops, k, f"group {'weighted' if weighted else 'value-free'}")


def test_elementwise_sliced_virtual_csr():
    ops = exact_operands("vcsr", "wide")
    adj = _adj(ops, slices=4)
    adj.set_gather_width(4)
    assert adj.num_slices == 4 and adj.main_kernel(64).startswith("gcn::spmm_quad_kernel<16,"), adj.main_kernel(64)
    _elementwise(adj, ops, 64, "virtual CSR with values")
    ops = exact_operands("col16", "wide_factored")
    adj = _adj(ops, slices=2)
    adj.set_value_factors(_t(ops["u_row"]), _t(ops["u_col"]))
    adj.set_gather_width(4)
    assert adj.has_value_factors and adj.main_kernel(64) == "gcn::spmm_quad_kernel<16, false, true, true>", adj.main_kernel(64)
    _elementwise(adj, ops, 64, "virtual CSR value-free, 16-bit columns")


def test_elementwise_panels():
    """LDS panels and dense MFMA panels (v_mfma_f32_32x32x2_f32: fp32 products and sums; a tile's zeros add exactly, so the
    operation count of a row stays its stored length)"""
    ops = exact_operands("lds", "wide")
    adj = _adj(ops, panels=1)
    assert adj.panel_rows > 0 and adj.dense_panels == 0
    for k in (64, 100):
        assert adj.main_kernel(k) == "gcn::spmm_panel_in_kernel"
        _elementwise(adj, ops, k, "LDS panels")
    ops = exact_operands("mfma", "wide")
    adj = _adj(ops, panels=1)
    assert adj.dense_panels >= 10
    for k in (36, 128):
        assert adj.main_kernel(k) == "gcn::spmm_panel_in_kernel"
        _elementwise(adj, ops, k, "MFMA panels")


@pytest.mark.parametrize("weighted", [False, True], ids=["value_free", "weighted"])
def test_bf16_bound_on_wide_range_operands(weighted):
    """util.bf16_assert_bound as tests/test_bf16_gpu.py uses it, on the wide-range operands: hot path, then a fallback plan"""
    adj, ops = _group_adj("group" if weighted else "group_dup", "wide" if weighted else "wide_factored")
    want = "gcn::spmm_group_bf16_weighted_kernel<" if weighted else "gcn::spmm_group_bf16_kernel<"
    for k in (64, 136):
        B16 = _t(wide_features(ops["n"], k, seed=9000 + k), torch.bfloat16)
        Cref, absref = bf16_reference(ops["rp"], ops["ci"], ops["va"], B16)
        C32 = adj.matmul_raw(B16, out=torch.empty((ops["m"], k), device=DEV))
        assert adj.main_kernel(k, dtype=torch.bfloat16).startswith(want), (k, adj.main_kernel(k, dtype=torch.bfloat16))
        bf16_assert_bound(C32, Cref, absref, bf16_out=False)
        bf16_assert_bound(adj.matmul_raw(B16), Cref, absref, bf16_out=True)
    if weighted:
        adj, ops = _unsliced_adj("quad16", 4, "wide")
        assert not adj.main_kernel(64, dtype=torch.bfloat16).startswith("gcn::spmm_group_bf16")
        B16 = _t(wide_features(ops["n"], 64, seed=9500), torch.bfloat16)
        Cref, absref = bf16_reference(ops["rp"], ops["ci"], ops["va"], B16)
        bf16_assert_bound(adj.matmul_raw(B16), Cref, absref, bf16_out=True)
