"""Operands that are not 16-byte aligned, on every kernel family.  A contiguous view at a 4-byte (bf16: 2-byte) offset
is legal input everywhere — a row slice of an odd-width matrix, a parameter inside a flat buffer — and the Python
wrappers hand its pointer straight to the C ABI.  The launchers then pick a scalar fallback from (ptr & 15) (DESIGN.md,
"Operand alignment"): these tests reach those fallbacks.  Every operand comes from util.offset_view: a view at a chosen
offset from a 16-byte boundary inside a sentinel-filled buffer, so a store outside the operand is seen.

Held to: the 1e-5 contract against the fp64 oracle; the same bits from two calls on one plan; empty rows exactly 0 (or
relu(bias)); guards intact; inputs unchanged.  Aligned and misaligned SpMM runs take different kernels, so their bits
may differ; the SDDMM and gather_rows promise the same bits everywhere and are held to that."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gcn_amd
from util import (banded_csr, bf16_assert_bound, bf16_reference, check_sddmm, dense_band_csr, guards_intact, offset_view,
                  oracle_spmm, random_csr, rel_err, sddmm_graph, sddmm_ref, sym_norm_graph)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-5
F32, BF16 = torch.float32, torch.bfloat16
SETS = ("B", "C", "bias", "all")                         # which operands sit off the 16-byte grid

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _adj(g, **kw):
    rp, ci, va, m, n = g
    return gcn_amd.CsrAdjacency(_t(rp), _t(ci), _t(va), (m, n), **kw)


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _graph(name):
    def make():
        if name == "long":                               # 80 per row (test_main_kernel_families_are_selected_as_documented)
            return (*random_csr(1000, 1000, 80000, seed=1), 1000, 1000)
        if name == "ragged":                             # empty rows, hub rows, rows of 1..5 (test_parity_gather_widths)
            m, n = 3000, 5000
            return (*random_csr(m, n, 30000, seed=64, empty_rows=0.2,
                                long_rows=[(0, 0), (5, 4097), (6, 64), (7, 128), (8, 1), (9, 2), (10, 3), (11, 63),
                                           (12, 65), (2000, 2500), (m - 1, 0), (m - 2, 5)]), m, n)
        if name == "sym":                                # normalised: the values factor (value-free pass when sliced)
            return (*sym_norm_graph(3000, 90000, seed=2), 3000, 3000)
        if name == "sym_random":                         # the same pattern, values that do not factor
            rp, ci, va = sym_norm_graph(3000, 90000, seed=2)
            return rp, ci, (np.random.default_rng(5).standard_normal(len(va)) * 0.5).astype(np.float32), 3000, 3000
        if name == "banded":                             # test_parity_lds_staged_row_panels
            return (*banded_csr(3001, 150, 3, seed=64, hub=(777, 2600)), 3001, 3001)
        if name == "dense_band":                         # test_dense_panels_run_on_the_matrix_cores
            return (*dense_band_csr(2500, 200, 0.6, seed=64, sparse_from=1700), 2500, 2500)
        if name == "bf16":                               # the plan of tests/test_bf16_gpu.py's hot path
            return (*sym_norm_graph(4000, 120000, seed=3), 4000, 4000)
        return sddmm_graph(name)                         # "rect", "reddit"
    return _cached(("graph", name), make)


def _features(name, k):
    def make():
        g = _graph(name)
        rng = np.random.default_rng(k)
        B = rng.standard_normal((g[4], k)).astype(np.float32)
        bias = rng.standard_normal(k).astype(np.float32)
        return B, bias, oracle_spmm(g[0], g[1], g[2], B)
    return _cached(("features", name, k), make)


def _offsets(which, off, epilogue):
    if which == "all":
        return off, off, off
    return (off if which == "B" else 0, off if which == "C" else 0, off if which == "bias" and epilogue else 0)


def _check_spmm(adj, name, k, which, off, epilogue, Cref=None):
    """one misaligned call, twice: oracle, determinism, empty rows, guards, inputs"""
    g = _graph(name)
    B, bias, ref = _features(name, k)
    if Cref is not None:
        ref = Cref
    ob, oc, obias = _offsets(which, off, epilogue)
    Bv, Bflat = offset_view(B, ob, F32, DEV)
    biasv, biasflat = offset_view(bias, obias, F32, DEV)
    B_bits, bias_bits = _bits(Bv).clone(), _bits(biasv).clone()
    kw = dict(bias=biasv, relu=True) if epilogue else {}
    where = (name, k, which, off, epilogue)
    runs = []
    for _ in range(2):
        out, outflat = offset_view((adj.m, k), oc, F32, DEV)           # sentinel-filled: every element must be written
        got = adj.matmul_raw(Bv, out=out, **kw)
        assert got.data_ptr() == out.data_ptr()
        assert guards_intact(outflat, out), where
        runs.append(out)
    assert torch.equal(_bits(runs[0]), _bits(runs[1])), where
    assert guards_intact(Bflat, Bv) and guards_intact(biasflat, biasv), where
    assert torch.equal(_bits(Bv), B_bits) and torch.equal(_bits(biasv), bias_bits), where
    C = runs[0].cpu().numpy()
    want = np.maximum(ref + bias, 0) if epilogue else ref
    assert rel_err(C, want) <= TOL, where                               # (a sentinel left behind is a NaN: fails here)
    empty = np.diff(g[0]) == 0
    if empty.any():
        fill = np.maximum(bias, 0) if epilogue else np.zeros(k, np.float32)
        assert np.array_equal(C[empty], np.broadcast_to(fill, C[empty].shape)), where
    return runs[0]


def _sets(epilogue):
    return SETS if epilogue else tuple(s for s in SETS if s != "bias")


# ---- unsliced SpMM, automatic gather width ----
@pytest.mark.parametrize("k", [4, 8, 15, 16, 32, 41, 64, 128])
def test_unsliced_spmm_every_operand_set(k):
    """aligned, k >= 16 (k % 4 == 0) runs the quad kernel; off the grid spmm_quad_eligible refuses and the call lands on
    the narrow kernels (k <= 16) or spmm_chunk_kernel<1> — and stays correct"""
    adj = _cached(("plan", "long"), lambda: _adj(_graph("long")))
    if k >= 16 and k % 4 == 0:
        assert "quad" in adj.main_kernel(k)
    for epilogue in (False, True):
        for which in _sets(epilogue):
            _check_spmm(adj, "long", k, which, 1, epilogue)


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("k", [16, 64])
def test_unsliced_spmm_every_offset(k, off):
    adj = _cached(("plan", "long"), lambda: _adj(_graph("long")))
    for epilogue in (False, True):
        for which in _sets(epilogue):
            _check_spmm(adj, "long", k, which, off, epilogue)


# ---- spmm_chunk_kernel<4> / <2>: the wide tiles ----
@pytest.mark.parametrize("tile", [256, 128])
def test_wide_tile_chunk_kernels(tile):
    """pick_vec looks at B, C and P — 16-byte rule for 4 floats per lane, 8-byte rule for 2.  The bias pointer is not
    among them: a bias at a 4-byte offset with B and C aligned keeps VEC = 4 / 2, and the kernel reads the bias float
    by float (the audited case: it used to be one 16- / 8-byte load)."""
    def make():
        adj = _adj(_graph("long"))
        adj.set_gather_width(1)
        adj.set_tile_cols(tile)
        return adj
    adj = _cached(("plan", "long", "tile", tile), make)
    assert adj.main_kernel(256, epilogue=True).startswith(f"gcn::spmm_chunk_kernel<{tile // 64},")
    for which, off in (("B", 0), ("bias", 1), ("bias", 2), ("bias", 3), ("B", 2), ("B", 1), ("C", 2), ("C", 1),
                       ("all", 2), ("all", 1)):
        _check_spmm(adj, "long", 256, which, off, True)


# ---- ragged matrix: empty rows through fill_empty_rows<1>, cut rows through P ----
@pytest.mark.parametrize("k", [16, 64, 128])
def test_ragged_matrix_with_the_output_off_the_grid(k):
    adj = _cached(("plan", "ragged"), lambda: _adj(_graph("ragged"), chunk_nnz=64))
    for which, off in (("C", 1), ("C", 2), ("bias", 1), ("all", 3)):
        _check_spmm(adj, "ragged", k, which, off, True)
    _check_spmm(adj, "ragged", k, "C", 1, False)


# ---- sliced plans ----
@pytest.mark.parametrize("k", [32, 64, 128, 512])
@pytest.mark.parametrize("plan", ["value_free", "mutable", "virtual_csr"])
def test_sliced_plans(plan, k):
    """value-free and weighted group kernels gather from the plan's own re-laid copy of B (a misaligned B takes the
    scalar loads of the re-lay); values that do not factor walk the virtual CSR on the quad / chunk kernels; an output
    or bias off the grid sends the reduction over slices to slice_reduce_kernel<1>"""
    name = "sym" if plan == "value_free" else "sym_random"
    adj = _cached(("plan", plan), lambda: _adj(_graph(name), slices=4, mutable_values=plan == "mutable"))
    assert adj.num_slices == 4
    for epilogue in (False, True):
        for which in _sets(epilogue):
            _check_spmm(adj, name, k, which, 1, epilogue)
    _check_spmm(adj, name, k, "all", 2, True)


# ---- LDS-staged panels, dense MFMA panels ----
@pytest.mark.parametrize("k", [64, 100])
@pytest.mark.parametrize("name", ["banded", "dense_band"])
def test_panels(name, k):
    """launch_panel_in looks at C only (its reads of B are 4 bytes wide); the out-of-window part accumulates through
    launch_spmm and its gates"""
    adj = _cached(("plan", name), lambda: _adj(_graph(name), panels=1))
    assert adj.panel_rows > 0
    if name == "dense_band":
        assert adj.dense_panels > 0
    for epilogue in (False, True):
        for which in _sets(epilogue):
            _check_spmm(adj, name, k, which, 1, epilogue)
    _check_spmm(adj, name, k, "C", 2, True)


# ---- bf16 ----
@pytest.mark.parametrize("k", [128, 40])
def test_bf16_operands(k):
    """hot path (k = 128: bf16 group walk; launch_relay_bf16_sliced's src_vec, launch_slice_reduce's vec_out for a bf16 result — an
    8-byte rule, so 4 halves pass it and fail the 16-byte ones) and fallback (k = 40); bounds of tests/test_bf16_gpu.py"""
    g = _graph("bf16")
    adj = _cached(("plan", "bf16"), lambda: _adj(g, symmetric=True, slices=4))
    assert adj.main_kernel(k, dtype=BF16).startswith("gcn::spmm_group_bf16") == (k == 128)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(k)
    B = torch.randn((g[4], k), generator=gen).to(BF16)
    Cref, absref = bf16_reference(g[0], g[1], g[2], B)
    cases = [(ob, BF16, 0) for ob in (1, 2, 4)] + [(0, BF16, 1), (0, BF16, 4), (0, F32, 1), (1, BF16, 1), (4, F32, 1)]
    for ob, cdtype, oc in cases:
        Bv, Bflat = offset_view(B, ob, BF16, DEV)
        B_bits = _bits(Bv).clone()
        runs = []
        for _ in range(2):
            out, outflat = offset_view((adj.m, k), oc, cdtype, DEV)
            adj.matmul_raw(Bv, out=out)
            assert guards_intact(outflat, out), (k, ob, cdtype, oc)
            runs.append(out)
        assert torch.equal(_bits(runs[0]), _bits(runs[1]))
        assert guards_intact(Bflat, Bv) and torch.equal(_bits(Bv), B_bits)
        bf16_assert_bound(runs[0], Cref, absref, bf16_out=cdtype == BF16)


# ---- the matrix arrays themselves ----
@pytest.mark.parametrize("plan", ["unsliced", "sliced", "mutable"])
def test_matrix_arrays_off_the_grid(plan):
    """rowptr, col and val at a 1-element offset (every kernel reads them 4 bytes at a time); update_values with new
    values at a 1-element offset"""
    name = {"unsliced": "ragged", "sliced": "sym", "mutable": "sym_random"}[plan]
    rp, ci, va, m, n = _graph(name)
    rpv, rpflat = offset_view(rp, 1, torch.int32, DEV)
    civ, ciflat = offset_view(ci, 1, torch.int32, DEV)
    vav, vaflat = offset_view(va, 1, F32, DEV)
    kw = dict(unsliced=dict(slices=0, chunk_nnz=64), sliced=dict(slices=4), mutable=dict(slices=4, mutable_values=True))[plan]
    adj = gcn_amd.CsrAdjacency(rpv, civ, vav, (m, n), **kw)
    assert adj.rowptr.data_ptr() == rpv.data_ptr() and adj.col.data_ptr() == civ.data_ptr()
    assert adj.rowptr.data_ptr() % 16 == 4
    for k in (16, 64):
        _check_spmm(adj, name, k, "B", 0, True)
        _check_spmm(adj, name, k, "all", 1, False)
    if plan == "mutable":
        new = (np.random.default_rng(9).standard_normal(len(va)) * 0.5).astype(np.float32)
        newv, newflat = offset_view(new, 1, F32, DEV)
        adj.update_values(newv)
        assert guards_intact(newflat, newv) and np.array_equal(newv.cpu().numpy(), new)
        B, _, _ = _features(name, 64)
        _check_spmm(adj, name, 64, "all", 1, True, Cref=oracle_spmm(rp, ci, new, B))
    for v, f, a in ((rpv, rpflat, rp), (civ, ciflat, ci), (vav, vaflat, va)):
        assert guards_intact(f, v) and np.array_equal(v.cpu().numpy(), a)


# ---- SDDMM ----
@pytest.mark.parametrize("k", [8, 41, 64, 128])
@pytest.mark.parametrize("name,slices", [("rect", 0), ("rect", 4), ("reddit", 4)])
def test_sddmm(name, slices, k):
    """sddmm_vec looks at A and B; the result is promised bit-identical on every plan and call, so also across the
    vector and scalar loads"""
    g = _graph(name)
    rp, ci, va, m, n = g
    adj = _cached(("plan", "sddmm", name, slices), lambda: _adj(g, slices=slices))
    rng = np.random.default_rng(k)
    A = rng.standard_normal((m, k)).astype(np.float32)
    B = rng.standard_normal((n, k)).astype(np.float32)
    ref, mag = sddmm_ref(rp, ci, A, B, DEV)
    aligned = adj.sddmm(_t(A), _t(B))
    check_sddmm(aligned, ref, mag)
    for oa, ob, oo in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 3, 0), (1, 1, 1), (3, 2, 2)):
        Av, Aflat = offset_view(A, oa, F32, DEV)
        Bv, Bflat = offset_view(B, ob, F32, DEV)
        out, outflat = offset_view((adj.nnz,), oo, F32, DEV)
        adj.sddmm(Av, Bv, out=out)
        assert guards_intact(outflat, out) and guards_intact(Aflat, Av) and guards_intact(Bflat, Bv), (oa, ob, oo)
        assert np.array_equal(Av.cpu().numpy(), A) and np.array_equal(Bv.cpu().numpy(), B)
        check_sddmm(out, ref, mag)
        assert torch.equal(_bits(out), _bits(aligned)), (name, slices, k, oa, ob, oo)


# ---- gather_rows ----
@pytest.mark.parametrize("k", [4, 41, 64])
def test_gather_rows(k):
    rng = np.random.default_rng(k)
    src = rng.standard_normal((777, k)).astype(np.float32)
    idx = rng.integers(0, 777, 1500).astype(np.int32)
    for os_, od, oi in ((1, 0, 0), (0, 1, 0), (1, 1, 0), (2, 3, 1), (0, 0, 1)):
        sv, sflat = offset_view(src, os_, F32, DEV)
        iv, iflat = offset_view(idx, oi, torch.int32, DEV)
        out, outflat = offset_view((1500, k), od, F32, DEV)
        gcn_amd.gather_rows(sv, iv, out=out)
        assert np.array_equal(out.cpu().numpy().view(np.int32), src[idx].view(np.int32)), (k, os_, od, oi)
        assert guards_intact(outflat, out) and guards_intact(sflat, sv) and guards_intact(iflat, iv)
        assert np.array_equal(sv.cpu().numpy(), src)


# ---- the pre-laid entry refuses instead of falling back ----
def test_prelaid_entry_refuses_operands_off_the_grid():
    """gcn_spmm_csr_f32_prelaid: B' or the output off the 16-byte grid -> GCN_ERR_INVALID_ARG, nothing written"""
    adj = lay = None
    for name, k in (("sym", 128), ("sym", 64), ("bf16", 128)):
        adj = _adj(_graph(name), symmetric=True, slices=4)
        lay = adj.prelaid_layout(k)
        if lay is not None:
            break
    assert lay is not None, "no small plan with a pre-laid layout"
    shape = (lay["table_rows"], lay["ld"])
    Bp = torch.zeros(shape, device=DEV)
    adj.matmul_prelaid(Bp, torch.empty((adj.m, k), device=DEV))            # aligned: accepted
    for ob, oo in ((1, 0), (0, 1), (2, 2)):
        Bv, _ = offset_view(Bp, ob, F32, DEV)
        out, outflat = offset_view((adj.m, k), oo, F32, DEV)
        with pytest.raises(gcn_amd.GcnAmdError) as e:
            adj.matmul_prelaid(Bv, out)
        assert e.value.status == 1                                          # GCN_ERR_INVALID_ARG
        torch.cuda.synchronize()
        assert bool(torch.all(_bits(outflat) == 0x7FC12345)), (ob, oo)      # the output too: untouched


# ---- autograd ----
def test_autograd_with_misaligned_features_and_gradient():
    m, n, k = 700, 900, 64
    rowptr, col, val = random_csr(m, n, 9000, seed=8)
    adj = _adj((rowptr, col, val, m, n), symmetric=False)
    rng = np.random.default_rng(2)
    B = rng.standard_normal((n, k)).astype(np.float32)
    G = rng.standard_normal((m, k)).astype(np.float32)
    Bv, Bflat = offset_view(B, 1, F32, DEV)
    Gv, Gflat = offset_view(G, 3, F32, DEV)
    Bv.requires_grad_(True)
    C = gcn_amd.spmm(adj, Bv)
    C.backward(Gv)
    assert rel_err(C.detach().cpu().numpy(), oracle_spmm(rowptr, col, val, B)) <= TOL
    At = sp.csr_matrix((val, col, rowptr), shape=(m, n)).T.tocsr(); At.sort_indices()
    gref = oracle_spmm(At.indptr.astype(np.int32), At.indices.astype(np.int32), At.data.astype(np.float32), G)
    assert rel_err(Bv.grad.cpu().numpy(), gref) <= TOL
    assert guards_intact(Bflat, Bv.detach()) and guards_intact(Gflat, Gv)
    assert np.array_equal(Bv.detach().cpu().numpy(), B) and np.array_equal(Gv.cpu().numpy(), G)
