"""The plan recipes of the exact-arithmetic SpMM tests, shared by tests/test_exact_gpu.py and tests/test_nonfinite_gpu.py: the
plans that force every kernel family onto util.exact_pattern's matrices (built once per process and kept), the assertion of the
group kernel a width runs, and the list of fused-epilogue cases with the plan and the kernel-name assertions of each.  The
recipes that force a family are those of tests/test_contract_gpu.py.  GPU only: importing this module needs no device, calling
it does."""
import os

import numpy as np
import torch

import gcn_amd
from util import EPILOGUE_NINE_SLICES, EXACT_EPILOGUE_CASES, HUB_MIN, exact_operands

DEV = torch.device("cuda:0")

UNSLICED = [("narrow4", 4, 0), ("narrow8", 8, 0), ("narrow16_dpp", 15, 0), ("quad4", 16, 4), ("quad16", 36, 4),
            ("quad16", 128, 4), ("chunk1", 100, 1), ("chunk1", 128, 1), ("chunk2", 128, 1), ("chunk4", 256, 1)]
UNSLICED_NAMES = {"narrow4": "spmm_narrow_kernel<4,", "narrow8": "spmm_narrow_kernel<8,", "narrow16_dpp": "spmm_narrow16_dpp_kernel",
                  "quad4": "spmm_quad_kernel<4,", "quad16": "spmm_quad_kernel<16,", "chunk1": "spmm_chunk_kernel<1,",
                  "chunk2": "spmm_chunk_kernel<2,", "chunk4": "spmm_chunk_kernel<4,"}
GROUP_WIDTHS = [16, 32, 40, 41, 64, 100, 128]
_G8 = os.environ.get("GCN_AMD_GROUP8", "1") != "0"


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _adj(ops, hub=True, **kw):
    lens = np.diff(ops["rp"])
    assert (lens.max() >= HUB_MIN or not hub) and (lens <= 1).sum() >= 2   # a hub row and empty (or diagonal-only) rows
    return gcn_amd.CsrAdjacency(_t(ops["rp"]), _t(ops["ci"]), _t(ops["va"]), (ops["m"], ops["n"]), **kw)


_PLANS = {}


def _unsliced_adj(family, gather, kind):
    """a plan per (family, values): chunk_nnz=128 (the hub row crosses 15 chunks), the family forced as test_contract_gpu does"""
    key = ("unsliced", family, kind)
    if key not in _PLANS:
        ops = exact_operands("unsliced", kind)
        adj = _adj(ops, chunk_nnz=128, slices=0)
        adj.set_gather_width(gather)
        if family == "chunk2":
            adj.set_tile_cols(128)
        if family == "chunk4":
            adj.set_tile_cols(256)
        _PLANS[key] = (adj, ops)
    return _PLANS[key]


def _group_adj(pattern, kind, hand_over=True, slices=3):
    """the slices=3 plan of a 6000-vertex graph: the 15-bit slice-major stream and its kernels (slices=9: the same graph in
    slices of 667 columns, one unrolled group of eight and a tail of one in the wide slice reduction)"""
    key = ("group", pattern, kind, hand_over, slices)
    if key not in _PLANS:
        ops = exact_operands(pattern, kind)
        adj = _adj(ops, slices=slices)
        if ops["u_row"] is not None and hand_over:
            adj.set_value_factors(_t(ops["u_row"]), _t(ops["u_col"]))
        assert adj.num_slices == slices
        assert adj.has_value_factors == (ops["u_row"] is not None), (pattern, kind)
        _PLANS[key] = (adj, ops)
    return _PLANS[key]


def _special_adj(pattern):
    """the cached plans of the sliced four-per-gather routes and of the panels, as their plain exact tests force them"""
    key = ("special", pattern)
    if key not in _PLANS:
        if pattern == "vcsr":                                        # slices of 35 000 columns cannot use the 15-bit stream
            ops = exact_operands("vcsr", "int")
            adj = _adj(ops, slices=4)
            adj.set_gather_width(4)
            assert adj.num_slices == 4 and not adj.has_value_factors
        elif pattern == "col16":                                     # value-free on the 16-bit column stream, two slices
            ops = exact_operands("col16", "pow2")
            adj = _adj(ops, slices=2)
            adj.set_value_factors(_t(ops["u_row"]), _t(ops["u_col"]))
            adj.set_gather_width(4)
            assert adj.num_slices == 2 and adj.has_value_factors
        elif pattern == "lds":
            ops = exact_operands("lds", "int")
            adj = _adj(ops, panels=1)
            assert adj.panel_rows > 0 and adj.dense_panels == 0 and adj.panel_coverage < 1.0
        elif pattern == "lds_all":                                   # nothing outside the windows: launch_panel_epilogue
            ops = exact_operands("lds_all", "int")
            adj = _adj(ops, hub=False, panels=1)
            assert adj.panel_rows > 0 and adj.dense_panels == 0 and adj.panel_coverage == 1.0
        else:
            ops = exact_operands("mfma", "int")
            adj = _adj(ops, panels=1)
            assert adj.dense_panels >= 10
        _PLANS[key] = (adj, ops)
    return _PLANS[key]


def _assert_group_kernel(adj, k, weighted):
    name = adj.main_kernel(k)
    assert name.startswith("gcn::spmm_group") and ("weighted" in name) == weighted, (k, name)
    if _G8 and k <= 32:                                              # eight 8-lane engines per wave
        assert name.startswith("gcn::spmm_group8_weighted_kernel<" if weighted else "gcn::spmm_group8_kernel<"), (k, name)
    elif k <= 32 or weighted:
        assert name.startswith("gcn::spmm_group_weighted_kernel<" if weighted else "gcn::spmm_group_ring_kernel<"), (k, name)
    elif 33 <= k <= 48:                                              # five 12-lane engines (GCN_AMD_GROUP12=0: the ring kernel)
        assert name in ("gcn::spmm_group12_kernel", "gcn::spmm_group_ring_kernel<false>"), (k, name)
    else:                                                            # four 16-lane engines
        assert name.startswith("gcn::spmm_group_ring_kernel<"), (k, name)
    return name


# the fused epilogue: every route x every piece of code that carries it
UNSLICED_EPI = {"narrow4": "spmm_narrow_kernel<4, 4, true,", "narrow8": "spmm_narrow_kernel<8, 8, true,",
                "narrow16_dpp": "spmm_narrow16_dpp_kernel<true>", "quad4": "spmm_quad_kernel<4, true,", "quad16": "spmm_quad_kernel<16, true,",
                "chunk1": "spmm_chunk_kernel<1, 32, true,", "chunk2": "spmm_chunk_kernel<2, 8, true,", "chunk4": "spmm_chunk_kernel<4, 4, true,"}
_VF = {"pow2": "value_free", "int": "weighted"}


def _epi_cases():
    """(id, carrier, pattern, kind, k, options).  Which slice reduction launch_slice_reduce's rule selects stands beside
    every case that has one: slice_reduce_wide_kernel for k % 4 == 0, k <= 256 and 16-byte aligned Cv, C, bias and cut slab
    (DROP = the mask is on; rows per wave and step 256 / k), slice_reduce_kernel<4> for k % 4 == 0 beyond 256 columns,
    slice_reduce_kernel<1> for everything else."""
    c = []
    # the main kernel carries bias / ReLU (EPI), the empty-row pass writes act(bias), the mask is launch_dropout over m * k
    for family, k, gather in [("narrow4", 4, 0), ("narrow8", 8, 0), ("narrow16_dpp", 15, 0), ("narrow16_dpp", 16, 0), ("quad4", 16, 4),
                              ("quad16", 36, 4), ("quad16", 128, 4), ("chunk1", 100, 1),
                              ("chunk1", 41, 1),            # gather width 1: no detour, VEC = 1, a mask count that is no multiple of 4
                              ("chunk2", 128, 1), ("chunk4", 256, 1)]:
        c.append((f"main-{family}-k{k}", "main", "unsliced", "int", k, dict(family=family, gather=gather)))
    # the detour at k' = ceil(k / 4) * 4: launch_unpad_rows carries bias / ReLU, the mask is launch_dropout over m * k with
    # the CALLER's k.  The group plans reduce at k' (44: wide kernel, DROP = false, five rows per step; 24: ten) with no epilogue
    c.append(("detour-unsliced-k41", "detour", "unsliced", "int", 41, dict(family="quad16", gather=4)))
    c.append(("detour-group_value_free-k41", "detour", "group_dup", "pow2", 41, {}))
    c.append(("detour-group_value_free-k21", "detour", "group_dup", "pow2", 21, {}))
    c.append(("detour-group_weighted-k41", "detour", "group_dup", "int", 41, {}))
    # the slice reduction carries everything, the row factor (value-free) and the cut-row pieces included
    for kind in ("pow2", "int"):
        for k in (16, 32,                                   # wide kernel, DROP, 16 and 8 rows per wave and step
                  40,                                       # wide kernel, six rows per step, four lanes idle
                  64, 128,                                  # wide kernel, four and two rows per step
                  260):                                     # k > 256: slice_reduce_kernel<4>
            c.append((f"reduce-{_VF[kind]}-k{k}", "reduce", "group_dup", kind, k, {}))
        for k in EPILOGUE_NINE_SLICES["group_dup"]:         # wide kernel: one unrolled group of eight slices and a tail of one
            c.append((f"reduce9-{_VF[kind]}-k{k}", "reduce", "group_dup", kind, k, dict(slices=9)))
        # the bias one float off the 16-byte grid: slice_reduce_kernel<1>, its scalar mask path
        c.append((f"reduce-{_VF[kind]}-k64-bias_off_grid", "reduce", "group_dup", kind, 64, dict(bias_off=1)))
    # sliced, four per gather: the wide kernel at k = 64 without cut lists; col16 with the row factor
    c.append(("reduce-vcsr-k64", "sliced_quad", "vcsr", "int", 64, {}))
    c.append(("reduce-col16-k64", "sliced_quad", "col16", "pow2", 64, {}))
    # panels: the accumulating chunk kernel over the entries outside the windows carries bias / ReLU; lds_all has none
    # outside, there launch_panel_epilogue does; the mask is launch_dropout
    for pattern, widths in (("lds", (64, 100)), ("mfma", (36, 64, 128)), ("lds_all", (64, 100))):
        for k in widths:
            c.append((f"panels-{pattern}-k{k}", "panels", pattern, "int", k, {}))
    # bf16 operands: an fp32 result through launch_slice_reduce (wide kernel), a bf16 one through slice_reduce_bf16_kernel
    # (one rounding after the epilogue); an unsliced plan widens, runs the fp32 entry (EPI in the main kernel) and narrows
    for kind in ("pow2", "int"):
        for k in (64, 128, 136):
            c.append((f"bf16-{_VF[kind]}-k{k}", "bf16", "group_dup", kind, k, {}))
    c.append(("bf16-fallback-quad16-k64", "bf16_fallback", "unsliced", "int", 64, dict(family="quad16", gather=4)))
    return c


EPI_CASES = _epi_cases()
assert all(any((p, kd) == (tp, tk) and k in tw for tp, tk, tw in EXACT_EPILOGUE_CASES) for _i, _c, p, kd, k, _o in EPI_CASES)


def smallest_epilogue_cases():
    """EPI_CASES at the smallest width of each family — one case per (carrier, matrix, values, options) — and every case
    beyond 256 columns, where the slice reduction is another kernel: what tests/test_nonfinite_gpu.py runs"""
    best = {}
    for case in EPI_CASES:
        _cid, carrier, pattern, kind, k, opt = case
        key = (carrier, pattern, kind, tuple(sorted(opt.items())))
        if key not in best or k < best[key][4]:
            best[key] = case
    picked = {c[0] for c in best.values()} | {c[0] for c in EPI_CASES if c[4] > 256}
    return [c for c in EPI_CASES if c[0] in picked]


def epilogue_slices(pattern, opt):
    """the column-slice count of an epilogue case's plan (0: unsliced or panels)"""
    return opt.get("slices", {"group_dup": 3, "vcsr": 4, "col16": 2}.get(pattern, 0))


def _epilogue_plan(carrier, pattern, kind, k, opt):
    """the plan of a case, with the assertion that it runs the kernel and takes the route the case is about"""
    bf16 = carrier.startswith("bf16")
    if pattern == "unsliced":
        adj, ops = _unsliced_adj(opt["family"], opt["gather"], kind)
        name, plain = adj.main_kernel(k, True), adj.main_kernel(k, False)
        if carrier == "detour":                              # the main kernel runs without its epilogue
            assert name == plain and "spmm_quad_kernel<16, false," in name, (name, plain)
        else:
            assert UNSLICED_EPI[opt["family"]] in name and UNSLICED_NAMES[opt["family"]] in plain and name != plain, (name, plain)
        if bf16:
            assert adj.main_kernel(k, True, dtype=torch.bfloat16) == name
    elif pattern == "group_dup":
        adj, ops = _group_adj(pattern, kind, slices=opt.get("slices", 3))
        assert adj.num_slices == opt.get("slices", 3)
        if not bf16:                                         # (the bf16 name after the call: k = 64 may build a slice set)
            name = _assert_group_kernel(adj, k, kind == "int")
            assert adj.main_kernel(k, True) == name          # the walk carries no epilogue: the reduction or the compaction does
    else:
        adj, ops = _special_adj(pattern)
        name = adj.main_kernel(k, True)
        if pattern == "vcsr":
            assert name.startswith("gcn::spmm_quad_kernel<16, false, false,") and name == adj.main_kernel(k), name
        elif pattern == "col16":
            assert name == "gcn::spmm_quad_kernel<16, false, true, true>", name
        else:
            assert name == "gcn::spmm_panel_in_kernel", name
    return adj, ops
