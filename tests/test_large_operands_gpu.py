"""Sparse-touch tests: every feature-table kernel with one operand past 2^31 elements or 4 GiB.  The graph is tiny (tens of
thousands of entries at the most); its row or column count is large enough that the rows it touches lie beyond the 32-bit
thresholds of one big dense operand (tests/large_ref.py: B32, E31, E32, and the bands of 64 rows around them).  The big
operand is filled on the device from ``large_ref.feat`` in row chunks, the twin evaluates feat only at the touched rows, and
every comparison is bit for bit: the values are small integers and eighths, so every sum is exact in fp32 in any order.  An
offset that wraps reads or writes a valid address lower in the same tensor; tests/test_large_operands_cpu.py proves that every
such truncation, on the gather side and on the store side, changes what is compared here.

A big result starts as NaN (arg: -2) wherever the entry point takes the result tensor; after the call the rows outside the
bands are checked on the device, in reductions over the tensor, to hold what the unit defines for an empty row, and the
bands are compared on the host with the twin.  Each case holds one big operand (or one big result with its arg), frees it in
a ``finally`` and prints one line: the main kernel's name, the peak device memory, the wall time.

The pre-laid entry is the one case that is no tiny graph: its value-free pass exists from 48 entries per column, so its table
passes 4 GiB by the width of its rows (8192 floats) on a matrix of 6.5 M entries, compared on sampled rows and columns.
Not here: the bf16 epilogue on forced slices at E32 (two fp32 planes of partial rows of 16 GiB beside the result: more than
the 40 GiB a test may hold; it runs at E31, where the result has 4 GiB).

Out of scope, because they take no [rows, k] operand and their sizes are bounded by nnz < 2^31, which the ABI refuses to
exceed (the *_cpu.py files): construct, coalesce, sampling and subgraph, SpGEMM and sampled_dot, lookup and negative
sampling.  The multi-rank exchange is out too."""
import contextlib
import time

import numpy as np
import pytest
import torch

import gcn_amd
import large_ref as lr
from gcn_amd._lib import call
from gcn_amd.aggregate import _DTYPE, _REDUCE, _scratch
from gcn_amd.attention import _workspace
from util import assert_exact

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TORCH = {"fp32": torch.float32, "bf16": torch.bfloat16}
GIB = 1 << 30
FILL_ROWS = 1 << 15                                      # rows per chunk of a fill (int64 temporaries of 128 MiB at k = 512)
SCAN_ROWS = 1 << 17


# what a case holds at its peak, in GiB, rounded up: the tensors of the test (measured: torch.cuda.max_memory_allocated) and
# the plan's own slabs beside them (the planes of partial rows of a sliced call, the fp32 copies the unsliced bf16 calls widen
# from and narrow to, the group layout's copy of a big table)
NEED = {"spmm_in_f32_E31": 9, "spmm_in_bf16_E32": 25, "spmm_in_f32_E31_group_big": 18, "spmm_in_bf16_E31_group_big": 10,
        "spmm_out_f32_E31_vec4": 9, "spmm_out_f32_E31_vec2": 9, "spmm_out_f32_E31_vec1": 9, "spmm_out_f32_E31_quad": 9,
        "spmm_out_f32_B32_sliced_k256": 13, "spmm_out_bf16_E32": 25, "epilogue_out_f32_E31": 9,
        "epilogue_out_f32_E31_sliced_k256": 25, "epilogue_out_bf16_E32": 25, "epilogue_out_bf16_E31_sliced_k256": 21,
        "prelaid_table_B32": 18, "spmm_backward_E31": 17, "sddmm_A_f32_E31": 9, "sddmm_B_f32_E31": 9, "sddmm_B_bf16_E31": 13,
        "aggregate_max_in_f32_E31": 9, "aggregate_min_in_bf16_E32": 9, "aggregate_max_out_bf16_E32": 25,
        "aggregate_min_out_f32_E31": 17, "aggregate_backward_E31": 17, "spmm_heads_in_E31": 9, "spmm_heads_in_E31_F63": 9,
        "spmm_heads_out_E31": 9, "spmm_heads_backward_E31": 17, "sddmm_heads_A_E31": 9, "sddmm_heads_B_E31": 9,
        "gatv2_src_E31": 9, "gatv2_dst_E31_F63": 9, "gatv2_grad_src_E31": 17, "gatv2_grad_dst_E31": 17,
        "gat_softmax_dst_E31": 17, "gat_softmax_src_E31": 17, "knn_y_E31": 9, "gather_rows_src_E31": 9,
        "gather_rows_out_E31": 9, "dropout_rows_f32_E32": 17, "dropout_rows_bf16_E32": 9}
assert set(NEED) == set(lr.CASES)


def names(unit, **where):
    return [n for n in sorted(lr.CASES) if lr.CASES[n]["unit"] == unit and all(lr.CASES[n].get(k) == v for k, v in where.items())]


@contextlib.contextmanager
def case(name):
    """the case, with the memory guard in front and the record (and the release of everything) behind"""
    need_gib = NEED[name]
    free = torch.cuda.mem_get_info(DEV)[0]
    if free < (need_gib + 2) * GIB:
        pytest.skip(f"{name} needs {need_gib} GiB + 2 GiB of device memory, {free / GIB:.1f} GiB are free")
    c = dict(lr.build(name))
    c["kernel"] = "-"
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    t0 = time.perf_counter()
    try:
        yield c
        torch.cuda.synchronize()
    finally:
        wall = time.perf_counter() - t0
        peak = torch.cuda.max_memory_allocated(DEV) / GIB
        for key in [k for k, v in c.items() if isinstance(v, (torch.Tensor, gcn_amd.CsrAdjacency))]:
            del c[key]
        torch.cuda.empty_cache()
        print(f"\nLARGE {name}: kernel {c['kernel']}; peak {peak:.2f} GiB; wall {wall:.2f} s" +
              (f" (plan {c['plan_s']:.2f} s)" if "plan_s" in c else ""))


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def fill_table(R, k, dtype, salt):
    """[R, k] of feat(r, j, salt), filled in row chunks with torch ops"""
    t = torch.empty((R, k), dtype=dtype, device=DEV)
    j = torch.arange(k, device=DEV, dtype=torch.int64)[None, :]
    for lo in range(0, R, FILL_ROWS):
        r = torch.arange(lo, min(R, lo + FILL_ROWS), device=DEV, dtype=torch.int64)[:, None]
        t[lo:lo + FILL_ROWS] = lr.feat(r, j, salt)
    return t


def filled(R, k, dtype, value):
    return torch.full((R, k), value, dtype=dtype, device=DEV)


def rows_of(t, rows):
    """the rows `rows` of a device tensor on the host, as fp64 (values) or int64 (indices)"""
    got = t.index_select(0, dev(rows))
    return got.cpu().numpy().astype(np.int64) if got.dtype == torch.int32 else got.double().cpu().numpy()


def outside_bad(t, c, expect=0, also=None):
    """how many elements of the rows outside the bands differ from `expect` (a number or a row [k]; `also`: a second
    admissible row), counted on the device in reductions over row chunks"""
    bad = torch.zeros((), dtype=torch.int64, device=DEV)
    prev = 0
    for _, lo, hi in lr.bands(c["R"], c["k"], lr.itemsizes(c)) + [("end", c["R"], c["R"])]:
        for a in range(prev, lo, SCAN_ROWS):
            seg = t[a:min(lo, a + SCAN_ROWS)]
            ne = seg != expect
            if also is not None:
                ne &= seg != also
            bad += torch.count_nonzero(ne)
        prev = max(prev, hi)
    return int(bad)


def adjacency(c, **kw):
    t0 = time.perf_counter()
    adj = gcn_amd.CsrAdjacency(dev(c["rp"]), dev(c["ci"]), dev(c["va"]), (c["m"], c["n"]), chunk_nnz=lr.CHUNK_NNZ, **kw)
    adj.plan
    torch.cuda.synchronize()
    c["plan_s"] = time.perf_counter() - t0
    return adj


def small(c, dtype=torch.float32):
    return dev(lr.small_x(c), dtype)


def compare(c, got, key="out", rows=None):
    want = lr.twin(c["name"])[key]
    assert_exact(rows_of(got, c["touched"] if rows is None else rows), want, f"{c['name']} {key}")


# ---- the SpMM ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", names("spmm", side="in"))
def test_matmul_raw_big_table(name):
    """the gathered table is big: fp32 at E31, bf16 at E32 (8 GiB each); an fp32 result of a few thousand rows.  Left to
    itself the plan decides the route, and at this size it must be one that forms its offsets in 64 bits; with slices of
    fewer than 32 768 columns forced it must be a group kernel's BIG variant (the slice base added in 64 bits)"""
    bf16 = lr.CASES[name]["dtype"] == "bf16"
    with case(name) as c:
        adj = c["adj"] = adjacency(c, **({"slices": c["slices"]} if "slices" in c else {}))
        c["kernel"] = adj.main_kernel(c["k"], dtype=TORCH[c["dtype"]])
        group, chunk = "group" in c["kernel"], c["kernel"].startswith("gcn::spmm_chunk_kernel<")
        if "slices" in c:
            assert adj.num_slices == c["slices"] and -(-c["n"] // c["slices"]) < 32768 and group, c["kernel"]
            assert ("bf16" in c["kernel"]) == bf16
        # (a group kernel's last template argument is BIG, a chunk kernel's is its buffer addressing)
        assert (group and c["kernel"].endswith("true>")) or (chunk and c["kernel"].endswith("false>")), c["kernel"]
        c["x"] = fill_table(c["R"], c["k"], TORCH[c["dtype"]], c["salt"])
        c["out"] = filled(c["m"], c["k"], torch.float32, float("nan"))
        adj.matmul_raw(c["x"], out=c["out"])
        compare(c, c["out"], rows=np.arange(c["m"]))
        assert bf16 == (c["x"].dtype == torch.bfloat16) and c["x"].numel() * c["x"].element_size() >= 4 * GIB


# the chunk family spmm_chunk_choice picks for a 512-wide unsliced call on a 3001-row table, by (tile_cols, gather_width):
# left to itself the plan takes 64-column tiles (the table sits in the Infinity Cache) and, the rows being short, the
# one-per-gather kernel with buffer addressing
FAMILY = {(0, 0): "gcn::spmm_chunk_kernel<1, 32, {e}, true>", (128, 0): "gcn::spmm_chunk_kernel<2, 8, {e}, false>",
          (256, 0): "gcn::spmm_chunk_kernel<4, 4, {e}, false>", (64, 4): "gcn::spmm_quad_kernel<16, {e}, false, false>"}


def run_spmm_out(c):
    """matmul_raw into a NaN-filled big result, on the route the case names, with its epilogue -> the result"""
    k, epi = c["k"], bool(c.get("epilogue"))
    adj = c["adj"] = adjacency(c, slices=c.get("slices", 0))
    if c.get("slices"):
        assert adj.num_slices == c["slices"]
        c["kernel"] = adj.main_kernel(k, epi, TORCH[c["dtype"]])
        assert "group" in c["kernel"], c["kernel"]
        # the slice reduction behind it is the wide one (k <= 256) and a plane of partial rows reaches 4 GiB: OFF32 = false
        assert c["R"] * k * 4 >= 2 ** 32 and k <= 256
    else:
        assert adj.num_slices == 0
        knobs = c.get("knobs", (0, 0))
        adj.set_tile_cols(knobs[0])
        adj.set_gather_width(knobs[1])
        c["kernel"] = adj.main_kernel(k, epi, TORCH[c["dtype"]])
        assert c["kernel"] == FAMILY[knobs].format(e="true" if epi else "false"), c["kernel"]
    c["x"] = small(c, TORCH[c["dtype"]])
    c["out"] = filled(c["R"], k, TORCH[c["dtype"]], float("nan"))
    kw = dict(bias=dev(lr.bias_of(c)), relu=True, dropout=lr.DROPOUT) if epi else {}
    adj.matmul_raw(c["x"], out=c["out"], **kw)
    return c["out"]


@pytest.mark.parametrize("name", names("spmm", side="out", epilogue=None))
def test_matmul_raw_big_result(name):
    """the result is big: one case per chunk family at E31 (the long rows of the top band span chunks: the fix-up writes
    there), one on two forced slices whose planes of partial rows pass 4 GiB (slice_reduce_wide_kernel with OFF32 = false),
    one with a bf16 result at E32"""
    with case(name) as c:
        out = run_spmm_out(c)
        assert outside_bad(out, c) == 0, "a row outside the bands is not zero"
        compare(c, out)


@pytest.mark.parametrize("name", names("spmm", side="out", epilogue=True))
def test_matmul_raw_big_result_epilogue(name):
    """bias + ReLU + dropout (p = 0.5: scale 2) into a big result, unsliced and on two forced slices: the mask is
    dropout_keep_at at every compared element; the empty rows of the bands hold dropout(relu(bias)), and every row outside
    the bands holds 0 or 2 relu(bias) in each element, about half of each"""
    with case(name) as c:
        out = run_spmm_out(c)
        twice = dev(2.0 * np.maximum(lr.bias_of(c), 0.0), out.dtype)
        assert outside_bad(out, c, 0, also=twice) == 0, "an element outside the bands is neither dropped nor 2 relu(bias)"
        compare(c, out)
        top = np.arange(c["R"] - lr.BAND, c["R"])
        empty = top[np.diff(c["rp"])[top] == 0]
        flat = empty[:, None] * c["k"] + np.arange(c["k"])[None, :]
        want = np.where(lr.keep_at(flat), 2.0 * np.maximum(lr.bias_of(c), 0.0)[None, :], 0.0)
        assert len(empty) >= 16
        assert_exact(rows_of(out, empty), want, f"{name}: empty rows of the top band")


@pytest.mark.parametrize("name", names("spmm_backward"))
def test_spmm_backward_big_gradient(name):
    """spmm(adj, x).backward: the gradient of x is [n, k] at E31, written by the transposed plan"""
    with case(name) as c:
        adj = c["adj"] = adjacency(c)
        c["x"] = torch.zeros((c["R"], c["k"]), dtype=torch.float32, device=DEV, requires_grad=True)
        y = gcn_amd.spmm(adj, c["x"])
        y.backward(small(c))
        c["gx"] = c["x"].grad
        c["kernel"] = adj.transpose().main_kernel(c["k"])
        assert c["gx"].shape == (c["R"], c["k"]) and outside_bad(c["gx"], c) == 0
        compare(c, c["gx"], "gx")
        c["x"].grad = None


@pytest.mark.parametrize("name", names("prelaid"))
def test_prelaid_table_past_4_gib(name):
    """rows of 8192 floats make a pre-laid table of 131 136 rows pass 4 GiB on a matrix of 6.5 M entries: the value-free BIG
    group kernel, once on the copy matmul_raw scales and re-lays itself and once on to_prelaid's table through
    matmul_prelaid with a gapped, scaled result; the zero row behind every slice is still zero afterwards.  Compared bit for
    bit on 48 rows x 256 columns (every row reads every band of the table)"""
    with case(name) as c:
        k, m, n, w = c["k"], c["m"], c["n"], c["w"]
        adj = c["adj"] = adjacency(c, slices=c["slices"])
        adj.set_value_factors(dev(c["u_row"]), dev(c["u_col"]))
        lay = adj.prelaid_layout(k)
        assert lay == dict(slices=c["slices"], slice_cols=w, table_rows=c["R"], ld=k) and c["R"] * k * 4 >= 2 ** 32
        c["kernel"] = adj.main_kernel(k)
        assert adj.has_value_factors and c["kernel"] == "gcn::spmm_group_ring_kernel<true>", c["kernel"]
        rows, cols = dev(c["check_rows"]), dev(c["check_cols"])
        want = lr.twin(name)
        c["B"] = fill_table(n, k, torch.float32, c["salt"])
        c["out"] = filled(m, k, torch.float32, float("nan"))
        adj.matmul_raw(c["B"], out=c["out"])
        assert not bool(torch.isnan(c["out"]).any())
        assert_exact(c["out"][rows][:, cols].double().cpu().numpy(), want["raw"], f"{name} matmul_raw")
        c["Bp"] = adj.to_prelaid(c["B"], dev(c["u_col"]))
        del c["B"]
        assert tuple(c["Bp"].shape) == (c["R"], k) and c["Bp"].numel() * 4 >= 2 ** 32
        gap = c["out_gap"]
        c["out"] = filled(m + (m - 1) // gap, k, torch.float32, float("nan"))
        adj.matmul_prelaid(c["Bp"], c["out"], out_scale=dev(c["out_scale"]), out_gap=gap)
        assert_exact(c["out"][rows + rows // gap][:, cols].double().cpu().numpy(), want["prelaid"], f"{name} matmul_prelaid")
        assert bool(torch.isnan(c["out"][gap::gap + 1]).all()), "a row behind a gap of the result was written"
        assert int(torch.isnan(c["out"]).sum()) == ((m - 1) // gap) * k
        assert float(c["Bp"][w::w + 1].abs().max()) == 0.0 and c["Bp"][w::w + 1].shape[0] == c["slices"]


# ---- SDDMM ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", names("sddmm"))
def test_sddmm_big_operand(name):
    """A big, then B big (fp32 at E31; bf16 B too: the entry point widens it to fp32 first)"""
    with case(name) as c:
        adj = c["adj"] = adjacency(c)
        big = fill_table(c["R"], c["k"], TORCH[c["dtype"]], c["salt"])
        c["A"], c["B"] = (big, small(c)) if c["side"] == "A" else (small(c), big)
        del big
        c["kernel"] = adj.sddmm_kernel(c["k"])
        got = adj.sddmm(c["A"], c["B"], out=filled(1, adj.nnz, torch.float32, float("nan")).view(-1))
        assert_exact(got.double().cpu().numpy(), lr.twin(name)["out"], name)


# ---- max / min aggregation ----------------------------------------------------------------------------------------------------------
def aggregate_into(adj, x, op, out, arg):
    """gcn_aggregate_csr into the caller's tensors (gcn_amd.aggregate allocates its own: a result could not start as NaN)"""
    ws = _scratch(adj, int(x.shape[1]), x.device)
    call("gcn_aggregate_csr", adj.rowptr, adj.col, adj.m, adj.n, adj.nnz, x, _DTYPE[x.dtype], int(x.shape[1]), _REDUCE[op],
         out, arg, ws, ws.numel() if ws is not None else 0, device=x.device)


@pytest.mark.parametrize("name", names("aggregate", side="in"))
def test_aggregate_big_table(name):
    with case(name) as c:
        adj = c["adj"] = adjacency(c)
        c["kernel"] = "gcn_aggregate_csr"
        c["x"] = fill_table(c["R"], c["k"], TORCH[c["dtype"]], c["salt"])
        out, arg = gcn_amd.aggregate(adj, c["x"], c["op"], return_arg=True)
        assert out.dtype == c["x"].dtype and arg.dtype == torch.int32
        compare(c, out, rows=np.arange(c["m"]))
        compare(c, arg, "arg", rows=np.arange(c["m"]))


@pytest.mark.parametrize("name", names("aggregate", side="out"))
def test_aggregate_big_result_and_arg(name):
    """the result and its int32 arg are big (bf16 at E32 puts arg at E32 too): both compared in every band, -1 on the empty
    rows of the top band; outside the bands the result is 0 and arg is -1"""
    with case(name) as c:
        adj = c["adj"] = adjacency(c)
        c["kernel"] = "gcn_aggregate_csr"
        c["x"] = small(c, TORCH[c["dtype"]])
        c["out"] = filled(c["R"], c["k"], TORCH[c["dtype"]], float("nan"))
        c["arg_t"] = filled(c["R"], c["k"], torch.int32, -2)
        aggregate_into(adj, c["x"], c["op"], c["out"], c["arg_t"])
        assert outside_bad(c["out"], c) == 0 and outside_bad(c["arg_t"], c, -1) == 0
        compare(c, c["out"])
        compare(c, c["arg_t"], "arg")
        top = np.arange(c["R"] - lr.BAND, c["R"])
        empty = top[np.diff(c["rp"])[top] == 0]
        assert len(empty) >= 16 and np.all(rows_of(c["arg_t"], empty) == -1)
        del c["out"], c["arg_t"]                          # once more through the binding, which allocates both itself
        c["out"], c["arg_t"] = gcn_amd.aggregate(adj, c["x"], c["op"], return_arg=True)
        assert c["out"].shape == c["arg_t"].shape == (c["R"], c["k"]) and c["arg_t"].dtype == torch.int32
        assert outside_bad(c["out"], c) == 0 and outside_bad(c["arg_t"], c, -1) == 0
        compare(c, c["out"])
        compare(c, c["arg_t"], "arg")


@pytest.mark.parametrize("name", names("aggregate_backward"))
def test_aggregate_backward_big_gradient(name):
    """gx [n, k] at E31 from gcn_aggregate_backward_csr: the rows of the bands receive gradient, the rest is exactly zero"""
    with case(name) as c:
        adj = c["adj"] = adjacency(c)
        c["kernel"] = "gcn_aggregate_backward_csr"
        g, k = small(c), c["k"]
        arg = dev(lr.backward_arg(c).astype(np.int32))
        c["gx"] = filled(c["R"], k, torch.float32, float("nan"))
        trowptr, trow, tperm = adj.tpattern()
        ws = _scratch(adj, k, DEV)
        call("gcn_aggregate_backward_csr", trowptr, trow, tperm, adj.n, adj.m, adj.nnz, g, _DTYPE[g.dtype], arg, k, c["gx"],
             ws, ws.numel() if ws is not None else 0, device=DEV)
        assert outside_bad(c["gx"], c) == 0
        compare(c, c["gx"], "gx")
        assert np.all(np.abs(lr.twin(name)["gx"]).sum(1) > 0)
        del c["gx"]                                       # once more through the autograd of aggregate(): x = feat, its arg is the twin's
        c["x"] = fill_table(c["R"], k, torch.float32, c["salt"]).requires_grad_(True)
        out, got_arg = gcn_amd.aggregate(adj, c["x"], c["op"], return_arg=True)
        assert torch.equal(got_arg, arg)
        out.backward(g)
        c["gx"] = c["x"].grad
        c["x"].grad = None
        del out
        assert c["gx"].shape == (c["R"], k) and outside_bad(c["gx"], c) == 0
        compare(c, c["gx"], "gx")


# ---- all heads in one pass: spmm_heads, sddmm_heads, gatv2_scores -----------------------------------------------------------------
def plain_adjacency(c):
    """(these units use no plan)"""
    return gcn_amd.CsrAdjacency(dev(c["rp"]), dev(c["ci"]), dev(c["va"]), (c["m"], c["n"]))


@pytest.mark.parametrize("name", names("spmm_heads"))
def test_spmm_heads_big(name):
    """x big (F = 64, and F = 63: no multiple of 4); then out big, written by gcn_spmm_heads_csr_f32 into a NaN-filled tensor"""
    with case(name) as c:
        adj = c["adj"] = plain_adjacency(c)
        c["kernel"], k, H = "gcn_spmm_heads_csr_f32", c["k"], c["heads"]
        vals = dev(lr.heads_vals(c))
        if c["side"] == "in":
            c["x"] = fill_table(c["R"], k, torch.float32, c["salt"])
            out = gcn_amd.spmm_heads(adj, c["x"], vals)
            compare(c, out, rows=np.arange(c["m"]))
        else:
            x = small(c)
            c["out"] = filled(c["R"], k, torch.float32, float("nan"))
            ws = _workspace(adj, adj.nnz, DEV, H, k)
            call("gcn_spmm_heads_csr_f32", adj.rowptr, adj.col, None, adj.m, adj.nnz, H, k, vals, x, c["out"], ws, ws.numel(), device=DEV)
            assert outside_bad(c["out"], c) == 0
            compare(c, c["out"])
            del c["out"]                                  # once more through the binding, which allocates the result itself
            c["out"] = gcn_amd.spmm_heads(adj, x, vals)
            assert c["out"].shape == (c["R"], k) and outside_bad(c["out"], c) == 0
            compare(c, c["out"])


@pytest.mark.parametrize("name", names("spmm_heads_backward"))
def test_spmm_heads_backward_big_gradient(name):
    """the gradient of x is [n, H F] at E31: the same kernel on the transposed pattern, the values through its permutation"""
    with case(name) as c:
        adj = c["adj"] = plain_adjacency(c)
        c["kernel"] = "gcn_spmm_heads_csr_f32"
        c["x"] = torch.zeros((c["R"], c["k"]), dtype=torch.float32, device=DEV, requires_grad=True)
        gcn_amd.spmm_heads(adj, c["x"], dev(lr.heads_vals(c))).backward(small(c))
        c["gx"] = c["x"].grad
        c["x"].grad = None
        assert c["gx"].shape == (c["R"], c["k"]) and outside_bad(c["gx"], c) == 0
        compare(c, c["gx"], "gx")


def score_operands(c, grad=False):
    """(a / h_dst [m, k], b / h_src [n, k]) of a score kernel: the big one filled from feat (and asking for its gradient)"""
    big = c["big"] = fill_table(c["R"], c["k"], torch.float32, c["salt"]).requires_grad_(grad)
    return (big, small(c)) if c["side"] == "A" else (small(c), big)


@pytest.mark.parametrize("name", names("sddmm_heads") + names("gatv2"))
def test_score_kernels_big_operand(name):
    """sddmm_heads and gatv2_scores with the row side big, then the column side (one of them with F = 63)"""
    with case(name) as c:
        adj = c["adj"] = plain_adjacency(c)
        a, b = score_operands(c)
        if c["unit"] == "sddmm_heads":
            c["kernel"] = "gcn_sddmm_heads_csr_f32"
            got = gcn_amd.sddmm_heads(adj, a, b, c["heads"])
        else:
            c["kernel"] = "gcn_gatv2_scores_csr_f32"
            got = gcn_amd.gatv2_scores(adj, a, b, dev(lr.att_of(c)), lr.SLOPE)
        del a, b
        assert got.shape == (adj.nnz, c["heads"])
        assert_exact(got.detach().double().cpu().numpy(), lr.twin(name)["out"], name)


@pytest.mark.parametrize("name", names("gatv2_backward"))
def test_gatv2_backward_big_gradient(name):
    """the gradient of h_src (the transposed walk) and of h_dst, [rows, H F] at E31 beside the operand itself"""
    with case(name) as c:
        adj = c["adj"] = plain_adjacency(c)
        c["kernel"] = "gcn_gatv2_scores_backward_csr_f32"
        a, b = score_operands(c, grad=True)
        gcn_amd.gatv2_scores(adj, a, b, dev(lr.att_of(c)), lr.SLOPE).backward(dev(lr.edge_grad(c)))
        c["grad"] = c["big"].grad
        c["big"].grad = None
        del a, b
        assert c["grad"].shape == (c["R"], c["k"]) and outside_bad(c["grad"], c) == 0
        compare(c, c["grad"], "grad")


# ---- the fused GAT edge softmax -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", names("gat_softmax"))
def test_gat_edge_softmax_big_operand(name):
    """a_dst, then a_src, [2^25 + 64, 64] (rows * H at E31), forward and backward: p on every entry with the bound of
    test_heads_gpu.check_forward, both gradients within the standing 1e-5 * sum|terms| + 1e-30 of that module against the
    fp64 twins, the big gradient compared in every band and exactly zero in every other row"""
    from test_heads_gpu import Graph, check_forward
    with case(name) as c:
        adj = c["adj"] = plain_adjacency(c)
        c["kernel"], H = "gcn_gat_edge_softmax_heads_csr_f32 / _backward", c["heads"]
        big = c["big"] = fill_table(c["R"], H, torch.float32, c["salt"]).mul_(0.5).requires_grad_(True)
        small_ = (small(c) * 0.5).requires_grad_(True)
        a_dst, a_src = (big, small_) if c["side"] == "A" else (small_, big)
        p = gcn_amd.gat_edge_softmax(adj, a_dst, a_src, lr.GAT_SLOPE)
        p.backward(dev(lr.edge_grad(c)))
        pn = p.detach().cpu().numpy()
        c["grad"], small_grad = big.grad, small_.grad.double().cpu().numpy()
        big.grad = None
        del a_dst, a_src, p
        ref = lr.softmax_reference(name, p=pn)
        check_forward(Graph(ref["rp"], ref["col"], ref["n"]), H, ref["s32"], pn, name)
        assert c["grad"].shape == (c["R"], H) and outside_bad(c["grad"], c) == 0
        key, other = ("gd", "gs") if c["side"] == "A" else ("gs", "gd")
        for what, got, want, mag in ((f"the big grad ({key})", rows_of(c["grad"], c["touched"]), ref[key], ref[key + "_mag"]),
                                     (f"the small grad ({other})", small_grad, ref[other], ref[other + "_mag"])):
            ratio = float((np.abs(got - want) / (1e-5 * mag + 1e-30)).max())
            print(f"[large] {name} {what}: max error / bound = {ratio:.4f}")
            assert got.shape == want.shape and ratio <= 1.0, (name, what, ratio)


# ---- kNN ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", names("knn"))
def test_knn_big_candidates(name):
    """y of n * d at E31 (d = 256): near neighbours planted in every band, every other row far away; indices (ascending by
    distance, ties by index) and distances equal knn_ref on the planted rows"""
    with case(name) as c:
        c["kernel"] = "gcn_knn_f32"
        planted = dev(c["touched"])
        y = c["y"] = filled(c["R"], c["k"], torch.float32, lr.FAR)
        y[planted] = lr.feat(planted[:, None], torch.arange(c["k"], device=DEV)[None, :], c["salt"]).float()
        idx, dist2 = gcn_amd.knn(dev(lr.knn_queries(c)), c["knn_k"], y=y)
        want = lr.twin(name)
        assert np.array_equal(idx.cpu().numpy().astype(np.int64), want["idx"]), "indices differ"
        assert_exact(dist2.double().cpu().numpy(), want["dist2"], name)
        assert (want["idx"] >= 2 ** 31 // c["k"]).sum() >= c["q"]      # (neighbours above the threshold are among them)


# ---- gather_rows, dropout_rows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", names("gather_rows"))
def test_gather_rows_big(name):
    """src at E31; then out at E31 with 2^22 + 64 indices"""
    with case(name) as c:
        c["kernel"] = "gcn_gather_rows_f32"
        idx = dev(c["idx"].astype(np.int32))
        if c["side"] == "in":
            c["src"] = fill_table(c["R"], c["k"], torch.float32, c["salt"])
            got = gcn_amd.gather_rows(c["src"], idx, out=filled(len(c["idx"]), c["k"], torch.float32, float("nan")))
            assert_exact(got.double().cpu().numpy(), lr.twin(name)["out"], name)
        else:
            src = small(c)
            c["out"] = filled(c["R"], c["k"], torch.float32, float("nan"))
            gcn_amd.gather_rows(src, idx, out=c["out"])
            compare(c, c["out"])
            bad = sum(int(torch.count_nonzero(c["out"][a:a + SCAN_ROWS] != src[idx[a:a + SCAN_ROWS].long()])) for a in range(0, c["R"], SCAN_ROWS))
            assert bad == 0, "a row of the result is not its source row"


@pytest.mark.parametrize("name", names("dropout_rows"))
def test_dropout_rows_big_in_place(name):
    """in place on more than 2^32 elements: dropout_keep_at around each threshold and at the end; everywhere else an element
    is its own value doubled or zero"""
    with case(name) as c:
        c["kernel"] = "gcn_dropout_" + ("f32" if c["dtype"] == "fp32" else "bf16")
        x = c["x"] = fill_table(c["R"], c["k"], TORCH[c["dtype"]], c["salt"])
        got = gcn_amd.dropout_rows(x, *lr.DROPOUT, out=x)
        assert got.data_ptr() == x.data_ptr() and x.numel() > 2 ** 32
        compare(c, x)
        flat, count = x.view(-1), x.numel()
        for at in (2 ** 31, 2 ** 32, count - 2048):      # 4096 flat indices around each threshold and the last 4096
            idx = np.arange(at - 2048, at + 2048, dtype=np.int64)
            want = np.where(lr.keep_at(idx), 2.0 * lr.feat(idx // c["k"], idx % c["k"], c["salt"]), 0.0)
            assert_exact(flat[at - 2048: at + 2048].double().cpu().numpy(), want, f"{name} around {at}")
        j = torch.arange(c["k"], device=DEV, dtype=torch.int64)[None, :]
        bad, kept, nonzero = (torch.zeros((), dtype=torch.int64, device=DEV) for _ in range(3))
        for lo in range(0, c["R"], FILL_ROWS):
            seg = x[lo:lo + FILL_ROWS]
            r = torch.arange(lo, lo + seg.shape[0], device=DEV, dtype=torch.int64)[:, None]
            twice = (2 * lr.feat(r, j, c["salt"])).to(seg.dtype)
            bad += torch.count_nonzero((seg != 0) & (seg != twice))
            kept += torch.count_nonzero((seg == twice) & (twice != 0))
            nonzero += torch.count_nonzero(twice)
        assert int(bad) == 0
        assert abs(int(kept) / int(nonzero) - 0.5) < 1e-3      # (4 . 10^9 draws at p = 0.5: the deviation is some 10^-5)
