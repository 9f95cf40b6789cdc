"""Edge-feature aggregation with edge_feat and its gradient past 2^31 elements and 4 GiB: the one problem of
tests/edge_aggregate_large_ref.py (4.21 M entries, k = 512: 8 GiB each), filled on the device from formulas of (entry,
column) on the exact grid and compared bit for bit with the twin on the rows, columns and entries around entries 2^21 (byte
offset 2^32) and 2^22 (element 2^31), at both ends and at random places.  tests/test_edge_aggregate_cpu.py proves that an
offset computed in 32 bits, on the gather side or on the store side, changes what is compared here.  The memory guard and
the release in a ``finally`` are those of tests/test_large_operands_gpu.py; the case prints the route of the kernels, the
peak device memory and the wall time."""
import time

import numpy as np
import pytest
import torch

import edge_aggregate_large_ref as big
import gcn_amd
from gcn_amd import _lib, edgefeat
from gcn_amd._lib import call

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GIB = 1 << 30
NEED_GIB = 24                                            # edge_feat and its gradient (8.03 GiB each), out, arg and g (1 GiB each), fills
FILL = 1 << 15                                           # entries (rows) per chunk of a fill: int64 temporaries of 128 MiB


def _fill(rows, f):
    t = torch.empty((rows, big.K), dtype=torch.float32, device=DEV)
    j = torch.arange(big.K, device=DEV, dtype=torch.int64)[None, :]
    for lo in range(0, rows, FILL):
        r = torch.arange(lo, min(rows, lo + FILL), device=DEV, dtype=torch.int64)[:, None]
        t[lo:lo + FILL] = f(r, j)
    return t


def _rows(t, idx):
    return t.index_select(0, torch.from_numpy(idx).to(DEV)).cpu().numpy()


def test_edge_feat_and_its_gradient_past_2_31_elements():
    free = torch.cuda.mem_get_info(DEV)[0]
    if free < (NEED_GIB + 2) * GIB:
        pytest.skip(f"needs {NEED_GIB} GiB + 2 GiB of device memory, {free / GIB:.1f} GiB are free")
    rp = big.rowptr()
    m, nnz, n, k = len(rp) - 1, int(rp[-1]), big.N, big.K
    assert nnz > 2 ** 22 and nnz * k > 2 ** 31
    rows, cols, ents = big.compared_rows(rp), big.compared_cols(rp), big.compared_entries(rp)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    t0 = time.perf_counter()
    hold = {}
    try:
        col = big.col_of(torch.arange(nnz, device=DEV, dtype=torch.int64)).to(torch.int32)
        adj = hold["adj"] = gcn_amd.CsrAdjacency(torch.from_numpy(rp.astype(np.int32)).to(DEV), col, torch.ones(nnz, device=DEV), (m, n))
        x = hold["x"] = torch.from_numpy(big.x_table()).to(DEV)
        w = hold["w"] = _fill(nnz, big.w_of)
        g = hold["g"] = _fill(m, big.g_of).contiguous()
        assert w.numel() > 2 ** 31 and w.numel() * 4 > 2 ** 33
        out = hold["out"] = torch.full((m, k), float("nan"), device=DEV)
        arg = hold["arg"] = torch.full((m, k), -2, dtype=torch.int32, device=DEV)
        ws = edgefeat._scratch(adj, k, DEV)
        route = edgefeat.route(k, x, w, out)
        assert route == (4, 64, 2)

        def forward(op, act, reduce):
            call("gcn_edge_aggregate_csr_f32", adj.rowptr, adj.col, m, n, nnz, x, w, k, op, act, reduce, out, arg, ws, ws.numel(), device=DEV)

        forward(_lib.EDGE_OP_ADD, _lib.EDGE_ACT_RELU, _lib.REDUCE_SUM)
        want = big.forward_rows(rp, rows, "add", "relu", "sum")
        assert np.array_equal(_rows(out, rows).astype(np.float64), want), "sum"
        assert not bool(torch.isnan(out).any())
        forward(_lib.EDGE_OP_MUL, _lib.EDGE_ACT_NONE, _lib.REDUCE_MAX)
        want, want_arg = big.forward_rows(rp, rows, "mul", None, "max")
        assert np.array_equal(_rows(arg, rows).astype(np.int64), want_arg), "arg"
        assert np.array_equal(_rows(out, rows), want), "max"
        assert 0 <= int(arg.min()) and int(arg.max()) < nnz                 # (no row is empty)
        del hold["out"], hold["arg"], out, arg

        trowptr, trow, tperm = adj.tpattern()
        gx = hold["gx"] = torch.full((n, k), float("nan"), device=DEV)
        for op, act in (("add", "relu"), ("mul", None)):
            call("gcn_edge_aggregate_backward_x_csr_f32", trowptr, trow, tperm, n, m, nnz, g, x, w, k, edgefeat._OP[op], edgefeat._ACT[act],
                 gx, ws, ws.numel(), device=DEV)
            assert np.array_equal(_rows(gx, cols).astype(np.float64), big.grad_x_cols(rp, cols, op, act)), f"gx {op}/{act}"
            assert not bool(torch.isnan(gx).any())

        ge = hold["ge"] = torch.empty((nnz, k), dtype=torch.float32, device=DEV)
        ge.fill_(float("nan"))                               # a row that no store reaches keeps its NaN
        call("gcn_edge_aggregate_backward_e_csr_f32", adj.rowptr, adj.col, m, n, nnz, g, x, w, k, _lib.EDGE_OP_MUL, _lib.EDGE_ACT_RELU, ge,
             ws, ws.numel(), device=DEV)
        assert ge.numel() > 2 ** 31
        assert np.array_equal(_rows(ge, ents), big.grad_e_rows(rp, ents, "mul", "relu")), "ge"
        for lo in range(0, nnz, 1 << 19):                    # every row was written (reductions over row chunks)
            assert not bool(torch.isnan(ge[lo:lo + (1 << 19)]).any()), lo
        torch.cuda.synchronize()
    finally:
        wall = time.perf_counter() - t0
        peak = torch.cuda.max_memory_allocated(DEV) / GIB
        hold.clear()
        col = adj = x = w = g = out = arg = gx = ge = ws = trowptr = trow = tperm = None
        torch.cuda.empty_cache()
        print(f"\nLARGE edge_aggregate: kernels edge_message VEC=4 LPS=64, 2 column tiles (sum, max, grad x, grad e); "
              f"nnz {nnz}, k {k}; peak {peak:.2f} GiB; wall {wall:.2f} s")
