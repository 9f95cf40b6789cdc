"""Randomised sweep of the plan-free units on the GPU against their host twins: the cases of tests/stress_units.py (their
coverage and their power to discriminate are proven without a GPU in tests/test_stress_units_cpu.py).  For one seed a group
makes three steps in sequence ON THE SAME ADJACENCY OBJECTS, each with its own sub-shape, width, dtype, operand offsets and
stream, so that whatever a call leaves behind on the adjacency — the sampling workspace and vertex map, the aggregation
workspace and its retired buffers, the edge workspace, the cached transposes and twins — is met by a call of another shape.
Every comparison is a helper of the unit's own test module with its own bound; an assertion carries the seed, the group, the
step and the drawn parameters, and ``stress_units.case(seed, group)`` reproduces the inputs on the host.

The groups added later go through the public functions AND their autograd, the path that uses the adjacency's own Scratch
keeper (kinds edge, gatv2, aggregate, edge_aggregate, sample) and its one cached ``tpattern()``: heads (the head-batched
softmax family within test_heads_gpu's bounds, spmm_heads / sddmm_heads and their gradients bit for bit, H changing between
the steps), gatv2 (scores and all four gradients bit for bit), edge_aggregate (every op, act and reduce, both gradients),
sampled_dot (both modes and SparseProduct.values with its backward, bit for bit against sampled_dot_ref), linkpred
(find_edges and negative_sample interleaved, integer for integer) and mixed: three DIFFERENT units in turn on one square,
mutable adjacency, with new values between steps 1 and 2 on one seed in two.  No tolerance is this module's own: every
bound is imported from the unit's test module, every exact comparison asserts first that its fp64 reference is on the fp32
grid.

Not here: the long kernel's second screening window (test_row_dispatch_gpu.py), tables past 4 GiB
(test_large_operands_gpu.py), rabbit_device."""
import contextlib

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import edge_aggregate_ref as ea
import gatv2_ref
import gcn_amd
import heads_ref
import stress_units as su
from coalesce_ref import (coalesce_ref, degree_ref, gcn_adjacency_ref, normalize_ref, symmetrize_ref, within_one_ulp)
from construct_ref import bucket_ref, csr_from_edges_ref, transpose_ref
from knn_ref import knn_ref
from linkpred_ref import find_entries_ref, negative_sample_ref
from sampled_dot_ref import sampled_dot_ref
from sampling_ref import sample_blocks_ref, sample_neighbors_ref
from spgemm_ref import sorted_merged_ref, spgemm_ref, transpose_ref as transpose_values_ref
from subgraph_ref import induced_subgraph_ref, random_walk_ref
from test_aggregate_gpu import assert_select, assert_terms, bits, ref_backward
from test_attention_gpu import Rows, _ds_ref, _gat_backward_raw, _torch_scores, check_forward
from test_coalesce_gpu import check_coalesce, same_values
from test_construct_gpu import _raw_bucket, check_bucket
from test_edge_aggregate_gpu import assert_close as ea_close, assert_exact as ea_exact
from test_gatv2_gpu import on_grid
from test_heads_gpu import (Graph as HeadsGraph, assert_rows_close, check_forward as heads_forward, ds_bound, raw_gat_backward)
from test_knn_gpu import _guarded_outputs, check_against_twin, raw as knn_raw, same_bits, sums_agree
from test_linkpred_gpu import _same as same_entries
from test_sampled_dot_gpu import same_values as same_dot_values
from test_sampling_gpu import _assert_blocks_equal_ref, _assert_sample
from test_spgemm_gpu import check_product
from test_stress_units_cpu import SEEDS
from test_subgraph_gpu import _assert_subgraph
from util import assert_exact, check_sddmm, guards_intact, offset_view

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FLOAT = {"fp32": torch.float32, "bf16": torch.bfloat16}
INDEX = {"int32": torch.int32, "int64": torch.int64}


class Operands:
    """device operands `off` elements past a 16-byte boundary, between guards that are checked when the step is over"""

    def __init__(self):
        self.guards = []

    def __call__(self, a, off, dtype):
        view, flat = offset_view(a, off, dtype, DEV)
        self.guards.append((flat, view))
        return view

    def index(self, a, off, name):
        """ids as int32 at an offset, or as int64 (which the guarded buffers do not hold) as they come"""
        if name == "int64":
            return torch.from_numpy(np.ascontiguousarray(a, np.int64)).to(DEV)
        return self(np.ascontiguousarray(a, np.int32), off, torch.int32)

    def adjacency(self, rp, ci, va, shape, offs, **kw):
        return gcn_amd.CsrAdjacency(self(rp, offs[0], torch.int32), self(ci, offs[1], torch.int32), self(va, offs[2], torch.float32),
                                    shape, **kw)

    def check(self):
        assert all(guards_intact(flat, view) for flat, view in self.guards), "a guard element around an operand was written"


@contextlib.contextmanager
def step(c, i, ops):
    """runs one step on the default stream or on a side stream, checks the guards after it and puts (seed, group, step, drawn
    parameters) in front of whatever it asserts"""
    what = su.describe(c, i)
    try:
        if c["steps"][i]["side_stream"]:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                yield what
            side.synchronize()
            torch.cuda.current_stream().wait_stream(side)
        else:
            yield what
            torch.cuda.synchronize()
        ops.check()
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from e


def same_ints(got, want, name):
    got = got.cpu().numpy()
    assert got.shape == np.shape(want) and np.array_equal(got, want), f"{name} differs"


# ---- the groups ---------------------------------------------------------------------------------------------------------------
def run_construct(c):
    ops = Operands()
    for i, s in enumerate(c["steps"]):
        with step(c, i, ops) as what:
            o, n = s["offsets"], c["n"]
            mm = s["rows"][1] - s["rows"][0]
            e_rows, e_cols, e_vals = su.edge_list(c, i)
            if s["op"] == "bucket_by_key":
                ref_off, ref_perm = bucket_ref(e_rows, mm)
                if s["raw"] and len(e_rows):
                    keys, perm = ops(e_rows.astype(np.int32), o[0], torch.int32), ops(len(e_rows), o[1], torch.int32)
                    same_ints(_raw_bucket(keys, mm, perm), ref_off, "offsets")
                    same_ints(perm, ref_perm, "perm")
                else:
                    check_bucket(e_rows, mm, INDEX[s["dtype"]])
            elif s["op"] == "csr_from_edges":
                adj, eid = gcn_amd.csr_from_edges(ops.index(e_rows, o[0], s["dtype"]), ops.index(e_cols, o[1], "int32"), (mm, n),
                                                  ops(e_vals, o[2], torch.float32), s["sort_columns"])
                rrp, rci, rva, reid = csr_from_edges_ref(e_rows, e_cols, (mm, n), e_vals, s["sort_columns"])
                assert (adj.m, adj.n, adj.nnz) == (mm, n, len(e_rows)) and eid.dtype == torch.int32
                same_ints(adj.rowptr, rrp, "rowptr"), same_ints(adj.col, rci, "col"), same_ints(eid, reid, "eid")
                assert np.array_equal(adj.val.cpu().numpy().view(np.int32), rva.view(np.int32)), "values are not carried"
            else:                                           # the transpose of the transpose: its buckets are the drawn rows
                trp, trow, tva = su.transpose_host(*su.step_matrix(c, i), n)
                adj = ops.adjacency(trp, trow, tva, (n, mm), o)
                t, eid = gcn_amd.transpose_csr(adj)
                rrp, rrow, rval, reid = transpose_ref(trp, trow, tva, mm)
                assert (t.m, t.n, t.nnz, t.symmetric) == (mm, n, len(trow), False) and eid.dtype == torch.int32
                same_ints(t.rowptr, rrp, "rowptr"), same_ints(t.col, rrow, "row"), same_ints(eid, reid, "eid")
                assert np.array_equal(t.val.cpu().numpy().view(np.int32), rval.view(np.int32)), "values are not carried"


def run_coalesce(c):
    ops = Operands()
    for i, s in enumerate(c["steps"]):
        with step(c, i, ops) as what:
            o, n = s["offsets"], c["n"]
            mm = s["rows"][1] - s["rows"][0]
            if s["op"] == "coalesce_csr":                   # check_coalesce, then the same call on operands off the grid
                rp, ci, va = su.step_matrix(c, i)
                ref = coalesce_ref(rp, ci, va, n, s["reduce"], s["diagonal"], s["diag_value"])
                check_coalesce(rp, ci, va, mm, n, s["reduce"], s["diagonal"], s["diag_value"], assume_sorted=True, ref=ref)
                out, seg = gcn_amd.coalesce_csr(ops.adjacency(rp, ci, va, (mm, n), o), s["reduce"], s["diagonal"], s["diag_value"],
                                                assume_sorted=True)
                same_ints(out.rowptr, ref[0], "rowptr"), same_ints(out.col, ref[1], "col"), same_ints(seg, ref[4], "seg")
                assert same_values(out.val.cpu().numpy(), ref[2]), "values differ"
            elif s["op"] == "symmetrize":
                rp, ci, va = su.square_part(c, i)
                merged, _ = gcn_amd.coalesce_csr(ops.adjacency(rp, ci, va, (mm, mm), o), "sum", assume_sorted=True)
                got = gcn_amd.symmetrize(merged, s["reduce"])
                ref = symmetrize_ref(*coalesce_ref(rp, ci, va, mm, "sum")[:3], s["reduce"])
                same_ints(got.rowptr, ref[0], "rowptr"), same_ints(got.col, ref[1], "col")
                assert same_values(got.val.cpu().numpy(), ref[2]), "values differ"
            elif s["op"] == "normalize_csr":
                rp, ci, va = su.square_part(c, i)
                va = np.abs(va)                             # positive terms, as in test_degree_and_normalize
                adj = gcn_amd.normalize_csr(ops.adjacency(rp, ci, va, (mm, mm), o, symmetric=False), s["norm"])
                ref = normalize_ref(rp, ci, va, degree_ref(rp, va), s["norm"])
                got = adj.val.cpu().numpy()
                assert np.all(np.isfinite(got)) and np.all(within_one_ulp(got, ref)), "normalised values differ"
            else:
                e_rows, e_cols, e_vals = su.edge_list(c, i, square=True)
                kw = dict(reduce=s["reduce"] if s["reduce"] != "first" else "max", self_loops=s["diagonal"], norm=s["norm"])
                out = gcn_amd.gcn_adjacency(ops.index(e_rows, o[0], s["dtype"]), ops.index(e_cols, o[1], "int32"), mm,
                                            values=ops(e_vals, o[2], torch.float32), **kw)
                ref = gcn_adjacency_ref(e_rows, e_cols, mm, values=e_vals, **kw)
                same_ints(out.rowptr, ref[0], "rowptr"), same_ints(out.col, ref[1], "col")
                assert np.all(within_one_ulp(out.val.cpu().numpy(), ref[2].astype(np.float64))), "normalised values differ"


def run_sampling(c):
    ops = Operands()
    rp, ci, va, n = c["rp"], c["ci"], c["va"], c["n"]
    adj = ops.adjacency(rp, ci, va, (n, n), c["adj_offsets"])          # one adjacency: sample.hip and subgraph.hip share its map
    for i, s in enumerate(c["steps"]):
        with step(c, i, ops) as what:
            seed, offset = s["philox"]
            ids = ops.index(s["ids"], s["offsets"][0], s["dtype"])
            if s["op"] == "sample_neighbors":
                got = gcn_amd.sample_neighbors(adj, ids, s["fanout"], seed=seed, offset=offset)
                _assert_sample(got, sample_neighbors_ref(rp, ci, s["ids"], s["fanout"], seed, offset), what)
            elif s["op"] == "sample_blocks":
                blocks, input_ids = gcn_amd.sample_blocks(adj, ids, s["fanouts"], seed=seed, offset=offset)
                _assert_blocks_equal_ref(blocks, input_ids, *sample_blocks_ref(rp, ci, va, s["ids"], s["fanouts"], seed, offset))
            elif s["op"] == "induced_subgraph":
                sub = gcn_amd.induced_subgraph(adj, ids)
                _assert_subgraph(sub, induced_subgraph_ref(rp, ci, s["ids"], n), s["ids"], va, what)
            else:
                got = gcn_amd.random_walk(adj, ids, s["length"], seed=seed, offset=offset)
                assert got.dtype == torch.int32 and got.shape == (len(s["ids"]), s["length"] + 1)
                same_ints(got, random_walk_ref(rp, ci, s["ids"], s["length"], seed, offset), "walks")
            vmap = getattr(adj, "_sample_map", None)
            assert vmap is None or bool((vmap == -1).all()), "the shared vertex map is not clear after the step"


def run_aggregate(c):
    ops = Operands()
    rp, ci, m, n = c["rp"], c["ci"], c["m"], c["n"]
    adj = ops.adjacency(rp, ci, c["va"], (m, n), c["adj_offsets"], mutable_values=c["mutable"])   # one: its workspace grows
    lens = np.diff(rp)
    for i, s in enumerate(c["steps"]):
        with step(c, i, ops) as what:
            dt, o = FLOAT[s["dtype"]], s["offsets"]
            xd = ops(s["x"], o[0], dt).requires_grad_(True)
            ref_out, ref_arg = su.select_host(rp, ci, s["x"], s["op"])                  # (integers in [-2, 2]: exact in bf16)
            out, arg = gcn_amd.aggregate(adj, xd, s["op"], return_arg=True)
            assert out.dtype == dt and out.shape == arg.shape == (m, s["k"])
            assert_select(out, arg, ref_out if dt == torch.float32 else torch.from_numpy(ref_out).to(dt), ref_arg, what)
            (gx,) = torch.autograd.grad(out, xd, ops(s["g"], o[1], dt))
            ref = ref_backward(ci, n, ref_arg, s["g"])
            assert ref_backward(ci, n, ref_arg, np.abs(s["g"])).max(initial=0) < 2 ** 24    # every fp32 sum is exact in any order
            if dt == torch.float32:
                assert np.array_equal(gx.cpu().numpy().astype(np.float64), ref), "the gradient differs"
            else:                                           # ... and rounded to bf16 once, at the store
                assert np.array_equal(bits(gx), bits(torch.from_numpy(ref).to(dt))), "the gradient differs"
            if s["linear"] is not None:
                val = np.ones(len(ci), np.float32) if s["linear"] == "sum" else \
                    np.repeat(np.float32(1.0) / np.maximum(lens, 1).astype(np.float32), lens)
                A = sp.csr_matrix((val.astype(np.float64), ci.astype(np.int64), rp.astype(np.int64)), shape=(m, n))
                got = gcn_amd.aggregate(adj, ops(s["x"], o[2], torch.float32), s["linear"])
                assert_terms(got, torch.from_numpy(A @ s["x"].astype(np.float64)), torch.from_numpy(A @ np.abs(s["x"]).astype(np.float64)),
                             what)
                assert bool((got[torch.from_numpy(lens == 0).to(DEV)] == 0).all())


def run_attention(c):
    ops = Operands()
    rp, ci, m, n = c["rp"], c["ci"], c["m"], c["n"]
    adj = ops.adjacency(rp, ci, c["va"], (m, n), c["adj_offsets"], mutable_values=True)
    R = Rows(rp)
    for i, s in enumerate(c["steps"]):
        with step(c, i, ops) as what:
            o = s["offsets"]
            if s["op"] == "edge_softmax":
                sd = ops(s["scores"], o[0], torch.float32).requires_grad_(True)
                p = gcn_amd.edge_softmax(adj, sd)
                check_forward(R, s["scores"], p.detach().cpu().numpy(), what)
                (ds,) = torch.autograd.grad(p, sd, ops(s["g"], o[1], torch.float32))
                ds_ref, bound = _ds_ref(R, p.detach().cpu().numpy(), s["g"])
                ratio = float((np.abs(ds.cpu().numpy() - ds_ref) / bound).max())
                assert ratio <= 1.0, f"backward: {ratio} of the bound"
            elif s["op"] == "gat_edge_softmax":
                slope = s["slope"]
                a_dst = ops(s["a_dst"], o[0], torch.float32).requires_grad_(True)
                a_src = ops(s["a_src"], o[1], torch.float32).requires_grad_(True)
                g = ops(s["g"], o[2], torch.float32)
                p = gcn_amd.gat_edge_softmax(adj, a_dst, a_src, slope)
                if slope <= 1.0:                            # (check_forward's bound is stated for a score range <= 16)
                    s32 = _torch_scores(adj, R, a_dst.detach(), a_src.detach(), slope)
                    check_forward(R, s32.cpu().numpy(), p.detach().cpu().numpy(), what)
                gd, gs = torch.autograd.grad(p, (a_dst, a_src), g)
                ds, gd_raw = _gat_backward_raw(adj, a_dst.detach(), a_src.detach(), slope, p.detach(), g)
                assert torch.equal(gd_raw, gd)
                pre = s["a_dst"].astype(np.float64)[R.row] + s["a_src"].astype(np.float64)[ci]
                ds_ref, bound = _ds_ref(R, p.detach().cpu().numpy(), s["g"], np.where(pre > 0, 1.0, slope))
                ratio = float((np.abs(ds.cpu().numpy() - ds_ref) / (bound * max(1.0, slope))).max())
                assert ratio <= 1.0, f"fused backward: {ratio} of the bound"
                gd_ref, gd_mag = R.full(R.rsum(ds_ref)), R.full(R.rsum(np.abs(ds_ref)))
                gs_ref, gs_mag = np.bincount(ci, weights=ds_ref, minlength=n), np.bincount(ci, weights=np.abs(ds_ref), minlength=n)
                r_dst = float((np.abs(gd.cpu().numpy() - gd_ref) / (1e-5 * gd_mag + 1e-30)).max())
                r_src = float((np.abs(gs.cpu().numpy() - gs_ref) / (1e-5 * gs_mag + 1e-30)).max())
                assert r_dst <= 1.0 and r_src <= 1.0, f"grad_a_dst {r_dst}, grad_a_src {r_src} of their bounds"
            else:                                           # row sums of a stretch of the rows, through a permutation or not
                lo, hi = s["rows"]
                b, e = int(rp[lo]), int(rp[hi])
                sub, x = (rp[lo:hi + 1] - rp[lo]).astype(np.int32), s["scores"][b:e]
                perm = np.argsort(s["perm"][b:e]).astype(np.int32) if s["perm"] is not None else None
                got = gcn_amd.segment_sum(ops(sub, o[0], torch.int32), ops(x, o[1], torch.float32),
                                          perm=ops(perm, o[2], torch.int32) if perm is not None else None)
                Rs, xs = Rows(sub), x.astype(np.float64) if perm is None else x.astype(np.float64)[perm]
                ref, mag = Rs.full(Rs.rsum(xs)), Rs.full(Rs.rsum(np.abs(xs)))
                ratio = float((np.abs(got.cpu().numpy() - ref) / (1e-5 * mag + 1e-30)).max())
                assert ratio <= 1.0, f"segment sum: {ratio} of the bound"


def run_sddmm(c):
    ops = Operands()
    rp, ci, va, m, n = c["rp"], c["ci"], c["va"], c["m"], c["n"]
    drawn = ops.adjacency(rp, ci, va, (m, n), c["adj_offsets"], **c["plan"])
    unsliced = ops.adjacency(rp, ci, va, (m, n), (0, 0, 0), slices=0)
    for i, s in enumerate(c["steps"]):
        with step(c, i, ops) as what:
            dt, o = FLOAT[s["dtype"]], s["offsets"]
            A, B = ops(s["A"], o[0], dt), ops(s["B"], o[1], dt)                        # (integers in [-8, 8]: exact in bf16)
            out = drawn.sddmm(A, B)
            assert out.dtype == torch.float32
            check_sddmm(out, *su.sddmm_host(rp, ci, s["A"], s["B"]))
            assert torch.equal(out, unsliced.sddmm(A, B)), "the bits differ from the unsliced plan's"


def run_spgemm(c):
    ops = Operands()
    p, n = c["p"], c["n"]
    b_dup = ops.adjacency(c["d_rp"], c["d_ci"], c["d_va"], (p, n), c["adj_offsets"])
    merged = sorted_merged_ref(c["d_rp"], c["d_ci"], c["d_va"])
    for i, s in enumerate(c["steps"]):
        with step(c, i, ops) as what:
            rp, ci, va = su.step_matrix(c, i)
            if s["op"] == "raw":
                a = (rp, ci, None if s["pattern"] == "a" else va)
                b = (c["b_rp"], c["b_ci"], None if s["pattern"] == "b" else c["b_va"])
                check_product(a, b, p, n)
            else:                                           # B repeats (row, column) pairs: spgemm merges it first
                got = gcn_amd.spgemm(ops.adjacency(rp, ci, va, (len(rp) - 1, p), s["offsets"]), b_dup)
                ref = spgemm_ref(rp, ci, va, *merged, p, n)
                same_ints(got.rowptr, ref[0], "rowptr"), same_ints(got.col, ref[1], "col")
                assert same_values(got.val.cpu().numpy(), ref[2]), "values differ"


def run_knn(c):
    ops = Operands()
    for i, s in enumerate(c["steps"]):
        with step(c, i, ops) as what:
            x, y, k, q, n, d, o = s["x"], s["y"], s["knn_k"], s["q"], s["n"], s["d"], s["offsets"]
            if s["op"] == "raw":
                check_against_twin(x, y, k, s["self_offset"], s["splits"], what)
                continue
            xp, yp = np.full((q, s["ldx"]), 99.0, np.float32), np.full((n, s["ldy"]), -99.0, np.float32)
            xp[:, :d], yp[:, :d] = x, y                     # row strides of d and more; the padding would change every distance
            xv, yv = ops(xp, o[0], torch.float32), ops(yp, o[1], torch.float32)
            ridx, rd2, rsum = knn_ref(x, y, k, s["self_offset"])
            if s["op"] == "knn":
                kw = dict(exclude_self=True, self_offset=s["self_offset"]) if s["self_offset"] >= 0 else {}
                idx, d2 = gcn_amd.knn(xv[:, :d], k, y=yv[:, :d], splits=s["splits"], **kw)
                assert np.array_equal(idx.cpu().numpy(), ridx) and same_bits(d2.cpu().numpy(), rd2)
            else:
                out, guards = _guarded_outputs(q, k)
                idx, d2, sums = knn_raw(xv, yv, k, s["self_offset"], s["splits"], ldx=s["ldx"], ldy=s["ldy"], d=d, out=out)
                assert np.array_equal(idx, ridx) and same_bits(d2, rd2) and sums_agree(sums, rsum, n)
                assert all(guards_intact(flat, view) for flat, view in guards)


# ---- the later units: one function per step kind (the mixed group runs them too), every one through the public function and
# its autograd — the path that uses the adjacency's own scratch and its one cached transposed pattern -------------------------------
F32 = torch.float32


def exact(got, ref, name):
    """bit for bit against an fp64 reference, which must lie on the fp32 grid (test_gatv2_gpu.on_grid asserts it)"""
    assert tuple(got.shape) == ref.shape and torch.equal(got, torch.from_numpy(on_grid(ref)).to(DEV)), f"{name} differs"


def within(got, ref, bound, name):
    ratio = float((np.abs(got.detach().cpu().numpy() - ref) / bound).max()) if ref.size else 0.0
    assert ratio <= 1.0, f"{name}: {ratio} of the bound"


def step_spmm_heads(ops, adj, c, i, x, what):
    s, rp, ci, n = c["steps"][i], c["rp"], c["ci"], c["n"]
    o, H = s["offsets"], s["H"]
    xd, vd = ops(x["x"], o[0], F32).requires_grad_(True), ops(x["vals"], o[1], F32).requires_grad_(True)
    out = gcn_amd.spmm_heads(adj, xd, vd)
    gx, gv = torch.autograd.grad(out, (xd, vd), ops(x["g"], o[2], F32))    # x: the walk of the transposed pattern; values: sddmm_heads
    trp, trow, tperm = heads_ref.transpose_pattern(rp, ci, n)
    exact(out, heads_ref.spmm_heads(rp, ci, None, x["vals"], x["x"], H), "spmm_heads")
    exact(gx, heads_ref.spmm_heads(trp, trow, tperm, x["vals"], x["g"], H), "the gradient in x")
    exact(gv, heads_ref.sddmm_heads(rp, ci, x["g"], x["x"], H), "the gradient in the values")


def step_sddmm_heads(ops, adj, c, i, x, what):
    s, rp, ci, n = c["steps"][i], c["rp"], c["ci"], c["n"]
    o, H = s["offsets"], s["H"]
    ad, bd = ops(x["a"], o[0], F32).requires_grad_(True), ops(x["b"], o[1], F32).requires_grad_(True)
    sd = gcn_amd.sddmm_heads(adj, ad, bd, H)
    ga, gb = torch.autograd.grad(sd, (ad, bd), ops(x["g"], o[2], F32))
    trp, trow, tperm = heads_ref.transpose_pattern(rp, ci, n)
    exact(sd, heads_ref.sddmm_heads(rp, ci, x["a"], x["b"], H), "sddmm_heads")
    exact(ga, heads_ref.spmm_heads(rp, ci, None, x["g"], x["b"], H), "the gradient in a")
    exact(gb, heads_ref.spmm_heads(trp, trow, tperm, x["g"], x["a"], H), "the gradient in b")


def step_edge_softmax(ops, adj, c, i, x, what):
    s, rp, ci, n = c["steps"][i], c["rp"], c["ci"], c["n"]
    o, H, G = s["offsets"], s["H"], HeadsGraph(rp, ci, n)
    sd = ops(x["scores"], o[0], F32).requires_grad_(True)
    p = gcn_amd.edge_softmax(adj, sd)
    assert p.shape == (len(ci), H)
    (ds,) = torch.autograd.grad(p, sd, ops(x["g"], o[1], F32))
    pn = p.detach().cpu().numpy()
    heads_forward(G, H, x["scores"], pn, what)
    within(ds, heads_ref.edge_softmax_backward(rp, pn, x["g"]), ds_bound(G, H, pn, x["g"]), "backward")


def step_gat_edge_softmax(ops, adj, c, i, x, what):
    """as test_heads_gpu.test_gat_edge_softmax_heads_forward_and_backward_match_fp64"""
    s, rp, ci, n = c["steps"][i], c["rp"], c["ci"], c["n"]
    o, H, slope, G = s["offsets"], s["H"], s["slope"], HeadsGraph(rp, ci, n)
    a_dst, a_src = ops(x["a_dst"], o[0], F32).requires_grad_(True), ops(x["a_src"], o[1], F32).requires_grad_(True)
    g = ops(x["g"], o[2], F32)
    p = gcn_amd.gat_edge_softmax(adj, a_dst, a_src, slope)
    gd, gs = torch.autograd.grad(p, (a_dst, a_src), g)
    pn = p.detach().cpu().numpy()
    # (a_dst, a_src in [-4, 4): a row's pre-activations span at most 8, its scores at most 12 at slope 1.5 — inside the range
    # of 16 that check_forward's bound is stated for, which check_forward asserts)
    heads_forward(G, H, heads_ref.gat_scores(rp, ci, x["a_dst"], x["a_src"], slope), pn, what)
    ds, gd_raw = raw_gat_backward(adj, a_dst.detach(), a_src.detach(), slope, p.detach(), g)
    assert torch.equal(gd_raw, gd)
    ds_ref, gd_ref = heads_ref.gat_edge_softmax_backward(rp, ci, x["a_dst"], x["a_src"], slope, pn, x["g"])
    within(ds, ds_ref, ds_bound(G, H, pn, x["g"]) * max(1.0, slope), "fused backward")
    assert_rows_close(G, gd, gd_ref, heads_ref.row_sums(rp, np.abs(ds_ref)), what + " grad_a_dst")
    trp, _trow, tperm = heads_ref.transpose_pattern(rp, ci, n)
    within(gs, heads_ref.segment_sum(trp, ds_ref, tperm), 1e-5 * heads_ref.segment_sum(trp, np.abs(ds_ref), tperm) + 1e-30, "grad_a_src")


def step_segment_sum(ops, adj, c, i, x, what):
    """row sums of a stretch of the rows, through a permutation or not (no adjacency: the scratch is the stream's)"""
    o = c["steps"][i]["offsets"]
    sub, xs, perm = su.segment_operands(c, i, x)
    got = gcn_amd.segment_sum(ops(sub, o[0], torch.int32), ops(xs, o[1], F32), perm=ops(perm, o[2], torch.int32) if perm is not None else None)
    G, x64 = HeadsGraph(sub, np.zeros(len(xs), np.int32), 1), xs.astype(np.float64)
    assert_rows_close(G, got, heads_ref.segment_sum(sub, x64, perm), heads_ref.segment_sum(sub, np.abs(x64), perm), what)


def step_gatv2_scores(ops, adj, c, i, x, what):
    s, rp, ci, n = c["steps"][i], c["rp"], c["ci"], c["n"]
    o, slope = s["offsets"], s["slope"]
    hd, hs, att = (ops(x[name], o[j], F32).requires_grad_(True) for j, name in enumerate(("hd", "hs", "att")))
    sc = gcn_amd.gatv2_scores(adj, hd, hs, att, slope)
    gd, gs, ga = torch.autograd.grad(sc, (hd, hs, att), ops(x["g"], o[3], F32))
    args = (x["hd"], x["hs"], x["att"], slope)
    ref_gd, ref_gs, _act, ref_ga = gatv2_ref.backward(rp, ci, n, *args, x["g"])
    exact(sc, gatv2_ref.scores(rp, ci, *args), "scores")
    exact(gd, ref_gd, "grad_h_dst"), exact(gs, ref_gs, "grad_h_src"), exact(ga, ref_ga, "grad_att")


def step_edge_aggregate(ops, adj, c, i, x, what):
    """test_edge_aggregate_gpu.check_case(exact=True) on operands off the grid; the mean as its own test has it: the sum
    divided once, and the gradients of the sum's kernels on g / len"""
    s, rp, ci, n = c["steps"][i], c["rp"].astype(np.int64), c["ci"], c["n"]
    o, msg, act, reduce = s["offsets"], s["msg"], s["act"], s["reduce"]
    select = reduce in ("max", "min")
    xt, wt = ops(x["x"], o[0], F32).requires_grad_(True), ops(x["w"], o[1], F32).requires_grad_(True)
    res = gcn_amd.edge_aggregate(adj, xt, wt, msg, act, reduce, return_arg=select)
    out, arg = res if select else (res, None)
    gx, ge = torch.autograd.grad(out, (xt, wt), ops(x["g"], o[2], F32))
    as_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    if select:
        want, want_arg = ea.forward(rp, ci, x["x"], x["w"], msg, act, reduce)
        assert torch.equal(arg, as_dev(want_arg.astype(np.int32))), what + " arg"
        ea_exact(None, out, want, what + " out")
        want_gx, _mag, want_ge = ea.backward_select(rp, ci, n, x["x"], x["w"], x["g"], want_arg, msg, act)
        ea_exact(None, gx, want_gx, what + " gx")
    else:
        want, _mag = ea.forward(rp, ci, x["x"], x["w"], msg, act, "sum")
        lens = np.maximum(np.diff(rp), 1)[:, None].astype(np.float32) if reduce == "mean" else np.float32(1)
        g = (x["g"] / lens).astype(np.float32)          # (the mean's autograd divides the gradient once, as IEEE does here)
        want_gx, mag_gx, want_ge = ea.backward_sum(rp, ci, n, x["x"], x["w"], g, msg, act)
        if reduce == "sum":
            ea_exact(None, out, want, what + " out"), ea_exact(None, gx, want_gx, what + " gx")
        else:
            assert torch.equal(out, as_dev(on_grid(want) / lens)), what + " out"
            ea_close(gx, want_gx, mag_gx, what + " gx")
            xs, ws = xt.detach().requires_grad_(True), wt.detach().requires_grad_(True)
            sgx, sge = torch.autograd.grad(gcn_amd.edge_aggregate(adj, xs, ws, msg, act, "sum"), (xs, ws), ops(g, o[3], F32))
            assert torch.equal(gx, sgx) and torch.equal(ge, sge), what + ": the mean's gradients are not the sum's on g / len"
    assert torch.equal(ge, as_dev(want_ge)), what + " ge"  # one product rounded once: the twin's bits


def step_aggregate(ops, adj, c, i, x, what):
    """the fp32 step of run_aggregate"""
    s, rp, ci, n = c["steps"][i], c["rp"], c["ci"], c["n"]
    o = s["offsets"]
    xd = ops(x["x"], o[0], F32).requires_grad_(True)
    ref_out, ref_arg = su.select_host(rp, ci, x["x"], s["select"])
    out, arg = gcn_amd.aggregate(adj, xd, s["select"], return_arg=True)
    assert_select(out, arg, ref_out, ref_arg, what)
    (gx,) = torch.autograd.grad(out, xd, ops(x["g"], o[1], F32))
    assert np.array_equal(gx.cpu().numpy().astype(np.float64), ref_backward(ci, n, ref_arg, x["g"])), "the gradient differs"


def step_sample_neighbors(ops, adj, c, i, x, what):
    s = c["steps"][i]
    seed, offset = s["philox"]
    ids = ops.index(s["ids"], s["offsets"][0], ("int32", "int64")[(c["seed"] + i) & 1])
    got = gcn_amd.sample_neighbors(adj, ids, s["fanout"], seed=seed, offset=offset)
    _assert_sample(got, sample_neighbors_ref(c["rp"], c["ci"], s["ids"], s["fanout"], seed, offset), what)


STEP_KINDS = dict(spmm_heads=step_spmm_heads, sddmm_heads=step_sddmm_heads, edge_softmax=step_edge_softmax,
                  gat_edge_softmax=step_gat_edge_softmax, segment_sum=step_segment_sum, gatv2_scores=step_gatv2_scores,
                  edge_aggregate=step_edge_aggregate, aggregate=step_aggregate, sample_neighbors=step_sample_neighbors)


def run_on_one_adjacency(c, mutable=True):
    """heads, gatv2, edge_aggregate: the three steps on ONE adjacency — one Scratch keeper, one cached tpattern()"""
    ops = Operands()
    adj = ops.adjacency(c["rp"], c["ci"], c["va"], (c["m"], c["n"]), c["adj_offsets"], mutable_values=mutable)
    for i, s in enumerate(c["steps"]):
        with step(c, i, ops) as what:
            STEP_KINDS[s["kind"]](ops, adj, c, i, su.step_inputs(c, i), what)
    return adj


def run_mixed(c):
    """three different units in turn on one square, mutable adjacency; new values between steps 1 and 2 on one seed in two:
    the pattern's cached transpose stays, the mutable transpose and a plain SpMM's backward carry the new values"""
    ops = Operands()
    rp, ci, n = c["rp"], c["ci"], c["n"]
    adj = ops.adjacency(rp, ci, c["va"], (n, n), c["adj_offsets"], mutable_values=True)
    trp, trow, tperm = heads_ref.transpose_pattern(rp, ci, n)
    for i, s in enumerate(c["steps"]):
        with step(c, i, ops) as what:
            if i == 2 and c["update"]:
                cached = adj.tpattern()
                assert np.array_equal(bits(adj.transpose().val), bits(c["va"][tperm])), "the transpose's values before the update"
                adj.update_values(ops(c["new_va"], s["offsets"][5], F32))
                assert all(a is b for a, b in zip(adj.tpattern(), cached)), "the cached transposed pattern was rebuilt"
                same_ints(cached[0], trp, "trowptr"), same_ints(cached[1], trow, "trow"), same_ints(cached[2], tperm, "tperm")
                assert np.array_equal(bits(adj.val), bits(c["new_va"])) and np.array_equal(bits(adj.transpose().val), bits(c["new_va"][tperm]))
                xs = np.random.default_rng(c["seed"]).integers(-3, 4, (n, 4)).astype(np.float32)     # eighths x integers: exact
                xd = ops(xs, 0, F32).requires_grad_(True)
                y = gcn_amd.spmm(adj, xd)
                (gxs,) = torch.autograd.grad(y, xd, ops(xs[::-1].copy(), 0, F32))
                A = sp.csr_matrix((c["new_va"].astype(np.float64), ci.astype(np.int64), rp.astype(np.int64)), shape=(n, n))
                assert_exact(y.detach().cpu().numpy(), A @ xs.astype(np.float64), "spmm on the new values")
                assert_exact(gxs.cpu().numpy(), A.T @ xs[::-1].astype(np.float64), "its backward through the transpose")
            STEP_KINDS[s["kind"]](ops, adj, c, i, su.step_inputs(c, i), what)


def run_linkpred(c):
    ops = Operands()
    rp, ci, m, n = c["rp"], c["ci"], c["m"], c["n"]
    adj = ops.adjacency(rp, ci, c["va"], (m, n), c["adj_offsets"])
    for i, s in enumerate(c["steps"]):
        with step(c, i, ops) as what:
            x, o = su.step_inputs(c, i), s["offsets"]
            rows = ops.index(x["q_rows"], o[0], s["dtype"])
            if s["op"] == "find_edges":
                got = gcn_amd.find_edges(adj, rows, ops.index(x["q_cols"], o[1], s["dtype"]))
                same_entries(got, find_entries_ref(rp, ci, x["q_rows"], x["q_cols"]), what)
            else:
                seed, offset = s["philox"]
                got = gcn_amd.negative_sample(adj, rows, s["num_neg"], seed, offset, s["max_tries"], s["exclude_self"])
                same_entries(got, negative_sample_ref(rp, ci, n, x["q_rows"], s["num_neg"], seed, offset, s["max_tries"], s["exclude_self"]), what)


def run_sampled_dot(c):
    ops = Operands()
    q, w, o3 = c["m"], c["w"], c["adj_offsets"]
    P = ops.adjacency(c["rp"], c["ci"], c["va"], (q, q), o3)
    X = ops.adjacency(c["x_rp"], c["x_ci"], c["x_va"], (q, w), o3[1:] + o3[:1])
    Y = ops.adjacency(c["y_rp"], c["y_ci"], c["y_va"], (q, w), o3[2:] + o3[:2])
    for i, s in enumerate(c["steps"]):
        with step(c, i, ops) as what:
            o = s["offsets"]
            p, np_cols, x, y, width, by_col = su.dot_operands(c, i)
            want = sampled_dot_ref(p[0], p[1], np_cols, *x, *y, width, x_by_col=by_col)
            if s["op"] != "product":
                given = lambda adj, mode, v, off: adj if mode == "own" else (adj, ops(v, off, F32) if mode == "given" else None)
                got = gcn_amd.sampled_dot(P, given(X, s["x_mode"], s["xv"], o[0]), given(Y, s["y_mode"], s["yv"], o[1]), x_by_col=by_col)
                assert got.shape == (len(c["ci"]),) and same_dot_values(got.cpu().numpy(), want), "the sampled product differs"
                continue
            # C = A · B with A = X's first rows (cut to 65 entries) and B = Yᵀ; values and both gradients, each the kernel again
            pr, ra = c["prod"], c["prod"]["ra"]
            order = np.argsort(c["y_ci"], kind="stable")                                 # B's entry t is Y's entry order[t]
            a, yv = (pr["a_rp"], pr["a_ci"], x[2]), y[2]
            b = transpose_values_ref(c["y_rp"], c["y_ci"], yv, w)
            SP = gcn_amd.SparseProduct(ops.adjacency(*a[:2], pr["a_va"], (ra, w), o[:3]), ops.adjacency(b[0], b[1], c["y_va"][order], (w, q), o[3:]))
            same_ints(SP.adj.rowptr, pr["c_rp"], "the product's rowptr"), same_ints(SP.adj.col, pr["c_ci"], "the product's columns")
            av = ops(a[2], o[0], F32).requires_grad_(True) if s["x_mode"] == "given" else None
            bv = ops(b[2], o[1], F32).requires_grad_(True) if s["y_mode"] == "given" else None
            got = SP.values(av, bv)
            assert same_dot_values(got.detach().cpu().numpy(), want), "SparseProduct.values differs"
            leaves = [t for t in (av, bv) if t is not None]
            if leaves:
                grads = dict(zip([id(t) for t in leaves], torch.autograd.grad(got, leaves, ops(s["g"], o[2], F32))))
                cc = (pr["c_rp"], pr["c_ci"], s["g"])
                if av is not None:                      # on A's pattern: X = (B, b_values), Y = (C, grad), x_by_col
                    ga = sampled_dot_ref(a[0], a[1], w, *b, *cc, q, x_by_col=True)
                    assert same_dot_values(grads[id(av)].cpu().numpy(), ga), "the gradient in a_values differs"
                if bv is not None:                      # on B's pattern: X = Aᵀ, Y = Cᵀ
                    gb = sampled_dot_ref(b[0], b[1], q, *transpose_values_ref(*a, w), *transpose_values_ref(*cc, q), ra)
                    assert same_dot_values(grads[id(bv)].cpu().numpy(), gb), "the gradient in b_values differs"


GROUPS = dict(construct=run_construct, coalesce=run_coalesce, sampling=run_sampling, aggregate=run_aggregate,
              attention=run_attention, sddmm=run_sddmm, spgemm=run_spgemm, knn=run_knn, heads=run_on_one_adjacency,
              gatv2=run_on_one_adjacency, edge_aggregate=run_on_one_adjacency, sampled_dot=run_sampled_dot, linkpred=run_linkpred,
              mixed=run_mixed)
assert tuple(GROUPS) == su.UNITS


@pytest.mark.parametrize("seed", range(SEEDS))
@pytest.mark.parametrize("group", su.UNITS)
def test_three_steps_on_one_adjacency(group, seed):
    GROUPS[group](su.case(seed, group))
