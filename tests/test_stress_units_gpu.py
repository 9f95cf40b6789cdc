"""Randomised sweep of the plan-free units on the GPU against their host twins: the cases of tests/stress_units.py (their
coverage and their power to discriminate are proven without a GPU in tests/test_stress_units_cpu.py).  For one seed a group
makes three steps in sequence ON THE SAME ADJACENCY OBJECTS, each with its own sub-shape, width, dtype, operand offsets and
stream, so that whatever a call leaves behind on the adjacency — the sampling workspace and vertex map, the aggregation
workspace and its retired buffers, the edge workspace, the cached transposes and twins — is met by a call of another shape.
Every comparison is a helper of the unit's own test module with its own bound; an assertion carries the seed, the group, the
step and the drawn parameters, and ``stress_units.case(seed, group)`` reproduces the inputs on the host.

Not here: the long kernel's second screening window (test_row_dispatch_gpu.py), tables past 4 GiB
(test_large_operands_gpu.py), rabbit_device."""
import contextlib

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gcn_amd
import stress_units as su
from coalesce_ref import (coalesce_ref, degree_ref, gcn_adjacency_ref, normalize_ref, symmetrize_ref, within_one_ulp)
from construct_ref import bucket_ref, csr_from_edges_ref, transpose_ref
from knn_ref import knn_ref
from sampling_ref import sample_blocks_ref, sample_neighbors_ref
from spgemm_ref import sorted_merged_ref, spgemm_ref
from subgraph_ref import induced_subgraph_ref, random_walk_ref
from test_aggregate_gpu import assert_select, assert_terms, bits, ref_backward
from test_attention_gpu import Rows, _ds_ref, _gat_backward_raw, _torch_scores, check_forward
from test_coalesce_gpu import check_coalesce, same_values
from test_construct_gpu import _raw_bucket, check_bucket
from test_knn_gpu import _guarded_outputs, check_against_twin, raw as knn_raw, same_bits, sums_agree
from test_sampling_gpu import _assert_blocks_equal_ref, _assert_sample
from test_spgemm_gpu import check_product
from test_stress_units_cpu import SEEDS
from test_subgraph_gpu import _assert_subgraph
from util import check_sddmm, guards_intact, offset_view

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


GROUPS = dict(construct=run_construct, coalesce=run_coalesce, sampling=run_sampling, aggregate=run_aggregate,
              attention=run_attention, sddmm=run_sddmm, spgemm=run_spgemm, knn=run_knn)
assert tuple(GROUPS) == su.UNITS


@pytest.mark.parametrize("seed", range(SEEDS))
@pytest.mark.parametrize("group", su.UNITS)
def test_three_steps_on_one_adjacency(group, seed):
    GROUPS[group](su.case(seed, group))
