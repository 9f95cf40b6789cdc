"""Seeded walks over an SpMM plan's reconfigurations on the GPU, every call exact: the walks of tests/stress_plan.py (their
coverage is proven without a GPU in tests/test_stress_plan_cpu.py).  All steps of a walk run in order ON ONE CsrAdjacency:
enable_slicing, enable_panels, set_value_factors, the three settings, prepare_width, update_values, autotune and their
refusals, with product calls between them — so a call meets whatever the calls before it left in the plan: a stream built
for another configuration, a workspace sized for another route, a plan half reset by a refused call.

After every reconfiguration the plan's own answers (num_slices, has_value_factors, panel_rows) must be the model's.  Before
every product call main_kernel, num_slices, has_value_factors, panel_rows and narrow_slices_for(k) are read and what
spmm_route guarantees whatever the history is asserted (_route_invariants); then the result, written into NaN, must EQUAL the
reference on every element (util.assert_exact; the one wide-range call per walk stays inside util.assert_elementwise), rows
without entries hold the epilogue of zero, and a second identical call returns the same bits.  References: the host oracle,
and for the `auto` family (4.5 M entries) an fp64 gather-sum on the device, exact for these operands.  Odd seeds run on a
side stream.  A failure prints the walk up to the failing step with the kernel name read at each call: a replayable recipe."""
import numpy as np
import pytest
import scipy.sparse as sp_
import torch

import gcn_amd
import stress_plan as sp
import util
from gcn_amd import _lib
from test_stress_plan_cpu import WALKS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PANEL_KERNEL = "gcn::spmm_panel_in_kernel"
_TRANSPOSED = {}


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _same_bits(a, b):
    view = torch.int32 if a.element_size() == 4 else torch.int16
    return torch.equal(a.view(view), b.view(view))


def _device_sum(rows, cols, vals, B, out_rows):
    """sum_e vals[e] * B[cols[e]] into row rows[e], in fp64 on the device, in pieces -> numpy fp64"""
    C = torch.zeros((out_rows, B.shape[1]), dtype=torch.float64, device=DEV)
    Bd = B.double()
    for i in range(0, len(rows), 1 << 18):
        C.index_add_(0, rows[i:i + (1 << 18)], vals[i:i + (1 << 18), None].double() * Bd[cols[i:i + (1 << 18)]])
    return C.cpu().numpy()


def _product(w, va, B, transposed=False, magnitude=False):
    """the raw sums A.B (A^T.B) of a call as fp64: the host oracle, on the device for the `auto` family"""
    o = w["ops"]
    if magnitude:
        va, B = np.abs(va), np.abs(B)
    if w["family"] == "auto":
        rows = _t(np.repeat(np.arange(o["m"]), np.diff(o["rp"])))
        cols = _t(o["ci"].astype(np.int64))
        return _device_sum(cols, rows, _t(va), _t(B), o["n"]) if transposed else _device_sum(rows, cols, _t(va), _t(B), o["m"])
    if not transposed:
        return util.oracle_spmm(o["rp"], o["ci"], va, B).astype(np.float64)
    key = (w["pattern"], hash(va.tobytes()) if w["mutable"] else None)
    if key not in _TRANSPOSED:
        At = sp_.csr_matrix((va.astype(np.float64), o["ci"], o["rp"]), shape=(o["m"], o["n"])).T.tocsr()
        _TRANSPOSED.clear()                              # (one at a time: a mutable walk makes a new one per value set)
        _TRANSPOSED[key] = (At.indptr.astype(np.int32), At.indices.astype(np.int32), At.data.astype(np.float32))
    return util.oracle_spmm(*_TRANSPOSED[key], B).astype(np.float64)


def _read(adj, s):
    dtype = torch.bfloat16 if s["dtype"] == "bf16" else torch.float32
    return dict(name=adj.main_kernel(s["k"], s["epi"] is not None, dtype), S=adj.num_slices, factors=adj.has_value_factors,
                panel_rows=adj.panel_rows, narrow=adj.narrow_slices_for(s["k"]))


def _route_invariants(r, s):
    """what spmm_route guarantees whatever the history (plan_policy.cpp)"""
    name, k = r["name"], s["k"]
    if s["dtype"] == "fp32":
        assert (name == PANEL_KERNEL) == (r["panel_rows"] > 0 and k > 32), (name, r)
    if name.startswith("gcn::spmm_group"):
        assert r["S"] > 0 and r["panel_rows"] == 0, (name, r)
        assert r["factors"] or "weighted" in name, (name, r)
    if s["kernel"] is not None:
        assert name == s["kernel"], (name, s["kernel"])


def _against_model(adj, want, what):
    if want is None:
        return
    got = dict(S=adj.num_slices, factors=adj.has_value_factors, panels=adj.panel_rows > 0)
    assert got == {k: want[k] for k in got}, f"{what}: the plan answers {got}, the model expects {want}"
    if not want["auto"]:
        assert adj.narrow_slices_for(16) == 0, f"{what}: a narrow slice set beside an explicit slice count"


def _settled(adj):
    return (adj.main_kernel(64), adj.main_kernel(16), adj.num_slices, adj.has_value_factors, adj.panel_rows, adj.narrow_slices_for(16))


def _reconf(adj, w, s):
    name, arg, o = s["name"], s["arg"], w["ops"]
    before = _settled(adj)

    def run():
        if name == "set_value_factors":
            if arg is None:
                adj.set_value_factors(None, None)
            elif arg == "doubled":
                u_row, u_col = sp.doubled_factors(w)
                adj.set_value_factors(_t(u_row), _t(u_col))
            elif o["u_row"] is None:                     # (a mutable plan refuses whatever the vectors hold)
                adj.set_value_factors(torch.ones(o["m"], device=DEV), torch.ones(o["n"], device=DEV))
            else:
                adj.set_value_factors(_t(o["u_row"]), _t(o["u_col"]))
        elif name == "update_values":
            adj.update_values(_t(util.int_values(len(o["ci"]), s["vseed"])))
        elif name == "autotune":
            adj.autotune(k=arg, reps=1)
        else:
            getattr(adj, name)(arg)

    if s["expect"] == "ok":
        run()
    else:
        with pytest.raises(_lib.GcnAmdError) as e:
            run()
        if arg == "doubled":
            assert e.value.status == _lib.ERR_NOT_FACTORED
        if s["expect"] == "refused":                     # a host-side argument check: nothing may have changed
            assert _settled(adj) == before, (before, _settled(adj))
        else:
            assert not adj.has_value_factors
    if (name, arg, s["expect"]) == ("enable_slicing", 0, "ok"):
        assert adj.num_slices == 0
    _against_model(adj, s["readings"], f"after {name}({arg!r})")


def _matmul(adj, w, s, va):
    o, k, m = w["ops"], s["k"], w["ops"]["m"]
    empty = np.diff(o["rp"]) == 0
    B = sp.features(s, o["n"])
    if s["kind"] == "wide":
        C1, C2 = (adj.matmul_raw(_t(B), out=_nan((m, k))) for _i in range(2))
        assert _same_bits(C1, C2), "a second identical call returns other bits"
        C = C1.cpu().numpy()
        util.assert_elementwise(C, _product(w, va, B), _product(w, va, B, magnitude=True), o["rp"], f"wide k={k}")
        assert np.all(C[empty] == 0.0)
        return
    bf16, out_dtype = s["dtype"] == "bf16", torch.bfloat16 if s["out"] == "bf16" else torch.float32
    Bd = _t(B, torch.bfloat16 if bf16 else None)
    assert not bf16 or torch.equal(Bd.float(), _t(B))
    bias, relu, drop = sp.epilogue_of(s)
    kw = dict(bias=None if bias is None else _t(bias), relu=relu, dropout=drop)
    C1, C2 = (adj.matmul_raw(Bd, out=_nan((m, k), out_dtype), **kw) for _i in range(2))
    assert C1.dtype == out_dtype and _same_bits(C1, C2), "a second identical call returns other bits"
    ref64, zero64 = sp.apply_epilogue(s, _product(w, va, B), m)
    ref, zero = ref64.astype(np.float32), zero64.astype(np.float32)
    assert np.array_equal(ref.astype(np.float64), ref64)             # an fp32 number: a bf16 result is rounded once, from it
    if s["out"] == "bf16":
        ref, zero = (torch.from_numpy(x).to(torch.bfloat16).float().numpy() for x in (ref, zero))
    C = C1.float().cpu().numpy()
    util.assert_exact(C, ref, f"{s['kind']} k={k}")
    assert np.array_equal(C[empty], zero[empty]), "a row without entries does not hold the epilogue of zero"


def _prelaid(adj, w, s, va):
    o, k, m, gap = w["ops"], s["k"], w["ops"]["m"], s["gap"]
    lay = adj.prelaid_layout(k)
    assert lay is not None, "the plan offers no pre-laid layout where the model knows it must"
    B = sp.features(s, o["n"])
    Bp = adj.to_prelaid(_t(B), _t(o["u_col"]))
    rows = m + (m - 1) // gap
    C1, C2 = (adj.matmul_prelaid(Bp, _nan((rows, k)), out_scale=_t(o["u_row"]), out_gap=gap) for _i in range(2))
    assert _same_bits(C1, C2), "a second identical call returns other bits"
    r = np.arange(m)
    C = C1.cpu().numpy()
    util.assert_exact(C[r + r // gap], (o["u_row"].astype(np.float64)[:, None] * _product(w, va, B)).astype(np.float32), f"prelaid k={k}")
    gaps = np.setdiff1d(np.arange(rows), r + r // gap)
    assert len(gaps) == (m - 1) // gap and np.isnan(C[gaps]).all(), "a gap row was written"


def _sddmm(adj, w, s):
    o, k = w["ops"], s["k"]
    A, B = util.int_features(o["m"], k, seed=s["bseed"]), util.int_features(o["n"], k, seed=s["bseed"] + 2)
    d1, d2 = (adj.sddmm(_t(A), _t(B), out=_nan((len(o["ci"]),))) for _i in range(2))
    assert _same_bits(d1, d2), "a second identical call returns other bits"
    ref, _mag = util.sddmm_ref(o["rp"], o["ci"], A, B, DEV)
    util.assert_exact(d1.cpu().numpy().astype(np.float64), ref, f"sddmm k={k}")


def _transpose(adj, w, s, va):
    o, k = w["ops"], s["k"]
    G = sp.features(s, o["m"])
    t = adj.transpose()
    C1, C2 = (t.matmul_raw(_t(G), out=_nan((o["n"], k))) for _i in range(2))
    assert _same_bits(C1, C2), "a second identical call returns other bits"
    util.assert_exact(C1.cpu().numpy(), _product(w, va, G, transposed=True).astype(np.float32), f"transpose k={k}")


def _backward(adj, w, s, va):
    """gcn_amd.spmm(adj, x, values=v): the forward re-lays v, x.grad = A(v)^T . G through the refreshed transpose,
    v.grad = SDDMM(G, x)"""
    o, k = w["ops"], s["k"]
    x = _t(sp.features(s, o["n"])).requires_grad_(True)
    v = _t(va).requires_grad_(True)
    G = util.int_features(o["m"], k, seed=s["bseed"] + 3)
    C = gcn_amd.spmm(adj, x, values=v)
    util.assert_exact(C.detach().cpu().numpy(), _product(w, va, sp.features(s, o["n"])).astype(np.float32), f"forward k={k}")
    assert _same_bits(C.detach(), adj.matmul_raw(x.detach(), out=_nan((o["m"], k)))), "a second identical call returns other bits"
    C.backward(_t(G))
    util.assert_exact(x.grad.cpu().numpy(), _product(w, va, G, transposed=True).astype(np.float32), "x.grad")
    ref, _mag = util.sddmm_ref(o["rp"], o["ci"], G, sp.features(s, o["n"]), DEV)
    util.assert_exact(v.grad.cpu().numpy().astype(np.float64), ref, "values.grad")


def _run(w):
    o = w["ops"]
    kw = dict(slices="auto" if w["family"] == "auto" else 0)
    if w["mutable"]:
        kw["mutable_values"] = True
    adj = gcn_amd.CsrAdjacency(_t(o["rp"]), _t(o["ci"]), _t(o["va"]), (o["m"], o["n"]), **kw)
    names = {}
    for i, s in enumerate(w["steps"]):
        try:
            if s["op"] == "reconf":
                _reconf(adj, w, s)
                continue
            _against_model(adj, s["readings"], "before the call")
            r = _read(adj, s)
            names[i] = r["name"]
            _route_invariants(r, s)
            va = sp.values_of(w, s["values"])
            if s["kind"] in ("spmm", "bf16", "wide"):
                _matmul(adj, w, s, va)
            elif s["kind"] == "prelaid":
                _prelaid(adj, w, s, va)
            elif s["kind"] == "sddmm":
                _sddmm(adj, w, s)
            elif s["kind"] == "transpose":
                _transpose(adj, w, s, va)
            else:
                _backward(adj, w, s, va)
            if s["builds_narrow"]:                       # the first narrow call of a value-free automatic plan built its set
                assert adj.narrow_slices_for(16) == sp.narrow_slices(o["m"], o["n"], len(o["ci"]), adj.num_slices) == 2
            _against_model(adj, s["readings"], "after the call")
        except Exception as e:
            raise AssertionError(f"{sp.describe(w, i, names)}\nstep {i} failed: {type(e).__name__}: {e}") from e


@pytest.mark.parametrize("family,seed", WALKS, ids=[f"{f}-{s}" for f, s in WALKS])
def test_walk(family, seed):
    w = sp.walk(seed, family)
    if w["side_stream"]:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _run(w)
        side.synchronize()
        torch.cuda.current_stream().wait_stream(side)
    else:
        _run(w)
        torch.cuda.synchronize()
