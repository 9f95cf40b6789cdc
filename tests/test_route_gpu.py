"""The route table: what every report of the plan API answers, and what the fp32 / bf16 SpMM computes, over a set of plans
that reaches every family of the dispatch (plan_policy.cpp, spmm_route) — recorded once from the commit named in
tests/golden/route_table.json and required to be EQUAL here, strings and digests alike (no kernel of these paths uses
floating-point atomics, so the same launches give the same bits).

record(name) builds one configuration and returns its records; the golden file holds them packed (pack / unpack below:
every report as runs along the widths, the three digests of a width as one).
"""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import gcn_amd
from gcn_amd import _lib
from util import GOLDEN, arrays_sha256, banded_csr, exact_operands, random_csr, sym_norm_graph

pytestmark = pytest.mark.gpu
TABLE = os.path.join(GOLDEN, "route_table.json")
SWITCHES = ("GCN_AMD_GROUP8", "GCN_AMD_GROUP12", "GCN_AMD_GROUP_BIG")
REPORT_WIDTHS = tuple(range(1, 73)) + (96, 100, 128, 130, 172, 256, 260)
DIGEST_WIDTHS = (8, 16, 17, 20, 32, 36, 41, 44, 47, 48, 52, 64, 100, 128, 130, 256)
BF16_WIDTHS = (64, 72, 128)
DROPOUT = (0.5, 0x5EED, 3)
BF16 = torch.bfloat16


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _adj(g, m, n, **kw):
    d = _dev()
    return gcn_amd.CsrAdjacency(torch.from_numpy(g[0]).to(d), torch.from_numpy(g[1]).to(d), torch.from_numpy(g[2]).to(d),
                                (m, n), **kw)


_GRAPHS = {}


def _graph(name):
    if name not in _GRAPHS:
        if name == "short":                                  # ~40 entries per row
            _GRAPHS[name] = random_csr(2048, 2048, 2048 * 40, seed=31)
        elif name == "norm":                                 # the smallest the automatic rule slices
            _GRAPHS[name] = sym_norm_graph(17000, 1200000, seed=21)
        elif name == "dense_small":                          # ~90 entries per column at n = 2 048
            _GRAPHS[name] = sym_norm_graph(2048, 100000, seed=32)
        elif name == "wide":                                 # slices wider than the 15-bit stream, 3 entries per column
            _GRAPHS[name] = random_csr(3000, 140000, 400000, seed=7, long_rows=[(11, 30000)])
        elif name == "banded":
            _GRAPHS[name] = banded_csr(3001, 150, 3, seed=5, hub=(777, 2600))
        elif name == "mid":
            _GRAPHS[name] = sym_norm_graph(6000, 260000, seed=3)
    return _GRAPHS[name]


def _a():
    return _adj(_graph("short"), 2048, 2048, slices=0)


def _gather(width):
    def make():
        adj = _a()
        adj.set_gather_width(width)
        return adj
    return make


def _tile(cols):
    """one non-zero per gather on a 128- / 256-column tile: the 2- and 4-float-per-lane chunk kernels"""
    def make():
        adj = _gather(1)()
        adj.set_tile_cols(cols)
        return adj
    return make


def _c():
    adj = _adj(_graph("norm"), 17000, 17000)
    adj.prepare_width(16)                                # (one slice of 128-byte rows fits an L2: no narrow set to build)
    assert adj.narrow_slices_for(16) == 0
    return adj


def _reddit_half():
    """Reddit-shaped at half size: the smallest graph of the suite whose plan has a narrow slice set (8 -> 4 slices)"""
    if "reddit_half" not in _GRAPHS:
        from gcn_amd import graphgen
        rowptr, col, val, n = graphgen.make_graph("reddit", device=_dev(), seed=1, scale=0.5)
        _GRAPHS["reddit_half"] = (rowptr, col, val, n, arrays_sha256(rowptr.cpu().numpy(), col.cpu().numpy(), val.cpu().numpy()))
    return _GRAPHS["reddit_half"]


def _narrow(prepared):
    def make():
        rowptr, col, val, n, _ = _reddit_half()
        adj = gcn_amd.CsrAdjacency(rowptr, col, val, (n, n), symmetric=True)
        assert adj.num_slices == 8 and adj.narrow_slices_for(16) == 0
        if prepared:
            adj.prepare_width(16)
            assert adj.narrow_slices_for(16) == 4
        return adj
    return make


def _d():
    rp, ci, va = _graph("norm")
    va = va.copy()
    va[len(va) // 2] *= 1.0001
    return _adj((rp, ci, va), 17000, 17000)


def _f16():
    ops = exact_operands("col16", "pow2")
    adj = _adj((ops["rp"], ops["ci"], ops["va"]), ops["m"], ops["n"], slices=2)
    adj.set_value_factors(torch.from_numpy(ops["u_row"]), torch.from_numpy(ops["u_col"]))
    adj.set_gather_width(4)                              # (short virtual rows: force the four-per-gather layout)
    return adj


def _f():
    adj = _adj(_graph("wide"), 3000, 140000, slices=4)
    adj.set_gather_width(4)
    return adj


def _empty():
    return _adj((np.zeros(2049, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)), 2048, 2048)


def _no_rows():
    return _adj((np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)), 0, 64)


def _is(prefixes, weighted=None):
    def check(adj, k=128):
        name = adj.main_kernel(k)
        assert name.startswith(tuple("gcn::" + p for p in prefixes)), name
        assert weighted is None or ("weighted" in name) == weighted, name
    return check


def _unsliced(adj):
    assert adj.num_slices == 0 and adj.panel_rows == 0
    _is(("spmm_chunk_kernel", "spmm_quad_kernel"))(adj)


def _narrow_4_and_8(adj):
    _unsliced(adj)
    assert adj.main_kernel(3) == "gcn::spmm_narrow_kernel<4, 4, false, true>", adj.main_kernel(3)
    assert adj.main_kernel(7) == "gcn::spmm_narrow_kernel<8, 8, false, true>", adj.main_kernel(7)


def _chunk_tile(vec, u, k):
    def check(adj):
        assert adj.num_slices == 0 and adj.panel_rows == 0
        assert adj.main_kernel(k) == f"gcn::spmm_chunk_kernel<{vec}, {u}, false, false>", adj.main_kernel(k)
    return check


def _group_free(adj):
    assert adj.num_slices >= 2 and adj.has_value_factors
    _is(("spmm_group",), weighted=False)(adj)


def _group_weighted(adj):
    assert adj.num_slices >= 2 and not adj.has_value_factors
    _is(("spmm_group",), weighted=True)(adj)


def _own_set_only(adj):
    _group_free(adj)
    assert adj.num_slices == 4
    adj.prepare_width(16)
    assert adj.narrow_slices_for(16) == 0


def _sliced_quad(adj):
    assert adj.num_slices == 4
    assert adj.main_kernel(128).startswith("gcn::spmm_quad_kernel<16, false, false,"), adj.main_kernel(128)


def _sliced_quad_col16(adj):
    assert adj.num_slices == 2 and adj.has_value_factors
    assert adj.main_kernel(128) == "gcn::spmm_quad_kernel<16, false, true, true>"


def _panels(adj):
    assert adj.panel_rows > 0
    assert adj.main_kernel(128) == "gcn::spmm_panel_in_kernel"


def _mutable(adj):
    assert adj.values_mutable
    _group_weighted(adj)


def _nothing(adj):
    assert adj.nnz == 0 and adj.num_slices == 0


NO_NARROW_CALL = tuple(k for k in DIGEST_WIDTHS if k > 32)     # (a call at k <= 32 would build the narrow set)

# name -> (builder, the family the configuration is named for, fp32 and bf16 widths whose results are recorded)
CONFIGS = {
    "a_unsliced": (_a, _unsliced, DIGEST_WIDTHS),
    "b_gather1": (_gather(1), lambda adj: _is(("spmm_chunk_kernel",))(adj), DIGEST_WIDTHS),
    "b_gather4": (_gather(4), lambda adj: _is(("spmm_quad_kernel",))(adj), DIGEST_WIDTHS),
    "c_auto_sliced": (_c, _group_free, DIGEST_WIDTHS),
    "c_narrow_set_absent": (_narrow(False), _group_free, NO_NARROW_CALL, (72, 128)),
    "c_narrow_set_present": (_narrow(True), _group_free, DIGEST_WIDTHS),
    "d_perturbed": (_d, _group_weighted, DIGEST_WIDTHS),
    "e_forced_slices": (lambda: _adj(_graph("dense_small"), 2048, 2048, slices=4), _own_set_only, DIGEST_WIDTHS),
    "f_sliced_quad": (_f, _sliced_quad, DIGEST_WIDTHS),
    "f_sliced_quad_col16": (_f16, _sliced_quad_col16, (16, 41, 64, 100)),
    "g_panels": (lambda: _adj(_graph("banded"), 3001, 3001, panels=1), _panels, DIGEST_WIDTHS),
    "h_mutable": (lambda: _adj(_graph("mid"), 6000, 6000, slices=3, mutable_values=True), _mutable, DIGEST_WIDTHS),
    "i_empty": (_empty, _nothing, DIGEST_WIDTHS),
    "i_no_rows": (_no_rows, _nothing, DIGEST_WIDTHS),
    # (recorded at meta.commit_chunk_walk: widths below 8 and the 128- / 256-column tiles, which the rows above do not call)
    "j_unsliced_narrow": (_a, _narrow_4_and_8, (1, 2, 3, 4, 5, 7), ()),
    "k_gather1_tile128": (_tile(128), _chunk_tile(2, 8, 128), (128, 130, 256), ()),
    "l_gather1_tile256": (_tile(256), _chunk_tile(4, 4, 256), (256, 260), ()),
}


def _prelaid(adj, k):
    """prelaid_layout(k), or the status gcn_spmm_plan_prelaid_layout refuses with"""
    lay = adj.prelaid_layout(k)
    if lay is not None:
        return lay
    return dict(status=int(_lib.load().gcn_spmm_plan_prelaid_layout(adj.plan, int(k), None, None, None, None)))


def meta():
    return dict(cu_count=int(_lib.load().gcn_device_cu_count()), switches={s: os.environ.get(s) for s in SWITCHES},
                reddit_half_sha256=_reddit_half()[4])


def _digests(adj, k, dtype, features, bias):
    B = features[:, :k].to(dtype).contiguous()
    b = bias[:k].contiguous()
    return dict(plain=arrays_sha256(adj.matmul_raw(B).view(torch.int16 if dtype == BF16 else torch.int32).cpu().numpy()),
                bias_relu=arrays_sha256(adj.matmul_raw(B, bias=b, relu=True).view(
                    torch.int16 if dtype == BF16 else torch.int32).cpu().numpy()),
                bias_relu_dropout=arrays_sha256(adj.matmul_raw(B, bias=b, relu=True, dropout=DROPOUT).view(
                    torch.int16 if dtype == BF16 else torch.int32).cpu().numpy()))


def record(name):
    make, family, widths, bf16_widths = (CONFIGS[name] + (BF16_WIDTHS,))[:4]
    with torch.cuda.device(_dev()):
        adj = make()
        family(adj)
        reports = []
        for k in REPORT_WIDTHS:
            reports.append(dict(k=k, main_kernel=adj.main_kernel(k), main_kernel_epilogue=adj.main_kernel(k, epilogue=True),
                                main_kernel_bf16=adj.main_kernel(k, dtype=BF16), num_passes=adj.num_passes(k),
                                narrow_slices_for=adj.narrow_slices_for(k), sddmm_kernel=adj.sddmm_kernel(k),
                                prelaid_layout=_prelaid(adj, k)))
        rng = np.random.default_rng(77)
        features = torch.from_numpy(rng.standard_normal((adj.n, max(DIGEST_WIDTHS))).astype(np.float32)).to(_dev())
        bias = torch.from_numpy(rng.standard_normal(max(DIGEST_WIDTHS)).astype(np.float32)).to(_dev())
        extra = max(widths + bf16_widths + (0,)) - max(DIGEST_WIDTHS)
        if extra > 0:                                    # columns past the widest of DIGEST_WIDTHS: a stream of their own
            more = np.random.default_rng(78)
            features = torch.cat([features, torch.from_numpy(more.standard_normal((adj.n, extra)).astype(np.float32)).to(_dev())], 1)
            bias = torch.cat([bias, torch.from_numpy(more.standard_normal(extra).astype(np.float32)).to(_dev())])
        results = {f"f32_{k}": _digests(adj, k, torch.float32, features, bias) for k in widths}
        results.update({f"bf16_{k}": _digests(adj, k, BF16, features, bias) for k in bf16_widths})
        after = [dict(k=k, main_kernel=adj.main_kernel(k), narrow_slices_for=adj.narrow_slices_for(k)) for k in (16, 32, 64)]
        torch.cuda.synchronize()
    return dict(reports=reports, results=results, reports_after_the_calls=after)


REPORT_FIELDS = ("main_kernel", "main_kernel_epilogue", "main_kernel_bf16", "num_passes", "narrow_slices_for", "sddmm_kernel",
                 "prelaid_layout")


def pack(rec):
    """reports: per field the runs [first width, value] along REPORT_WIDTHS; results: sha256 over a width's three digests"""
    runs = {}
    for f in REPORT_FIELDS:
        runs[f] = []
        for r in rec["reports"]:
            if not runs[f] or runs[f][-1][1] != r[f]:
                runs[f].append([r["k"], r[f]])
    one = lambda d: hashlib.sha256((d["plain"] + d["bias_relu"] + d["bias_relu_dropout"]).encode()).hexdigest()
    return dict(reports=runs, results={key: one(d) for key, d in rec["results"].items()},
                reports_after_the_calls=rec["reports_after_the_calls"])


def unpack_reports(runs):
    """the reports of pack() as one record per width again"""
    reports = [dict(k=k) for k in REPORT_WIDTHS]
    for f in REPORT_FIELDS:
        starts = {k: v for k, v in runs[f]}
        assert runs[f][0][0] == REPORT_WIDTHS[0] and set(starts) <= set(REPORT_WIDTHS), f
        for r in reports:
            if r["k"] in starts:
                value = starts[r["k"]]
            r[f] = value
    return reports


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        t = json.load(f)
    have = meta()
    assert have["cu_count"] == t["meta"]["cu_count"], (have, t["meta"])
    assert have["switches"] == t["meta"]["switches"] == {s: None for s in SWITCHES}, (have, t["meta"])
    assert have["reddit_half_sha256"] == t["meta"]["reddit_half_sha256"], "graphgen gives another graph than the recorded one"
    assert sorted(t["configs"]) == sorted(CONFIGS)
    yield t
    _GRAPHS.clear()                                      # (the Reddit-shaped graph lives on the device)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_reports_and_results_equal_the_recorded_route_table(table, name):
    have, want = record(name), table["configs"][name]
    for h, w in zip(have["reports"], unpack_reports(want["reports"])):
        assert h == w, (name, h, w)
    packed = pack(have)
    assert sorted(packed["results"]) == sorted(want["results"])
    for key in want["results"]:
        assert packed["results"][key] == want["results"][key], (name, key, adj_hint(have, key), have["results"][key])
    assert have["reports_after_the_calls"] == want["reports_after_the_calls"]


# The live kernel timing (profile_begin / profile_end) on every family of the launch, both element types: (plan, operand
# dtype, k, result dtype) -> the event pairs three calls record.  The counts are those of the library of commit 4ca21ae
# (loaded through GCN_AMD_LIB), which had the fp32 and the bf16 group pass as two copies of the code that arms the events.
PROFILE_CASES = {
    "norm-f32-k64": (_c, torch.float32, 64, torch.float32, 3),
    "norm-f32-k16": (_c, torch.float32, 16, torch.float32, 3),
    "norm-bf16-k128-f32_result": (_c, BF16, 128, torch.float32, 3),
    "norm-bf16-k128-bf16_result": (_c, BF16, 128, BF16, 3),
    "perturbed-weighted-f32-k64": (_d, torch.float32, 64, torch.float32, 3),
    "short-unsliced-f32-k64": (_a, torch.float32, 64, torch.float32, 3),
    "banded-panels-f32-k64": (CONFIGS["g_panels"][0], torch.float32, 64, torch.float32, 3),
    "col16-sliced_quad-f32-k64": (_f16, torch.float32, 64, torch.float32, 3),
}


@pytest.mark.parametrize("name", list(PROFILE_CASES))
def test_profile_records_one_pair_per_main_launch(name):
    make, dtype, k, out_dtype, pairs = PROFILE_CASES[name]
    with torch.cuda.device(_dev()):
        adj = make()
        B = torch.from_numpy(np.random.default_rng(5).standard_normal((adj.n, k)).astype(np.float32)).to(_dev()).to(dtype)
        out = torch.empty((adj.m, k), dtype=out_dtype, device=_dev())
        adj.profile_begin(8)
        for _ in range(3):
            adj.matmul_raw(B, out=out)
        ms = adj.profile_end()
        print(name, adj.main_kernel(k, dtype=dtype), "pairs", len(ms), "ms", ms)
    assert len(ms) == pairs, (name, ms)
    assert all(np.isfinite(t) and t > 0 for t in ms), (name, ms)


def adj_hint(have, key):
    """the kernel the width of a differing digest is reported to run on"""
    k = int(key.split("_")[1])
    return next((r["main_kernel_bf16" if key.startswith("bf16") else "main_kernel"] for r in have["reports"] if r["k"] == k), None)
