"""The device merge on the GPU against the numpy twins of tests/coalesce_ref.py: integers equal, values of a merged run bit
for bit (the fold order is the contract's) — every row length on both sides of the wave width, of the pass width and of
the long-row bound, runs across those boundaries, every place a diagonal can take, NaN and infinities, unsorted rows,
off-grid operands, a side stream; then the degrees and the normalisation, the union with the transpose, and the whole way
from an edge list to Â against the host pipeline, into the SpMM and through a layer."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gcn_amd
from gcn_amd import _lib
from gcn_amd.coalesce import DIAGONAL, NORM, REDUCE
from gcn_amd.preprocess import normalize_adj
from coalesce_ref import (coalesce_ref, degree_ref, gcn_adjacency_ref, normalize_ref, sorted_csr_ref, symmetrize_ref,
                          within_one_ulp)
from test_spmm_gpu import TOL
from util import guards_intact, offset_view, oracle_spmm, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
LONG = _lib.SAMPLE_LONG_ROW
_cache = {}


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def make_adj(rp, ci, va, m, n, **kw):
    return gcn_amd.CsrAdjacency(t(rp.astype(np.int32)), t(ci.astype(np.int32)), t(va), (m, n), **kw)


def same_values(got, want):
    """bit for bit, except that a NaN matches any NaN (which NaN an operation returns is not part of the contract, and
    differs between processors)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return (got.shape == want.shape and np.array_equal(np.isnan(got), nan)
            and np.array_equal(got[~nan].view(np.int32), want[~nan].view(np.int32)))


def check_coalesce(rp, ci, va, m, n, reduce, diagonal, dv=1.0, assume_sorted=True, ref=None):
    out, seg = gcn_amd.coalesce_csr(make_adj(rp, ci, va, m, n), reduce, diagonal, dv, assume_sorted=assume_sorted)
    orp, oci, ova, _, rseg = ref if ref is not None else coalesce_ref(rp, ci, va, n, reduce, diagonal, dv)
    assert (out.m, out.n, out.nnz) == (m, n, len(oci)) and seg.dtype == torch.int32
    assert np.array_equal(out.rowptr.cpu().numpy(), orp) and np.array_equal(out.col.cpu().numpy(), oci)
    assert np.array_equal(seg.cpu().numpy(), rseg)
    assert same_values(out.val.cpu().numpy(), ova)
    return out, seg


def rows_matrix(m, n, lens_at, seed):
    """rows of the given lengths at the given row indices (the rest empty), columns drawn with replacement from a window
    of 1.3 x the length around the diagonal — about a third of the entries repeat, and the diagonal is there or not —
    column-sorted; values N(0, 1)"""
    rng = np.random.default_rng(seed)
    lens = np.zeros(m, np.int64)
    cols = []
    for r, L in sorted(lens_at.items()):
        lens[r] = L
        K = min(n, max(1, int(1.3 * L)))
        lo = min(max(0, r - K // 2), n - K)
        cols.append(np.sort(rng.integers(lo, lo + K, L)))
    rp = np.zeros(m + 1, np.int32)
    rp[1:] = np.cumsum(lens)
    ci = np.concatenate(cols).astype(np.int32) if cols else np.zeros(0, np.int32)
    return rp, ci, rng.standard_normal(len(ci)).astype(np.float32)


LENS = [0, 1, 2, 63, 64, 65, 127, 128, 129, LONG - 1, LONG, LONG + 1, 5000]


def lens_matrix():
    if "lens" not in _cache:
        n = 6000
        rp, ci, va = rows_matrix(n, n, {37 + 450 * i: L for i, L in enumerate(LENS)}, seed=1)
        rows = np.repeat(np.arange(n), np.diff(rp))
        frac = 1 - len(np.unique(rows * n + ci)) / len(ci)
        assert 0.2 < frac < 0.45 and np.diff(rp).max() == 5000
        _cache["lens"] = (rp, ci, va, n)
    return _cache["lens"]


@pytest.mark.parametrize("diagonal", list(DIAGONAL))
@pytest.mark.parametrize("reduce", list(REDUCE))
def test_every_row_length_with_every_reduce_and_diagonal_code(reduce, diagonal):
    rp, ci, va, n = lens_matrix()
    out, seg = check_coalesce(rp, ci, va, n, n, reduce, diagonal, 0.75)
    assert out.symmetric is (False if reduce == "first" else None)


def test_runs_across_wave_pass_and_long_row_boundaries():
    n = 6000

    def row_with_run(L, lo, hi, start):                 # L entries, ascending columns from `start`, entries lo .. hi one run
        step = np.ones(L, np.int64)
        step[lo + 1:hi + 1] = 0
        return start + np.cumsum(step) - 1

    rows = [row_with_run(130, 62, 66, 10),              # across the wave width of the first pass
            row_with_run(LONG + 300, LONG - 2, LONG + 2, 100),     # across entry 2048 of a long row
            row_with_run(LONG + 1, 254, 258, 200),      # across the first pass boundary of the 256-thread tier
            np.full(300, 4321),                         # one single run
            row_with_run(5000, 1000, 3999, 50)]         # a 3000-entry run inside a long row
    assert len(np.unique(rows[4])) == 5000 - 2999
    m = len(rows)
    rp = np.zeros(m + 1, np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.concatenate(rows).astype(np.int32)
    va = np.random.default_rng(2).standard_normal(len(ci)).astype(np.float32)
    for reduce, diagonal in (("sum", "keep"), ("max", "fill"), ("first", "add"), ("min", "drop")):
        check_coalesce(rp, ci, va, m, n, reduce, diagonal, 2.5)


DIAG_ROWS = {0: [0, 3, 9],                              # the diagonal first
             1: [],                                     # absent in an empty row
             2: [0, 1, 2],                              # ... last
             3: [1, 3, 3, 7],                           # ... twice, as a run, in the middle
             4: [0, 1, 2, 3],                           # absent, every column left of it
             5: [6, 7, 7, 9],                           # absent, every column right of it
             6: [2, 6, 8],                              # in the middle
             7: [0, 9],                                 # absent, between
             8: [8],                                    # alone
             9: [3, 3, 3]}                              # absent, one run


@pytest.mark.parametrize("diagonal", list(DIAGONAL))
def test_every_place_of_the_diagonal(diagonal):
    m = n = 10
    rp = np.zeros(m + 1, np.int32)
    rp[1:] = np.cumsum([len(DIAG_ROWS[r]) for r in range(m)])
    ci = np.concatenate([DIAG_ROWS[r] for r in range(m)]).astype(np.int32)
    va = (np.arange(len(ci)) + 1).astype(np.float32)
    out, seg = check_coalesce(rp, ci, va, m, n, "sum", diagonal, 0.5)
    if diagonal in ("fill", "add"):
        assert sorted(out.col[out.rowptr[7]:out.rowptr[8]].tolist()) == [0, 7, 9] and out.col[out.rowptr[1]].item() == 1
    for shape in ((7, 19), (19, 7)):                    # rectangular: the rows r >= n have no diagonal
        rpr, cir, var = rows_matrix(shape[0], shape[1], {r: 1 + (3 * r) % 6 for r in range(shape[0]) if r != 4}, seed=3)
        out, _ = check_coalesce(rpr, cir, var, shape[0], shape[1], "max", diagonal, 0.5)
        if diagonal == "fill":                          # (row 4 is empty, and 4 < n in both shapes)
            assert int(out.rowptr[5] - out.rowptr[4]) == 1 and out.col[out.rowptr[4]].item() == 4
    for c in ([0], [], [0, 0]):                         # m = n = 1
        rp1 = np.array([0, len(c)], np.int32)
        check_coalesce(rp1, np.array(c, np.int32), np.ones(len(c), np.float32), 1, 1, "sum", diagonal, 0.5)


def test_no_entries_with_fill_gives_the_identity_pattern():
    z = np.zeros(0, np.int32)
    for m, n in ((5, 5), (3, 7), (7, 3)):
        out, seg = check_coalesce(np.zeros(m + 1, np.int32), z, np.zeros(0, np.float32), m, n, "sum", "fill", 2.0)
        k = min(m, n)
        assert out.col.tolist() == list(range(k)) and out.val.tolist() == [2.0] * k and seg.numel() == 0
        assert out.rowptr.tolist() == [min(r, k) for r in range(m + 1)]
    out, _ = check_coalesce(np.zeros(6, np.int32), z, np.zeros(0, np.float32), 5, 5, "sum", "keep")
    assert out.nnz == 0
    out, seg = check_coalesce(np.array([0, 1, 3], np.int32), np.array([0, 1, 1], np.int32), np.ones(3, np.float32), 2, 2, "sum",
                              "drop")                   # every entry dropped: nothing to fill
    assert out.nnz == 0 and seg.tolist() == [-1, -1, -1]


@pytest.mark.parametrize("reduce", ["sum", "max", "min"])
def test_nan_and_infinities_inside_runs(reduce):
    inf, nan = np.inf, np.nan
    runs = [[1, nan, 2], [nan, 1], [1, 2, nan], [inf, 1], [1, -inf, 2], [inf, -inf], [-inf, inf, 3], [inf, inf], [nan, inf],
            [3, 1, 2], [-0.0, 0.0], [0.0, -0.0]]
    ci = np.concatenate([[c] * len(r) for c, r in enumerate(runs)]).astype(np.int32)
    va = np.concatenate(runs).astype(np.float32)
    rp = np.array([0, len(ci)], np.int32)
    out, _ = check_coalesce(rp, ci, va, 1, 20, reduce, "keep")
    got = out.val.cpu().numpy()
    want_nan = {"sum": [0, 1, 2, 5, 6, 8], "max": [0, 1, 2, 8], "min": [0, 1, 2, 8]}[reduce]
    assert np.flatnonzero(np.isnan(got)).tolist() == want_nan
    assert got[3] == {"sum": inf, "max": inf, "min": 1}[reduce] and got[4] == {"sum": -inf, "max": 2, "min": -inf}[reduce] and got[9] == {"sum": 6, "max": 3, "min": 1}[reduce]


def test_unsorted_rows_merge_adjacent_columns_only_and_a_full_merge_after_sorting():
    rng = np.random.default_rng(4)
    m, n = 50, 30
    lens = rng.integers(0, 40, m)
    lens[[3, 20]] = [0, 300]
    rp = np.zeros(m + 1, np.int32)
    rp[1:] = np.cumsum(lens)
    ci = rng.integers(0, n, rp[-1]).astype(np.int32)   # unsorted, with adjacent repeats here and there
    va = rng.standard_normal(len(ci)).astype(np.float32)
    rows = np.repeat(np.arange(m), lens)
    for reduce, diagonal in (("sum", "keep"), ("first", "fill"), ("max", "add"), ("sum", "drop")):
        out, _ = check_coalesce(rp, ci, va, m, n, reduce, diagonal, 0.5, assume_sorted=True)
        assert diagonal != "keep" or out.nnz > len(np.unique(rows * n + ci))                 # not a full merge
        srp, eid = sorted_csr_ref(rows, ci, m)
        ref = coalesce_ref(srp, ci[eid], va[eid], n, reduce, diagonal, 0.5)
        seg = np.empty(len(ci), np.int32)
        seg[eid] = ref[4]                                                    # the twin's seg, in the original entry order
        out, _ = check_coalesce(rp, ci, va, m, n, reduce, diagonal, 0.5, assume_sorted=False, ref=ref[:4] + (seg,))
        assert diagonal != "keep" or out.nnz == len(np.unique(rows * n + ci))                # every distinct pair once


# ---- the raw calls -------------------------------------------------------------------------------------------------------------
def _p(x):
    return ctypes.c_void_p(x.data_ptr()) if x is not None else None


def raw_count(rp, ci, m, n, diagonal, stream=None):
    lib = _lib.load()
    st = ctypes.c_void_p(stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    ws = torch.empty(_lib.COALESCE_WS_BYTES, dtype=torch.uint8, device=DEV)
    out_len = torch.zeros(m, dtype=torch.int32, device=DEV)
    _lib.check(lib.gcn_csr_coalesce_count(_p(rp), _p(ci), m, n, ci.numel(), DIAGONAL[diagonal], _p(out_len), _p(ws), ws.numel(), st),
               "count")
    return out_len


def raw_fill(rp, ci, va, m, n, reduce, diagonal, dv, orp, oci, ova, first, seg, stream=None):
    lib = _lib.load()
    st = ctypes.c_void_p(stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    ws = torch.empty(_lib.COALESCE_WS_BYTES, dtype=torch.uint8, device=DEV)
    _lib.check(lib.gcn_csr_coalesce_fill(_p(rp), _p(ci), _p(va), m, n, ci.numel(), REDUCE[reduce], DIAGONAL[diagonal], dv, _p(orp),
                                         _p(oci), _p(ova), _p(first), _p(seg), _p(ws), ws.numel(), st), "fill")


def small_matrix():
    if "small" not in _cache:
        m, n = 400, 400
        lens = {r: L for r, L in zip(range(0, 400, 3), np.random.default_rng(5).integers(1, 90, 134))}
        lens.update({100: LONG + 70, 301: 64, 302: 65})
        _cache["small"] = rows_matrix(m, n, lens, seed=6) + (m, n)
    return _cache["small"]


def test_operands_off_the_grid_a_pattern_call_two_calls_and_a_side_stream():
    rp, ci, va, m, n = small_matrix()
    ref = coalesce_ref(rp, ci, va, n, "sum", "fill", 0.5)
    total = len(ref[1])
    # every operand 4 bytes past a 16-byte boundary, between guards
    (rpv, rpf), (civ, cif), (vav, vaf) = (offset_view(a, 1, dt, DEV) for a, dt in ((rp, torch.int32), (ci, torch.int32),
                                                                                  (va, torch.float32)))
    out_len = raw_count(rpv, civ, m, n, "fill")
    assert np.array_equal(out_len.cpu().numpy(), np.diff(ref[0]))
    orpv, orpf = offset_view(ref[0], 1, torch.int32, DEV)
    outs = [offset_view(total, 1, dt, DEV) for dt in (torch.int32, torch.float32, torch.int32)] + [offset_view(len(ci), 1, torch.int32, DEV)]
    (ociv, _), (ovav, _), (firstv, _), (segv, _) = outs
    assert all(v.data_ptr() % 16 == 4 for v in (rpv, civ, vav, orpv, ociv, ovav, firstv, segv))
    raw_fill(rpv, civ, vav, m, n, "sum", "fill", 0.5, orpv, ociv, ovav, firstv, segv)
    for (view, flat), want in zip(outs, (ref[1], ref[2], ref[3], ref[4])):
        assert np.array_equal(view.cpu().numpy().view(np.int32), want.view(np.int32)) and guards_intact(flat, view)
    assert guards_intact(rpf, rpv) and guards_intact(cif, civ) and guards_intact(vaf, vav) and guards_intact(orpf, orpv)
    # a pattern: no values in, none out; first and seg left out as well
    pat = coalesce_ref(rp, ci, None, n, "sum", "fill")
    oci = torch.full((total,), -7, dtype=torch.int32, device=DEV)
    raw_fill(t(rp), t(ci), None, m, n, "sum", "fill", 0.5, t(ref[0]), oci, None, None, None)
    assert pat[2] is None and np.array_equal(oci.cpu().numpy(), pat[1]) and np.array_equal(pat[1], ref[1])
    # twice, and once on a side stream: the same bits
    adj = make_adj(rp, ci, va, m, n)
    a, sa = gcn_amd.coalesce_csr(adj, "sum", "fill", 0.5, assume_sorted=True)
    b, sb = gcn_amd.coalesce_csr(adj, "sum", "fill", 0.5, assume_sorted=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c, sc = gcn_amd.coalesce_csr(adj, "sum", "fill", 0.5, assume_sorted=False)     # (sorted already: the same result)
    side.synchronize()
    for x, sx in ((b, sb), (c, sc)):
        assert torch.equal(a.rowptr, x.rowptr) and torch.equal(a.col, x.col) and torch.equal(sa, sx)
        assert torch.equal(a.val.view(torch.int32), x.val.view(torch.int32))
    assert np.array_equal(a.val.cpu().numpy().view(np.int32), ref[2].view(np.int32))


def test_fill_with_a_wrong_slot_writes_nothing_for_that_row():
    rp, ci, va, m, n = small_matrix()
    ref = coalesce_ref(rp, ci, va, n, "max", "keep")
    for bad in (99, 100):                               # a wave's row and the long row
        assert rp[bad + 1] > rp[bad]
        orp = ref[0].copy()
        orp[bad + 1:] += 1                              # the slot of row `bad` one too long; the rows behind it move up by one
        total = int(orp[-1])
        S = -7
        oci, first = (torch.full((total,), S, dtype=torch.int32, device=DEV) for _ in range(2))
        ova = torch.full((total,), float(S), device=DEV)
        seg = torch.full((len(ci),), S, dtype=torch.int32, device=DEV)
        raw_fill(t(rp), t(ci), t(va), m, n, "max", "keep", 0.0, t(orp), oci, ova, first, seg)
        lo, hi = int(orp[bad]), int(orp[bad + 1])
        oci, ova, first, seg = (x.cpu().numpy() for x in (oci, ova, first, seg))
        assert np.all(oci[lo:hi] == S) and np.all(ova[lo:hi] == S) and np.all(first[lo:hi] == S)
        assert np.all(seg[rp[bad]:rp[bad + 1]] == S)
        cut = int(ref[0][bad]), int(ref[0][bad + 1])    # the row's place in the twin's arrays
        for got, want in ((oci, ref[1]), (ova, ref[2]), (first, ref[3])):
            assert np.array_equal(got[:lo], want[:cut[0]]) and np.array_equal(got[hi:], want[cut[1]:])
        assert np.array_equal(seg[:rp[bad]], ref[4][:rp[bad]]) and np.array_equal(seg[rp[bad + 1]:], ref[4][rp[bad + 1]:] + 1)


# ---- degrees and normalisation -------------------------------------------------------------------------------------------------
def raw_degree(rp, va, m):
    deg = torch.full((m,), -1.0, dtype=torch.float64, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().gcn_csr_degree_f64(_p(rp), _p(va), m, int(rp[-1]), _p(deg), st), "degree")
    return deg


def raw_normalize(rp, ci, va, m, n, deg, mode):
    out = torch.full((ci.numel(),), float("nan"), device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.load().gcn_csr_normalize_f32(_p(rp), _p(ci), _p(va), m, n, ci.numel(), _p(deg), NORM[mode], _p(out), st), "normalize")
    return out


def test_degree_and_normalize():
    n = 6000
    special = {37 + 450 * i: L for i, L in enumerate(LENS)}                 # every length of LENS, the other rows 1 .. 4 entries
    short = np.random.default_rng(9).integers(1, 5, n)
    rp, ci, va = rows_matrix(n, n, {r: special.get(r, short[r]) for r in range(n)}, seed=10)
    va = np.abs(va) + np.float32(0.01)                  # positive terms: the bound on the fp64 sum is relative to the sum
    zero = 37 + 450 * 2                                 # the row of two entries: values 1 and -1, so its degree is exactly zero
    assert rp[zero + 1] - rp[zero] == 2
    va[rp[zero]:rp[zero] + 2] = [1.0, -1.0]
    hub = 37 + 450 * 12
    ci[rp[hub]] = zero                                  # (the hub's first entry points at the zero-degree vertex)
    rpd, cid, vad = t(rp), t(ci), t(va)
    # pattern degrees are exact; weighted ones within 1e-12 relative of the fp64 twin (the order of the fp64 sum is not
    # specified: for at most 5000 positive terms the two orders differ by at most about 5000 * 2^-53 = 6e-13 relative)
    assert np.array_equal(raw_degree(rpd, None, n).cpu().numpy(), degree_ref(rp, None))
    deg = raw_degree(rpd, vad, n)
    ref_deg = degree_ref(rp, va)
    got = deg.cpu().numpy()
    print("max relative degree error", np.max(np.abs(got - ref_deg) / np.maximum(ref_deg, 1e-300)))
    assert np.all(np.abs(got - ref_deg) <= 1e-12 * ref_deg) and got[zero] == 0 and ref_deg[zero] == 0
    assert torch.equal(deg.view(torch.int64), raw_degree(rpd, vad, n).view(torch.int64))          # twice: the same bits
    for mode in ("sym", "row"):
        out = raw_normalize(rpd, cid, vad, n, n, deg, mode)
        ref = normalize_ref(rp, ci, va, ref_deg, mode)
        o = out.cpu().numpy()
        assert np.all(np.isfinite(o)) and np.all(within_one_ulp(o, ref))
        assert np.all(o[rp[zero]:rp[zero + 1]] == 0) and (mode == "row" or o[rp[hub]] == 0)       # zeros, not inf or NaN
        assert torch.equal(out.view(torch.int32), raw_normalize(rpd, cid, vad, n, n, deg, mode).view(torch.int32))
        adj = gcn_amd.normalize_csr(make_adj(rp, ci, va, n, n, symmetric=False), mode)
        assert torch.equal(adj.val.view(torch.int32), out.view(torch.int32)) and adj.symmetric is False
    pat = raw_normalize(rpd, cid, None, n, n, raw_degree(rpd, None, n), "row").cpu().numpy()     # a pattern: v = 1
    assert np.all(within_one_ulp(pat, normalize_ref(rp, ci, None, degree_ref(rp, None), "row")))
    with pytest.raises(ValueError, match="square"):
        gcn_amd.normalize_csr(make_adj(rp[:8], ci[:rp[7]], va[:rp[7]], 7, n), "sym")


# ---- the union with the transpose, and the whole way to Â --------------------------------------------------------------------
NV = 300


def directed_graph():
    """a directed 300-vertex edge list with repeats and some self-loops (none on vertex 0), vertices without edges; values
    small positive multiples of 1/8"""
    if "graph" not in _cache:
        rng = np.random.default_rng(7)
        rows, cols = rng.integers(0, NV, 2500), rng.integers(0, NV, 2500)
        keep = ~np.isin(rows, [9, 150]) & ~np.isin(cols, [9, 150]) & (rows != cols)
        rows, cols = rows[keep], cols[keep]
        loops = np.array([3, 3, 40, 77, 299])
        rows, cols = np.concatenate([rows, rows[:200], loops]), np.concatenate([cols, cols[:200], loops])
        order = rng.permutation(len(rows))
        rows, cols = rows[order], cols[order]
        _cache["graph"] = (rows, cols, (rng.integers(1, 9, len(rows)) / 8).astype(np.float32))
    return _cache["graph"]


def host_a_hat():
    """the symmetrisation lines of io.load_deeprobust_npz followed by preprocess.normalize_adj (fp64)"""
    if "a_hat" not in _cache:
        rows, cols, _ = directed_graph()
        adj = sp.coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(NV, NV)).tocsr()
        adj = (adj + adj.T).tolil()
        adj[adj > 1] = 1
        adj.setdiag(0)
        adj = adj.astype(np.float32).tocsr()
        adj.eliminate_zeros()
        assert adj[0, 0] == 0
        out = sp.csr_matrix(normalize_adj(adj))
        out.sort_indices()
        _cache["a_hat"] = out
    return _cache["a_hat"]


def test_symmetrize_is_scipys_maximum_with_the_transpose():
    rows, cols, vals = directed_graph()
    adj, _ = gcn_amd.csr_from_edges(t(rows), t(cols), (NV, NV), t(vals))
    merged, seg = gcn_amd.coalesce_csr(adj, "sum", assume_sorted=True)       # (csr_from_edges sorts the columns)
    A = sp.coo_matrix((vals, (rows, cols)), shape=(NV, NV)).tocsr()          # (sums the repeats; eighths: exact in any order)
    A.sort_indices()
    assert A.nnz < len(rows) and np.array_equal(merged.rowptr.cpu().numpy(), A.indptr)
    assert np.array_equal(merged.col.cpu().numpy(), A.indices) and np.array_equal(merged.val.cpu().numpy(), A.data)
    sym = gcn_amd.symmetrize(merged)
    S = A.maximum(A.T).tocsr()
    S.sort_indices()
    assert np.array_equal(sym.rowptr.cpu().numpy(), S.indptr) and np.array_equal(sym.col.cpu().numpy(), S.indices)
    assert np.array_equal(sym.val.cpu().numpy(), S.data)
    assert sym.symmetric is True and sym.transpose() is sym
    for reduce in ("sum", "min"):
        got = gcn_amd.symmetrize(merged, reduce)
        ref = symmetrize_ref(A.indptr, A.indices, A.data, reduce)
        assert np.array_equal(got.rowptr.cpu().numpy(), ref[0]) and np.array_equal(got.col.cpu().numpy(), ref[1])
        assert same_values(got.val.cpu().numpy(), ref[2])
    with pytest.raises(ValueError, match="square"):
        gcn_amd.symmetrize(make_adj(np.array([0, 1], np.int32), np.array([2], np.int32), np.ones(1, np.float32), 1, 3))


def test_gcn_adjacency_is_the_host_pipeline_and_feeds_the_spmm_and_a_layer():
    rows, cols, vals = directed_graph()
    host = host_a_hat()
    a_hat = gcn_amd.gcn_adjacency(t(rows), t(cols).to(torch.int32), NV)
    assert (a_hat.m, a_hat.n, a_hat.symmetric) == (NV, NV, True)
    assert np.array_equal(a_hat.rowptr.cpu().numpy(), host.indptr) and np.array_equal(a_hat.col.cpu().numpy(), host.indices)
    got = a_hat.val.cpu().numpy()
    assert np.all(within_one_ulp(got, host.data))
    twin = gcn_adjacency_ref(rows, cols, NV)
    assert np.array_equal(twin[1], host.indices) and np.all(within_one_ulp(got, twin[2].astype(np.float64)))
    # the other options against the twin: weighted sum with added self-loops and row normalisation; no normalisation
    for kw in (dict(values=vals, reduce="sum", self_loops="add", norm="row"), dict(values=vals, symmetrize=False, self_loops="drop", norm=None),
               dict(reduce="sum", self_loops="keep", norm=None), dict(self_loops="keep", norm=None)):
        dkw = dict(kw, values=t(vals)) if "values" in kw else kw
        out = gcn_amd.gcn_adjacency(t(rows), t(cols), NV, **dkw)
        ref = gcn_adjacency_ref(rows, cols, NV, **kw)
        assert np.array_equal(out.rowptr.cpu().numpy(), ref[0]) and np.array_equal(out.col.cpu().numpy(), ref[1])
        if kw.get("norm", "sym") is None:
            assert same_values(out.val.cpu().numpy(), ref[2])
        else:
            assert np.all(within_one_ulp(out.val.cpu().numpy(), ref[2].astype(np.float64)))
        assert out.symmetric is (kw.get("symmetrize", True) and kw.get("norm", "sym") != "row")
    # into the SpMM: the device-built Â and the host-built one against an fp64 product, at the SpMM tests' tolerance
    k = 32
    X = np.random.default_rng(8).standard_normal((NV, k)).astype(np.float32)
    ref = oracle_spmm(host.indptr, host.indices, host.data.astype(np.float32), X)
    from_host = gcn_amd.CsrAdjacency.from_scipy(host.astype(np.float32), symmetric=True)
    for adj in (a_hat, from_host):
        assert rel_err(gcn_amd.spmm(adj, t(X)).cpu().numpy(), ref) <= TOL
    # and through a layer, forward and backward
    torch.manual_seed(0)
    layer = gcn_amd.GraphConvolution(k, 8).to(DEV)
    x = t(X).requires_grad_(True)
    out = layer(x, a_hat)
    out.square().sum().backward()
    dense = torch.from_numpy(host.toarray()).to(DEV)
    xr = t(X).double().requires_grad_(True)
    outr = dense @ (xr @ layer.weight.detach().double()) + layer.bias.detach().double()
    outr.square().sum().backward()
    # (every product is within TOL by the suite's yardstick: the forward chains two of them, the backward three and the
    # factor 2 of the square)
    assert rel_err(out.detach().cpu().numpy(), outr.detach().cpu().numpy()) <= 2 * TOL
    assert rel_err(x.grad.cpu().numpy(), xr.grad.cpu().numpy()) <= 4 * TOL
