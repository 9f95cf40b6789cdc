"""The sparse x sparse product on the GPU against the numpy twin of tests/spgemm_ref.py: every integer equal, every value bit
for bit (the fold order is the contract's) — product counts on both sides of the wave width and of the two class bounds,
tables at their stated load, probing, dense rows that reuse a workgroup's stamps, empty operands, the fold order made
visible, NaN, infinities and a lone -0.0, patterns, unsorted B, off-grid operands, a side stream, a wrong slot; then
gcn_amd.spgemm against scipy within the summation bound and the hypergraph Laplacian against its twin, its transpose, the
dense fp64 formula, into the SpMM and through a layer.

The shapes follow the exported limits W = SPGEMM_WAVE_MAX, G = SPGEMM_BLOCK_MAX, D = SPGEMM_DENSE_BLOCKS.  The matrix pair of
the first tests has n = G + G / 4 columns (10 240), not 6 000: a row's class is decided by min(products, n), so with
n = 6 000 < G no row reaches the dense class and no row can hold G distinct columns — the cases the pair exists for."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gcn_amd
from gcn_amd import _lib
from spgemm_ref import hypergraph_laplacian_ref, sorted_merged_ref, spgemm_ref
from test_spgemm_cpu import U24, _random_csr, dense_g, hypergraph_fixture, shared_hyperedges, summation_bound
from test_spmm_gpu import TOL
from util import guards_intact, offset_view, oracle_spmm, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
W, G, D = _lib.SPGEMM_WAVE_MAX, _lib.SPGEMM_BLOCK_MAX, _lib.SPGEMM_DENSE_BLOCKS
_cache = {}


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_values(got, want):
    """bit for bit, except that a NaN matches any NaN (which NaN an operation returns is not part of the contract)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return (got.shape == want.shape and np.array_equal(np.isnan(got), nan)
            and np.array_equal(got[~nan].view(np.int32), want[~nan].view(np.int32)))


def _p(x):
    return ctypes.c_void_p(x.data_ptr()) if x is not None else None


def _stream(stream):
    return ctypes.c_void_p(stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream)


def raw_count(a, b, m, p, n, stream=None):
    """a, b: (rowptr, col, val or None) device tensors -> out_len int32 [m]"""
    ws = torch.empty(_lib.spgemm_ws_bytes(m, n), dtype=torch.uint8, device=DEV)
    out_len = torch.full((m,), -7, dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().gcn_spgemm_count_csr(_p(a[0]), _p(a[1]), m, p, a[1].numel(), _p(b[0]), _p(b[1]), n, b[1].numel(),
                                                _p(out_len), _p(ws), ws.numel(), _stream(stream)), "count")
    return out_len


def raw_fill(a, b, m, p, n, orp, oci, ova, stream=None):
    ws = torch.empty(_lib.spgemm_ws_bytes(m, n), dtype=torch.uint8, device=DEV)
    _lib.check(_lib.load().gcn_spgemm_fill_csr(_p(a[0]), _p(a[1]), _p(a[2]), m, p, a[1].numel(), _p(b[0]), _p(b[1]), _p(b[2]), n,
                                               b[1].numel(), _p(orp), _p(oci), _p(ova), _p(ws), ws.numel(), _stream(stream)), "fill")


def raw_product(a, b, p, n, stream=None):
    """count, the scan, fill for numpy operands (rowptr, col, val or None) -> numpy (rowptr, col, val or None)"""
    m = len(a[0]) - 1
    da, db = (tuple(t(x) if x is not None else None for x in op) for op in (a, b))
    out_len = raw_count(da, db, m, p, n, stream)
    orp = np.zeros(m + 1, np.int32)
    orp[1:] = np.cumsum(out_len.cpu().numpy())
    total = int(orp[-1])
    values = a[2] is not None or b[2] is not None
    oci = torch.full((total,), -7, dtype=torch.int32, device=DEV)
    ova = torch.full((total,), -7.0, device=DEV) if values else None
    if total > 0:                                       # (a caller whose counts sum to 0 has nothing to fill: no arrays to hand over)
        raw_fill(da, db, m, p, n, t(orp), oci, ova, stream)
    torch.cuda.synchronize()
    return orp, oci.cpu().numpy(), ova.cpu().numpy() if values else None


def check_product(a, b, p, n, ref=None):
    ref = ref if ref is not None else spgemm_ref(*a, *b, p, n)
    orp, oci, ova = raw_product(a, b, p, n)
    assert np.array_equal(orp, ref[0]) and np.array_equal(oci, ref[1])
    assert (ova is None and ref[2] is None) or same_values(ova, ref[2])
    return orp, oci, ova


def csr_of(rows, dtype):
    rp = np.zeros(len(rows) + 1, np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    return rp, (np.concatenate([np.asarray(r, dtype) for r in rows]) if rp[-1] else np.zeros(0, dtype)).astype(dtype)


# ---- the matrix pair of the classes --------------------------------------------------------------------------------------------
N = G + G // 4                                          # 20 blocks of W columns
COUNTS = [0, 1, 2, 63, 64, 65, W - 1, W, W + 1, G - 1, G, G + 1, 3 * G]


def class_pair():
    """B: row 0 empty; rows 1 .. 20: block k = the columns [k W, (k + 1) W) in a random order; row 21: 64 columns; rows
    22 .. 26: one column each; row 27: the columns equal to 5 modulo 2 W (the slots of a full wave table).
    A: rows with the product counts of COUNTS, built from q entries on row 21 (64 products each, all on the same 64 columns)
    and r on the single-column rows, so the distinct columns stay below 70 whatever the count; then the special rows."""
    if "pair" in _cache:
        return _cache["pair"]
    rng = np.random.default_rng(11)
    nblk = N // W
    assert N == nblk * W and nblk >= 17 and N > G
    b_rows = [[]] + [rng.permutation(np.arange(k * W, (k + 1) * W)) for k in range(nblk)]
    BLK64, ONE, MOD = nblk + 1, nblk + 2, nblk + 7
    b_rows.append(rng.choice(N, 64, replace=False))
    b_rows += [[c] for c in (7, 4107, 64, N - 1, 0)]
    b_rows.append(np.arange(5, N, 2 * W))
    p = len(b_rows)
    a_rows = {}
    at = 3
    for u in COUNTS:                                    # product counts, most products colliding
        q, r = divmod(u, 64)
        ent = [BLK64] * q + [ONE + (i % 5) for i in range(r)]
        if u in (65, W + 1):
            ent = ent[:1] + [0] + ent[1:]               # ... with an entry that points at the empty row of B in between
        a_rows[at] = rng.permutation(ent)
        at += 7
    special = {"one_column": [ONE] * 300,               # 300 products on one column
               "w_distinct": [4],                       # exactly W distinct columns: a wave's table at its stated load
               "g_distinct": list(range(1, 1 + G // W)),         # exactly G distinct columns: the workgroup's table at its load
               "probing": [MOD] * (W // len(b_rows[MOD]) - 1)}   # every column on slot 5 of 2 W slots
    where = {}
    for name, ent in special.items():
        a_rows[at] = np.array(ent)
        where[name] = at
        at += 5
    m = 16 * (D + 6)
    dense = [0] + [16 * k + 5 for k in range(D // 2 + 1)] + [16 * k + 10 + k for k in range(1, D + 3 - D // 2 - 1)]
    assert len(dense) == D + 3 and len(set(dense)) == D + 3 and not set(dense) & set(a_rows) and max(dense) < m
    for k, r in enumerate(dense):                       # 17 of the 20 blocks, the window moving: overlapping columns
        a_rows[r] = np.array([1 + (k + s) % nblk for s in range(G // W + 1)] + [BLK64, BLK64])
    rows = [a_rows.get(i, []) for i in range(m)]
    a_rp, a_ci = csr_of(rows, np.int32)
    b_rp, b_ci = csr_of(b_rows, np.int32)
    a = (a_rp, a_ci, rng.standard_normal(len(a_ci)).astype(np.float32))
    b = (b_rp, b_ci, rng.standard_normal(len(b_ci)).astype(np.float32))
    ref = spgemm_ref(*a, *b, p, N)
    products, lens = ref[3], np.diff(ref[0])
    cls = np.where(np.minimum(products, N) <= W, 0, np.where(np.minimum(products, N) <= G, 1, 2))
    assert sorted(products[[3 + 7 * i for i in range(len(COUNTS))]].tolist()) == COUNTS
    assert np.all(lens[[3 + 7 * i for i in range(1, len(COUNTS))]] < 70)                    # far below the product counts
    assert products[where["one_column"]] == 300 and lens[where["one_column"]] == 1
    assert products[where["w_distinct"]] == W == lens[where["w_distinct"]]
    assert products[where["g_distinct"]] == G == lens[where["g_distinct"]]
    pr = where["probing"]
    assert W // 2 < products[pr] <= W and len(set(ref[1][ref[0][pr]:ref[0][pr + 1]] % _lib.spgemm_slots(int(products[pr])))) == 1
    assert cls[0] == 2 and np.all(cls[dense] == 2) and np.all(lens[dense] > G) and (cls == 2).sum() == D + 5
    assert np.bincount(np.flatnonzero(cls == 2) % D).max() >= 3 and (cls == 1).sum() >= 3 and (lens == 0).sum() > 100
    _cache["pair"] = (a, b, p, ref)
    return _cache["pair"]


def test_every_product_count_both_sides_of_the_class_bounds():
    a, b, p, ref = class_pair()
    check_product(a, b, p, N, ref)


@pytest.mark.parametrize("which", ["pattern_pattern", "pattern_valued", "valued_pattern"])
def test_patterns_on_the_class_pair(which):
    a, b, p, ref = class_pair()
    pa = (a[0], a[1], None if which.startswith("pattern") else a[2])
    pb = (b[0], b[1], None if which.endswith("pattern") else b[2])
    orp, oci, ova = raw_product(pa, pb, p, N)
    assert np.array_equal(orp, ref[0]) and np.array_equal(oci, ref[1])
    if which == "pattern_pattern":
        assert ova is None
    else:                                               # a pattern operand counts as ones
        ones = spgemm_ref(a[0], a[1], pa[2] if pa[2] is not None else np.ones_like(a[2]), b[0], b[1],
                          pb[2] if pb[2] is not None else np.ones_like(b[2]), p, N)
        assert same_values(ova, ones[2])


# ---- empty operands, small shapes -----------------------------------------------------------------------------------------------
def test_empty_rows_empty_operands_and_small_shapes():
    rng = np.random.default_rng(12)
    f = np.float32
    # empty rows of A, entries of A on empty rows of B
    a = csr_of([[], [0, 2], [], [1], [1, 1], []], np.int32)
    b = csr_of([[3, 0], [], [2]], np.int32)
    a, b = a + (rng.standard_normal(5).astype(f),), b + (rng.standard_normal(3).astype(f),)
    orp, oci, _ = check_product(a, b, 3, 4)
    assert orp.tolist() == [0, 0, 3, 3, 3, 3, 3] and oci.tolist() == [0, 2, 3]
    # nnz_a == 0 and nnz_b == 0: through the raw calls (null column pointers) and through spgemm
    none_a = (np.zeros(7, np.int32), np.zeros(0, np.int32), np.zeros(0, f))
    none_b = (np.zeros(4, np.int32), np.zeros(0, np.int32), np.zeros(0, f))
    lib = _lib.load()
    for x, y in ((none_a, b), (a, none_b), (none_a, none_b)):
        out_len = torch.full((6,), -7, dtype=torch.int32, device=DEV)
        dx, dy = (tuple(t(z) if len(z) else None for z in op) for op in (x, y))
        st = lib.gcn_spgemm_count_csr(_p(dx[0]), _p(dx[1]), 6, 3, len(x[1]), _p(dy[0]), _p(dy[1]), 4, len(y[1]), _p(out_len), None, 0,
                                      _stream(None))
        assert st == 0 and out_len.tolist() == [0] * 6
        adj = [gcn_amd.CsrAdjacency(t(z[0]), t(z[1]), t(z[2]), shape) for z, shape in ((x, (6, 3)), (y, (3, 4)))]
        c = gcn_amd.spgemm(*adj)
        assert (c.m, c.n, c.nnz) == (6, 4, 0) and c.rowptr.tolist() == [0] * 7 and c.symmetric is False
    # 7 x 19 · 19 x 5 and m = p = n = 1
    a, b = _random_csr(7, 19, 0.4, rng, repeats=True), _random_csr(19, 5, 0.4, rng)
    check_product(a, b, 19, 5)
    one = (np.array([0, 1], np.int32), np.array([0], np.int32), np.array([3.0], f))
    orp, oci, ova = check_product(one, (one[0], one[1], np.array([-0.5], f)), 1, 1)
    assert orp.tolist() == [0, 1] and ova.tolist() == [-1.5]
    check_product((np.array([0, 0], np.int32), none_a[1], none_a[2]), one, 1, 1)


# ---- the fold order, special values, unsorted B -----------------------------------------------------------------------------------
def test_fold_order_is_visible_in_the_bits_and_special_values_propagate():
    f = np.float32
    inf, nan = np.inf, np.nan
    # every B row j holds column 3 with value 1 (and row 3 a second column): the entries of A's row add in entry order
    b = csr_of([[3], [3], [3], [3, 1]], np.int32) + (np.array([1, 1, 1, 1, 2], f),)
    a_rows = [([0, 1, 2], [1e8, 1, -1e8]),              # (1e8 + 1) - 1e8 = 0
              ([0, 2, 1], [1e8, -1e8, 1]),              # (1e8 - 1e8) + 1 = 1
              ([1, 0, 2], [1, 1e8, -1e8]),              # (1 + 1e8) - 1e8 = 0
              ([0, 0, 0, 1], [1e8, -1e8, 1, 1]),        # the same pair three times: ((1e8 - 1e8) + 1) + 1 = 2
              ([0, 1, 0, 0], [1e8, 1, 1, -1e8]),        # ((1e8 + 1) + 1) - 1e8 = 0
              ([0], [-0.0]),                            # a lone -0.0 stays -0.0
              ([0, 1], [-0.0, 0.0]),                    # -0.0 + 0.0 = +0.0
              ([0, 1], [inf, 1]), ([0, 1], [inf, -inf]), ([0, 1, 2], [1, nan, 2]), ([3], [inf]), ([3, 0], [0.0, nan]),
              ([0, 1], [3e38, 3e38]),                   # overflows to inf
              ([0, 1], [1.0, -1.0])]                    # cancels: the entry stays, value 0
    a = csr_of([r[0] for r in a_rows], np.int32) + (np.concatenate([r[1] for r in a_rows]).astype(f),)
    orp, oci, ova = check_product(a, b, 4, 5)
    at3 = [int(np.flatnonzero(oci[orp[i]:orp[i + 1]] == 3)[0]) + orp[i] for i in range(len(a_rows))]
    v = ova[at3]
    assert v[:5].tolist() == [0, 1, 0, 2, 0]
    assert v[5] == 0 and np.signbit(v[5]) and v[6] == 0 and not np.signbit(v[6])
    assert v[7] == inf and np.isnan(v[8]) and np.isnan(v[9]) and v[10] == inf and np.isnan(v[11]) and v[12] == inf
    assert v[13] == 0 and orp[14] - orp[13] == 1
    assert oci[orp[10]:orp[11]].tolist() == [1, 3] and oci[orp[11]:orp[12]].tolist() == [1, 3] and ova[orp[11]] == 0


def test_b_with_unsorted_rows_and_operands_out_of_range():
    rng = np.random.default_rng(13)
    a = _random_csr(300, 200, 0.05, rng, repeats=True)
    b = _random_csr(200, 900, 0.08, rng)                # (_random_csr leaves the columns of a row in random order)
    assert np.any(np.diff(b[1])[np.diff(np.repeat(np.arange(200), np.diff(b[0]))) == 0] < 0)
    check_product(a, b, 200, 900)
    # columns of A outside [0, p), columns of B outside [0, n), row pointers outside their arrays: nothing, nothing out of bounds
    a_ci, b_ci = a[1].copy(), b[1].copy()
    a_ci[::17], a_ci[5::29] = -3, 200
    b_ci[::13], b_ci[3::31] = 900, -1
    a_rp, b_rp = a[0].copy(), b[0].copy()
    for rp, rows in ((a_rp, (4, 50)), (b_rp, (7, 120))):
        rp[rows[0] + 1] = len(a[1]) + len(b[1]) + 5     # rows r and r + 1 both unusable
        rp[rows[1] + 1] = -2
    ref = spgemm_ref(a_rp, a_ci, a[2], b_rp, b_ci, b[2], 200, 900)
    assert 0 < len(ref[1]) < len(spgemm_ref(*a, *b, 200, 900)[1]) and ref[0][5] == ref[0][4] and ref[0][6] == ref[0][5]
    check_product((a_rp, a_ci, a[2]), (b_rp, b_ci, b[2]), 200, 900, ref)


# ---- call mechanics ----------------------------------------------------------------------------------------------------------------
def small_pair():
    """400 x 300 · 300 x 700 with rows of two classes: short rows for the waves, and row 100 with more than W products"""
    if "small" not in _cache:
        rng = np.random.default_rng(14)
        a = _random_csr(400, 300, 0.03, rng, repeats=True)
        b = _random_csr(300, 700, 0.05, rng)
        rows = [a[1][a[0][i]:a[0][i + 1]] for i in range(400)]
        rows[100] = rng.integers(0, 300, 90)            # about 90 * 35 products on 700 columns
        a_rp, a_ci = csr_of(rows, np.int32)
        a = (a_rp, a_ci, rng.standard_normal(len(a_ci)).astype(np.float32))
        ref = spgemm_ref(*a, *b, 300, 700)
        assert min(ref[3][100], 700) > W and 0 < ref[3][99] <= W and ref[0][100] > ref[0][99]
        _cache["small"] = (a, b, ref)
    return _cache["small"]


def test_operands_off_the_grid_two_calls_and_a_side_stream():
    a, b, ref = small_pair()
    m, p, n = 400, 300, 700
    total = len(ref[1])
    # every operand 4 bytes past a 16-byte boundary, between guards
    ins = [offset_view(x, 1, dt, DEV) for x, dt in ((a[0], torch.int32), (a[1], torch.int32), (a[2], torch.float32),
                                                   (b[0], torch.int32), (b[1], torch.int32), (b[2], torch.float32))]
    da, db = tuple(v for v, _ in ins[:3]), tuple(v for v, _ in ins[3:])
    out_len = raw_count(da, db, m, p, n)
    assert np.array_equal(out_len.cpu().numpy(), np.diff(ref[0]))
    orpv, orpf = offset_view(ref[0], 1, torch.int32, DEV)
    (ociv, ocif), (ovav, ovaf) = offset_view(total, 1, torch.int32, DEV), offset_view(total, 1, torch.float32, DEV)
    assert all(v.data_ptr() % 16 == 4 for v in da + db + (orpv, ociv, ovav))
    raw_fill(da, db, m, p, n, orpv, ociv, ovav)
    assert np.array_equal(ociv.cpu().numpy(), ref[1]) and same_values(ovav.cpu().numpy(), ref[2])
    assert guards_intact(ocif, ociv) and guards_intact(ovaf, ovav) and guards_intact(orpf, orpv)
    assert all(guards_intact(flat, view) for view, flat in ins)
    # twice, and once on a side stream: the same bits
    adj_a = gcn_amd.CsrAdjacency(t(a[0]), t(a[1]), t(a[2]), (m, p), chunk_nnz=4096)
    adj_b = gcn_amd.CsrAdjacency(t(b[0]), t(b[1]), t(b[2]), (p, n))
    x = gcn_amd.spgemm(adj_a, adj_b, assume_coalesced=True)
    y = gcn_amd.spgemm(adj_a, adj_b, assume_coalesced=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        z = gcn_amd.spgemm(adj_a, adj_b, assume_coalesced=True)
    side.synchronize()
    for c in (y, z):
        assert torch.equal(x.rowptr, c.rowptr) and torch.equal(x.col, c.col) and torch.equal(x.val.view(torch.int32), c.val.view(torch.int32))
    assert np.array_equal(x.col.cpu().numpy(), ref[1]) and same_values(x.val.cpu().numpy(), ref[2])
    assert x.symmetric is False and x.chunk_nnz == 4096 and (x.m, x.n) == (m, n)


def test_fill_with_a_wrong_slot_writes_nothing_for_that_row():
    a, b, ref = small_pair()
    m, p, n = 400, 300, 700
    da, db = (tuple(t(x) for x in op) for op in (a, b))
    for bad in (99, 100):                               # a wave's row and a workgroup's row
        orp = ref[0].copy()
        orp[bad + 1:] += 1                              # the slot of row `bad` one too long; the rows behind it move up by one
        total = int(orp[-1])
        S = -7
        oci = torch.full((total,), S, dtype=torch.int32, device=DEV)
        ova = torch.full((total,), float(S), device=DEV)
        raw_fill(da, db, m, p, n, t(orp), oci, ova)
        lo, hi = int(orp[bad]), int(orp[bad + 1])
        oci, ova = oci.cpu().numpy(), ova.cpu().numpy()
        assert hi - lo > 1 and np.all(oci[lo:hi] == S) and np.all(ova[lo:hi] == S)
        cut = int(ref[0][bad]), int(ref[0][bad + 1])
        assert np.array_equal(oci[:lo], ref[1][:cut[0]]) and np.array_equal(oci[hi:], ref[1][cut[1]:])
        assert same_values(ova[:lo], ref[2][:cut[0]]) and same_values(ova[hi:], ref[2][cut[1]:])


def test_a_dense_row_with_a_wrong_slot_writes_nothing():
    a, b, p, ref = class_pair()
    m = len(a[0]) - 1
    bad = 0                                             # row 0 is in the dense class
    orp = ref[0].copy()
    orp[bad + 1:] += 1
    total = int(orp[-1])
    oci = torch.full((total,), -7, dtype=torch.int32, device=DEV)
    ova = torch.full((total,), -7.0, device=DEV)
    raw_fill(tuple(t(x) for x in a), tuple(t(x) for x in b), m, p, N, t(orp), oci, ova)
    hi = int(orp[1])
    oci, ova = oci.cpu().numpy(), ova.cpu().numpy()
    assert np.all(oci[:hi] == -7) and np.all(ova[:hi] == -7)
    assert np.array_equal(oci[hi:], ref[1][ref[0][1]:]) and same_values(ova[hi:], ref[2][ref[0][1]:])


# ---- gcn_amd.spgemm ----------------------------------------------------------------------------------------------------------------
def test_spgemm_against_scipy_and_with_a_b_that_repeats_pairs():
    rng = np.random.default_rng(15)
    n = 2000
    a = _random_csr(n, n, 8 / n, rng, repeats=True)
    b = _random_csr(n, n, 8 / n, rng, repeats=True)     # B repeats pairs: spgemm merges it first
    adj_a = gcn_amd.CsrAdjacency(t(a[0]), t(a[1]), t(a[2]), (n, n))
    adj_b = gcn_amd.CsrAdjacency(t(b[0]), t(b[1]), t(b[2]), (n, n))
    c = gcn_amd.spgemm(adj_a, adj_b)
    merged = sorted_merged_ref(*b)
    assert len(merged[1]) < len(b[1])
    d = gcn_amd.spgemm(adj_a, gcn_amd.CsrAdjacency(t(merged[0]), t(merged[1]), t(merged[2]), (n, n)), assume_coalesced=True)
    assert torch.equal(c.rowptr, d.rowptr) and torch.equal(c.col, d.col) and torch.equal(c.val.view(torch.int32), d.val.view(torch.int32))
    # against scipy: the merged B's values carry one rounding per merged pair already, so the bound is taken for A · merged B
    ref, bound = summation_bound(a, merged, (n, n), (n, n))
    assert np.array_equal(c.rowptr.cpu().numpy(), ref.indptr) and np.array_equal(c.col.cpu().numpy(), ref.indices) and c.nnz > 50000
    err = np.abs(c.val.cpu().numpy().astype(np.float64) - ref.data)
    print("largest error / bound", np.max(err / bound))
    assert np.all(err <= bound)
    twin = spgemm_ref(*a, *merged, n, n)
    assert same_values(c.val.cpu().numpy(), twin[2])


# ---- the hypergraph Laplacian ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_hypergraph_laplacian(weighted):
    rp, ci, va, dense, w = hypergraph_fixture()
    H = gcn_amd.CsrAdjacency(t(rp), t(ci), t(va), (40, 12))
    g = gcn_amd.hypergraph_laplacian(H, t(w) if weighted else None)
    grp, gci, gva = hypergraph_laplacian_ref(rp, ci, va, 12, w if weighted else None)
    assert (g.m, g.n, g.symmetric) == (40, 40, True)
    assert np.array_equal(g.rowptr.cpu().numpy(), grp) and np.array_equal(g.col.cpu().numpy(), gci)
    assert same_values(g.val.cpu().numpy(), gva)                          # the twin, bit for bit
    gt, _ = gcn_amd.transpose_csr(g)
    assert torch.equal(gt.rowptr, g.rowptr) and torch.equal(gt.col, g.col) and torch.equal(gt.val.view(torch.int32), g.val.view(torch.int32))
    ref = dense_g(dense, w.astype(np.float64) if weighted else np.ones(12))
    got = sp.csr_matrix((g.val.cpu().numpy(), gci, grp), shape=(40, 40)).toarray()
    d = shared_hyperedges(dense)
    err = np.abs(got - ref)
    print("largest relative error", (err[ref != 0] / ref[ref != 0]).max(), "bound", (d + 4) * U24)
    assert np.array_equal(got != 0, ref != 0) and np.all(err <= (d + 4) * U24 * ref)
    if weighted:
        return
    # into the SpMM at its tolerance, and through a layer against the dense computation
    k = 32
    X = np.random.default_rng(16).standard_normal((40, k)).astype(np.float32)
    assert rel_err(gcn_amd.spmm(g, t(X)).cpu().numpy(), oracle_spmm(grp, gci, gva, X)) <= TOL
    torch.manual_seed(0)
    layer = gcn_amd.GraphConvolution(k, 8).to(DEV)
    x = t(X).requires_grad_(True)
    out = layer(x, g)
    out.square().sum().backward()
    xr = t(X).double().requires_grad_(True)
    outr = t(ref) @ (xr @ layer.weight.detach().double()) + layer.bias.detach().double()
    outr.square().sum().backward()
    # (every product is within TOL by the suite's yardstick: the forward chains two of them, the backward three and the
    # factor 2 of the square — the bounds of tests/test_coalesce_gpu.py)
    assert rel_err(out.detach().cpu().numpy(), outr.detach().cpu().numpy()) <= 2 * TOL
    assert rel_err(x.grad.cpu().numpy(), xr.grad.cpu().numpy()) <= 4 * TOL
