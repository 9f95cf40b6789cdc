"""Stable bucketing, the device CSR transpose and CSR from an edge list on the GPU, bit for bit against the numpy twins of
tests/construct_ref.py: every ordering tier and both sides of each tier bound (read from gcn_amd._lib), off-grid operands, a
side stream, the transposes CsrAdjacency builds against the torch formulations they replace, and the gradients that ride
on them."""
import ctypes

import numpy as np
import pytest
import torch

import gcn_amd
from gcn_amd import _lib
from construct_ref import bucket_ref, csr_from_edges_ref, torch_coo_transpose, torch_transposed_pattern, transpose_ref
from util import elementwise_bound, guards_intact, offset_view, random_rows_csr

pytestmark = pytest.mark.gpu
DEV = "cuda"
WAVE, BLOCK = _lib.BUCKET_WAVE_MAX, _lib.BUCKET_BLOCK_MAX
_cache = {}


def keys_of_lengths(lens, order, seed=0):
    """keys with lens[b] entries of bucket b: ascending, descending or shuffled"""
    keys = np.repeat(np.arange(len(lens)), lens)
    if order == "reverse":
        keys = keys[::-1].copy()
    elif order == "random":
        keys = np.random.default_rng(seed).permutation(keys)
    return keys.astype(np.int64)


# one bucket of each length on both sides of every bound, four times the LDS tier's bound once, two long buckets side by side
TIER_LENS = [0, 1, 2, 63, 64, 65, WAVE - 1, WAVE, WAVE + 1, 0, BLOCK - 1, BLOCK, BLOCK + 1, 4 * BLOCK, 2 * BLOCK + 3, 1, 0, 5]


def check_bucket(keys, nbuckets, dtype=torch.int32):
    offsets, perm = gcn_amd.bucket_by_key(torch.from_numpy(keys).to(DEV, dtype), nbuckets)
    ref_off, ref_perm = bucket_ref(keys, nbuckets)
    assert offsets.dtype == torch.int32 and perm.dtype == torch.int32
    assert np.array_equal(offsets.cpu().numpy(), ref_off)
    got = perm.cpu().numpy()
    bad = np.flatnonzero(got != ref_perm)
    assert len(bad) == 0, f"perm differs at {len(bad)} of {len(got)} places, first {bad[0]} (bucket {keys[ref_perm[bad[0]]]})"
    return offsets, perm


@pytest.mark.parametrize("order", ["sorted", "reverse", "random"])
def test_every_tier_and_both_sides_of_every_bound_in_one_call(order):
    keys = keys_of_lengths(TIER_LENS, order, seed=1)
    assert keys.max() == len(TIER_LENS) - 1
    check_bucket(keys, len(TIER_LENS), torch.int64 if order == "random" else torch.int32)


@pytest.mark.parametrize("lens", [[0], [1], [2], [63], [64], [65], [WAVE - 1], [WAVE], [WAVE + 1], [BLOCK - 1], [BLOCK],
                                  [BLOCK + 1], [3 * BLOCK + 17, 2 * BLOCK + 1]], ids=str)
def test_single_lengths(lens):
    """nbuckets = 1 with every key 0 among them; the last: two long buckets next to each other"""
    check_bucket(keys_of_lengths(lens, "random", seed=2), len(lens))


def test_no_keys_and_almost_only_empty_buckets():
    offsets, perm = check_bucket(np.zeros(0, np.int64), 5)
    assert offsets.tolist() == [0] * 6 and perm.numel() == 0
    offsets, perm = check_bucket(np.zeros(0, np.int64), 0)
    assert offsets.tolist() == [0]
    rng = np.random.default_rng(3)
    keys = rng.integers(0, 100000, 50)
    keys[7] = 100000 - 1
    keys[11] = keys[12] = keys[40] = 31                # one bucket of three among the singles
    check_bucket(keys, 100000)
    for bad in ([0, 5], [-1, 2]):
        with pytest.raises(ValueError, match="keys must lie"):
            gcn_amd.bucket_by_key(torch.tensor(bad, device=DEV), 5)
    with pytest.raises(ValueError, match="keys must lie"):
        gcn_amd.bucket_by_key(torch.tensor([0], device=DEV), 0)


def test_many_short_buckets_and_a_hub():
    """what a transpose looks like: tens of thousands of buckets of a few entries (several waves of list per tier) and one
    hub bucket of 20 000, whose keys meet inside the waves of the count and the scatter"""
    rng = np.random.default_rng(4)
    keys = np.concatenate([rng.integers(0, 30000, 90000), np.full(20000, 12345)])
    check_bucket(rng.permutation(keys), 30000)
    check_bucket(np.sort(keys), 30000)


def _raw_bucket(keys_view, nbuckets, perm_view, stream=None):
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    count = keys_view.numel()
    st = ctypes.c_void_p(stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    offsets = torch.empty(nbuckets + 1, dtype=torch.int32, device=DEV)
    _lib.check(lib.gcn_bucket_count_i32(p(keys_view), count, nbuckets, p(offsets), st), "count")
    offsets.cumsum_(0)
    ws = torch.empty(_lib.bucket_ws_bytes(count, nbuckets), dtype=torch.uint8, device=DEV)
    _lib.check(lib.gcn_bucket_fill_i32(p(keys_view), count, nbuckets, p(offsets), p(perm_view), p(ws), ws.numel(), st), "fill")
    return offsets


def test_operands_one_element_off_the_grid():
    keys = keys_of_lengths([3, 0, WAVE + 5, 70, BLOCK + 9, 1], "random", seed=5)
    kv, kflat = offset_view(keys.astype(np.int32), 1, torch.int32, DEV)
    pv, pflat = offset_view(len(keys), 1, torch.int32, DEV)
    assert kv.data_ptr() % 16 == 4 and pv.data_ptr() % 16 == 4
    offsets = _raw_bucket(kv, 6, pv)
    ref_off, ref_perm = bucket_ref(keys, 6)
    assert np.array_equal(offsets.cpu().numpy(), ref_off) and np.array_equal(pv.cpu().numpy(), ref_perm)
    assert guards_intact(pflat, pv) and guards_intact(kflat, kv)


def test_two_calls_agree_and_a_side_stream_works():
    keys = keys_of_lengths([WAVE + 1, 2, 0, BLOCK + 1, 40, 1], "random", seed=6)
    kd = torch.from_numpy(keys).to(DEV)
    a = gcn_amd.bucket_by_key(kd, 6)
    b = gcn_amd.bucket_by_key(kd, 6)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = gcn_amd.bucket_by_key(kd, 6)
        k32 = kd.to(torch.int32)
        perm = torch.empty(len(keys), dtype=torch.int32, device=DEV)
        offsets = _raw_bucket(k32, 6, perm, stream=side)
    side.synchronize()
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]) and torch.equal(a[0], offsets) and torch.equal(a[1], perm)


# ---- transposes ----------------------------------------------------------------------------------------------------------------
def make_adj(rp, ci, m, n, seed=0, **kw):
    va = np.random.default_rng(seed).standard_normal(len(ci)).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(DEV)
    return gcn_amd.CsrAdjacency(t(rp), t(ci), t(va), (m, n), **kw), va


def hub_graph():
    """3 x BLOCK rows by 500 columns with repeated entries, empty rows and a hub column (column 0 leads two rows in three:
    more entries than the LDS tier holds)"""
    if "hub" not in _cache:
        m, n = 3 * BLOCK, 500
        lens = np.random.default_rng(7).integers(0, 6, m)
        rp, ci = random_rows_csr(m, n, lens, seed=8)
        ci[rp[:-1][(lens > 0) & (np.arange(m) % 3 != 1)]] = 0          # first entry of most rows: column 0 (rows stay sorted)
        rows = np.repeat(np.arange(m), np.diff(rp))
        assert np.bincount(ci, minlength=n).max() > BLOCK and len(np.unique(rows * n + ci)) < len(ci) and (lens == 0).any()
        _cache["hub"] = (rp, ci, m, n)
    return _cache["hub"]


@pytest.mark.parametrize("m, n, top", [(300, 70, 9), (70, 300, 40), (50, 1, 3), (1, 50, 30), (2000, 2000, 12)])
def test_transpose_csr_is_the_twin(m, n, top):
    lens = np.random.default_rng(m).integers(0, top, m)
    lens[m // 2] = 0 if m > 1 else 30
    rp, ci = random_rows_csr(m, n, lens, seed=n)
    adj, va = make_adj(rp, ci, m, n)
    t, eid = gcn_amd.transpose_csr(adj)
    trp, trow, tval, ref_eid = transpose_ref(rp, ci, va, n)
    assert (t.m, t.n, t.nnz, t.symmetric) == (n, m, len(ci), False) and eid.dtype == torch.int32
    assert np.array_equal(t.rowptr.cpu().numpy(), trp) and np.array_equal(t.col.cpu().numpy(), trow)
    assert np.array_equal(eid.cpu().numpy(), ref_eid)
    assert np.array_equal(t.val.cpu().numpy().view(np.int32), tval.view(np.int32))
    # the transpose of the transpose: entry t is entry eid[eid2[t]] of adj, and adj's rows are column-sorted, so it is adj
    tt, eid2 = gcn_amd.transpose_csr(t)
    assert torch.equal(eid[eid2.long()], torch.arange(len(ci), dtype=torch.int32, device=DEV))
    assert torch.equal(tt.rowptr, adj.rowptr) and torch.equal(tt.col, adj.col) and torch.equal(tt.val, adj.val)


def test_transpose_csr_of_nothing():
    z = lambda *s: torch.zeros(*s, dtype=torch.int32, device=DEV)
    adj = gcn_amd.CsrAdjacency(z(4), z(0), torch.zeros(0, device=DEV), (3, 5))
    t, eid = gcn_amd.transpose_csr(adj)
    assert t.rowptr.tolist() == [0] * 6 and t.nnz == 0 and eid.numel() == 0 and (t.m, t.n) == (5, 3)


def test_transposed_pattern_is_the_torch_formulation_it_replaces():
    rp, ci, m, n = hub_graph()
    adj, _ = make_adj(rp, ci, m, n)
    new, old = adj._transposed_pattern(), torch_transposed_pattern(adj)
    for a, b in zip(new, old):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert [a.dtype for a in new] == [torch.int32, torch.int32, torch.int64]
    mut, va = make_adj(rp[:200], ci[:rp[199]], 199, n, mutable_values=True)
    t = mut.transpose()                                # the mutable transpose rides on the same pattern
    tperm = mut.tpattern()[2].long()
    assert torch.equal(t.val, mut.val[tperm]) and torch.equal(tperm, torch_transposed_pattern(mut)[2])


def test_transpose_of_a_duplicate_free_bipartite_matrix_is_the_coo_round_trip():
    m, n = 700, 1900
    rng = np.random.default_rng(9)
    lens = rng.integers(0, 25, m)
    rp = np.zeros(m + 1, np.int32)
    rp[1:] = np.cumsum(lens)
    ci = np.concatenate([np.sort(rng.choice(n, l, replace=False)) for l in lens]).astype(np.int32)
    adj, _ = make_adj(rp, ci, m, n, symmetric=False)
    t = adj.transpose()
    orp, oci, ova = torch_coo_transpose(adj)
    assert t.transpose() is adj and (t.m, t.n) == (n, m)
    assert torch.equal(t.rowptr, orp.to(torch.int32)) and torch.equal(t.col, oci.to(torch.int32))
    assert torch.equal(t.val.view(torch.int32), ova.view(torch.int32))


# ---- edge lists ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort_columns", [True, False])
@pytest.mark.parametrize("values", [None, "tensor", "gcn"])
def test_csr_from_edges_is_the_twin(sort_columns, values):
    n = 400
    rng = np.random.default_rng(10)
    rows, cols = rng.integers(0, n, 6000), rng.integers(0, n, 6000)
    rows[100], cols[100] = rows[5], cols[5]            # a repeated edge, and a row and a column without edges
    keep = (rows != 17) & (cols != 23)
    rows, cols = rows[keep], cols[keep]
    vals = rng.standard_normal(len(rows)).astype(np.float32)
    v_in = {None: None, "tensor": torch.from_numpy(vals).to(DEV), "gcn": "gcn"}[values]
    v_ref = {None: None, "tensor": vals, "gcn": "gcn"}[values]
    dt = torch.int64 if sort_columns else torch.int32
    adj, eid = gcn_amd.csr_from_edges(torch.from_numpy(rows).to(DEV, dt), torch.from_numpy(cols).to(DEV), (n, n), v_in, sort_columns)
    rrp, rci, rva, reid = csr_from_edges_ref(rows, cols, (n, n), v_ref, sort_columns)
    assert (adj.m, adj.n, adj.nnz) == (n, n, len(rows)) and eid.dtype == torch.int32
    assert np.array_equal(adj.rowptr.cpu().numpy(), rrp) and np.array_equal(adj.col.cpu().numpy(), rci)
    assert np.array_equal(eid.cpu().numpy(), reid)
    got = adj.val.cpu().numpy()
    if values == "gcn":                                # (rsqrt of an fp64 product, rounded to fp32: one more rounding than 1 / sqrt)
        assert np.allclose(got, rva, rtol=2 ** -22, atol=0)
    else:
        assert np.array_equal(got.view(np.int32), rva.view(np.int32))
    if sort_columns:
        assert np.array_equal(reid, np.lexsort((cols, rows)))


def test_csr_from_edges_rectangular_empty_and_out_of_range():
    rows, cols = np.array([2, 0, 2, 2, 0]), np.array([8, 3, 1, 8, 3])
    adj, eid = gcn_amd.csr_from_edges(torch.from_numpy(rows).to(DEV), torch.from_numpy(cols).to(DEV), (4, 9))
    assert adj.rowptr.tolist() == [0, 2, 2, 5, 5] and adj.col.tolist() == [3, 3, 1, 8, 8] and eid.tolist() == [1, 4, 2, 0, 3]
    assert adj.val.tolist() == [1.0] * 5 and adj.symmetric is False
    x = torch.eye(9, device=DEV)
    dense = gcn_amd.spmm(adj, x)                       # repeated edges add
    assert dense[0, 3] == 2 and dense[2, 8] == 2 and dense[2, 1] == 1 and float(dense.sum()) == 5
    e = torch.zeros(0, dtype=torch.int64, device=DEV)
    adj, eid = gcn_amd.csr_from_edges(e, e, (3, 4))
    assert adj.rowptr.tolist() == [0, 0, 0, 0] and adj.nnz == 0 and eid.numel() == 0
    r, c = torch.tensor([0, 3], device=DEV), torch.tensor([1, 2], device=DEV)
    for rr, cc, shape in ((r, c, (3, 4)), (c, r, (4, 3)), (r - 1, c, (4, 4)), (r, c - 2, (4, 4)), (r, c, (0, 4))):
        with pytest.raises(ValueError, match="must lie in"):
            gcn_amd.csr_from_edges(rr, cc, shape)


# ---- gradients that ride on the transposes ---------------------------------------------------------------------------------------
def _bipartite_7x19():
    rng = np.random.default_rng(11)
    lens = np.array([3, 0, 5, 1, 4, 2, 6])
    rp, ci = random_rows_csr(7, 19, lens, seed=12)
    ci[rp[2] + 1] = ci[rp[2]]                          # a repeated entry (the row stays column-sorted)
    va = rng.standard_normal(len(ci)).astype(np.float32)
    return rp, ci, va


def test_spmm_gradient_through_the_device_transpose_matches_dense_fp64():
    rp, ci, va = _bipartite_7x19()
    t = lambda a: torch.from_numpy(a).to(DEV)
    adj = gcn_amd.CsrAdjacency(t(rp), t(ci), t(va), (7, 19), symmetric=False)
    x = torch.randn(19, 8, generator=torch.Generator().manual_seed(1)).to(DEV).requires_grad_(True)
    gout = torch.randn(7, 8, generator=torch.Generator().manual_seed(2)).to(DEV)
    out = gcn_amd.spmm(adj, x)
    out.backward(gout)
    dense = np.zeros((7, 19))
    np.add.at(dense, (np.repeat(np.arange(7), np.diff(rp)), ci), va.astype(np.float64))
    mag = np.abs(dense).T @ np.abs(gout.cpu().numpy().astype(np.float64))
    ref = dense.T @ gout.cpu().numpy().astype(np.float64)
    bound = elementwise_bound(transpose_ref(rp, ci, va, 19)[0], mag)      # the element-wise bound of the SpMM tests, on Âᵀ's rows
    assert np.all(np.abs(x.grad.cpu().numpy().astype(np.float64) - ref) <= bound)
    assert np.allclose(out.detach().cpu().numpy(), dense @ x.detach().cpu().numpy().astype(np.float64), rtol=1e-5, atol=1e-6)
    x.grad = None
    gcn_amd.spmm(adj, x).sum().backward()
    assert np.allclose(x.grad.cpu().numpy(), np.repeat(dense.sum(0)[:, None], 8, 1), rtol=1e-5, atol=1e-6)


def test_max_aggregation_gradient_through_the_device_transpose_is_exact():
    """the reference of tests/test_aggregate_gpu.py: gx[col[arg[r, j]], j] += g[r, j], with small-integer gradients whose
    fp32 sums are exact in any order"""
    rp, ci, va = _bipartite_7x19()
    t = lambda a: torch.from_numpy(a).to(DEV)
    adj = gcn_amd.CsrAdjacency(t(rp), t(ci), t(va), (7, 19), symmetric=False)
    xs = np.random.default_rng(13).integers(-2, 3, (19, 5)).astype(np.float32)
    g = np.random.default_rng(14).integers(-8, 9, (7, 5)).astype(np.float32)
    x = t(xs).requires_grad_(True)
    out, arg = gcn_amd.aggregate(adj, x, "max", return_arg=True)
    out.backward(t(g))
    a = arg.cpu().numpy()
    ref = np.zeros((19, 5))
    rr, jj = np.nonzero(a >= 0)
    np.add.at(ref, (ci[a[rr, jj]], jj), g[rr, jj].astype(np.float64))
    for r in range(7):                                 # (arg is the first maximum of the row's slab)
        if rp[r + 1] > rp[r]:
            assert np.array_equal(a[r], rp[r] + np.argmax(xs[ci[rp[r]:rp[r + 1]]], axis=0))
    assert np.array_equal(x.grad.cpu().numpy().astype(np.float64), ref)
