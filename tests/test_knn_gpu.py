"""gcn_knn_f32 on the GPU against the numpy twin of tests/knn_ref.py — on integer features, where every distance is exact in
fp32 whatever the order, indices and distances bit for bit: both sides of the query tile, the candidate tile, the feature
chunk and k; lattices and identical points, where only the index decides; candidate orders that make every tile, no tile or
one key per tile pass the threshold; every split count; float inputs for symmetry, the zero diagonal and the error bound;
self exclusion, tails, NaN rows, empty operands; off-grid operands and strides, guards, a side stream, refused arguments,
graph capture — then gcn_amd.knn / knn_graph / knn_hypergraph, on to the SpMM and to the hypergraph Laplacian."""
import ctypes
import glob
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gcn_amd
from gcn_amd import _lib
from knn_ref import dist2_f64, dist2_ref, knn_ref
from test_spgemm_cpu import U24, summation_bound
from test_spmm_gpu import TOL
from util import GOLDEN, guards_intact, offset_view, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
KMAX = _lib.KNN_K_MAX
INVALID = 1
U53 = 2.0 ** -53
GOLDEN_FILES = sorted(glob.glob(os.path.join(GOLDEN, "knn_hypergraph_*.npz")))


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _p(x):
    return ctypes.c_void_p(x.data_ptr()) if x is not None else None


def raw(x, y, k, self_offset=-1, splits=0, ldx=None, ldy=None, d=None, out=None, stream=None):
    """one gcn_knn_f32 call on device tensors -> (idx int32 [q, k], dist2 fp32 [q, k], sum fp64 [q]) as numpy arrays, or the
    tensors of `out` = (idx, dist2, sum) filled in place"""
    q, n = x.shape[0], y.shape[0]
    d = x.shape[1] if d is None else d
    lib = _lib.load()
    nbytes = ctypes.c_size_t(0)
    _lib.check(lib.gcn_knn_ws_bytes(q, n, k, splits, ctypes.byref(nbytes)), "ws_bytes")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=DEV)
    if out is None:
        out = (torch.full((q, k), -7, dtype=torch.int32, device=DEV), torch.full((q, k), -7.0, dtype=torch.float32, device=DEV),
               torch.full((q,), -7.0, dtype=torch.float64, device=DEV))
    s = stream if stream is not None else torch.cuda.current_stream()
    st = lib.gcn_knn_f32(_p(x), ldx or max(x.stride(0), d), _p(y), ldy or max(y.stride(0), d), q, n, d, k, self_offset, splits,
                         _p(out[0]), _p(out[1]), _p(out[2]), _p(ws), ws.numel(), ctypes.c_void_p(s.cuda_stream))
    _lib.check(st, "gcn_knn_f32")
    s.synchronize()
    return tuple(o.cpu().numpy() if o is not None else None for o in out)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def sums_agree(got, want, n, terms=2):
    """two fp64 sums of the same n non-negative terms in different orders: each is within (n - 1) * 2^-53 of the exact sum,
    and a term (an fp64 square root) within one more rounding: (2 n + 2) * 2^-53 relative between them (`terms` = 1: the
    terms are the same bits, n * 2^-53 as the contract states)"""
    bound = (2 * n + 2) * U53 if terms == 2 else n * U53
    return bool(np.all(np.abs(got - want) <= bound * np.abs(want)))


def check_against_twin(x, y, k, self_offset=-1, splits=0, what=""):
    idx, d2, rsum = raw(t(x), t(y), k, self_offset, splits)
    ridx, rd2, rsum_ref = knn_ref(x, y, k, self_offset)
    assert np.array_equal(idx, ridx), what
    assert same_bits(d2, rd2), what
    assert sums_agree(rsum, rsum_ref, y.shape[0]), what
    return idx, d2


# (q, n, d, k): every value of every axis, each tile edge with its neighbours, n = k - 1 and n = k
CASES = [(1, 1, 1, 1), (63, 63, 31, 10), (64, 64, 32, 2), (65, 65, 33, 10), (130, 200, 64, KMAX), (65, 1000, 3, 10),
         (64, 9, 32, 10), (63, 10, 33, 10), (130, KMAX - 1, 3, KMAX), (1, KMAX, 1, KMAX), (65, 200, 31, 2), (130, 1000, 33, KMAX),
         (64, 65, 64, 1), (1, 1000, 32, 10), (130, 1, 64, 2)]


def int_points(rows, d, seed):
    return np.random.default_rng(seed).integers(-8, 9, (rows, d)).astype(np.float32)


def lattice_points(rows, d, shift=0):
    """a 7 x 5 integer lattice visited over and over (dozens of candidates tie at every distance, and every point repeats);
    with d == 1 a line of 7; the columns past the second hold a constant"""
    i = np.arange(rows) + shift
    p = np.full((rows, d), 3.0, np.float32)
    p[:, 0] = i % 7
    if d > 1:
        p[:, 1] = (i // 7) % 5
    return p


@pytest.mark.parametrize("q, n, d, k", CASES)
def test_exact_arithmetic_matches_the_twin_bit_for_bit(q, n, d, k):
    for self_offset in (-1, 0):
        check_against_twin(int_points(q, d, 1), int_points(n, d, 2), k, self_offset, what=("int", self_offset))
        check_against_twin(lattice_points(q, d, 3), lattice_points(n, d), k, self_offset, what=("lattice", self_offset))
        same = np.tile(int_points(1, d, 4), (max(q, n), 1))
        idx, d2 = check_against_twin(same[:q], same[:n], k, self_offset, what=("identical", self_offset))
        for i in (0, q - 1):                              # identical points: the indices alone decide
            want = [j for j in range(n) if self_offset < 0 or j != i][:k]
            assert idx[i].tolist() == want + [-1] * (k - len(want)) and np.all(d2[i, :len(want)] == 0)


@pytest.mark.parametrize("k", [10, KMAX])
@pytest.mark.parametrize("order", ["descending", "ascending", "one_per_tile"])
def test_adversarial_candidate_orders(order, k):
    """a 1-D line, queries at -i: `descending` sorts the candidates by falling distance to every query (every tile beats the
    threshold, every tile compacts), `ascending` lets nothing pass after the first tiles, `one_per_tile` has one improving
    candidate in every tile of 64"""
    n, q = 1000, 65
    x = -np.arange(q, dtype=np.float32)[:, None]
    j = np.arange(n, dtype=np.float32)
    if order == "descending":
        y = 1000 - j
    elif order == "ascending":
        y = 1 + j
    else:
        y = 3000 + j
        tiles = np.arange((n + 63) // 64)
        y[np.minimum(tiles * 64 + 17, n - 1)] = 2000 - 10 * tiles
    for splits in (1, 2):
        idx, _ = check_against_twin(x, y[:, None].astype(np.float32), k, splits=splits, what=(order, splits))
    if order == "descending":
        assert idx[0].tolist() == list(range(n - 1, n - 1 - k, -1))


def test_split_invariance_and_repeatable_sums():
    rng = np.random.default_rng(7)
    n, q, d, k = 1000, 130, 33, 10
    y = rng.standard_normal((n, d)).astype(np.float32)
    x = rng.standard_normal((q, d)).astype(np.float32)
    xd, yd = t(x), t(y)
    base = raw(xd, yd, k, splits=1)
    ridx, rd2, _ = knn_ref(x, y, k)
    assert np.array_equal(base[0], ridx) and same_bits(base[1], rd2)      # (the twin's chain, on floats too)
    for splits in (2, 3, 7, 1000):
        assert _lib.load().gcn_knn_splits(q, n, splits) == min(splits, 16)
        got = raw(xd, yd, k, splits=splits)
        again = raw(xd, yd, k, splits=splits)
        assert np.array_equal(got[0], base[0]) and same_bits(got[1], base[1]), splits
        assert sums_agree(got[2], base[2], n, terms=1), splits
        assert np.array_equal(got[2].view(np.int64), again[2].view(np.int64)), splits


@pytest.mark.parametrize("d", [3, 33, 100])
def test_float_inputs_symmetry_error_bound_and_selection(d):
    n, k = 500, 10
    x = np.random.default_rng(d).standard_normal((n, d)).astype(np.float32)
    xd = t(x)
    D = np.empty((n, n), np.float32)                     # the whole matrix, 64 candidates at a time (all of them returned)
    for j0 in range(0, n, 64):
        part = x[j0:j0 + 64]
        idx, d2, _ = raw(xd, t(part), len(part), splits=1)
        assert np.array_equal(np.sort(idx, axis=1), np.tile(np.arange(len(part)), (n, 1)))
        np.put_along_axis(D[:, j0:j0 + 64], idx.astype(np.int64), d2, axis=1)
    assert same_bits(D, np.ascontiguousarray(D.T))       # d2(a, b) and d2(b, a): the same bits
    assert np.all(D.diagonal() == 0)
    assert same_bits(D, dist2_ref(x, x))
    ref = dist2_f64(x)
    rtol = (d + 4) * U24
    err = np.abs(D - ref) / np.where(ref > 0, ref, 1)
    print("largest relative distance error", err.max(), "bound", rtol)
    assert err.max() <= rtol
    idx, d2, _ = raw(xd, xd, k, self_offset=0)
    rows = np.arange(n)[:, None]
    assert same_bits(d2, D[rows, idx])                    # the tile a pair falls into does not change its distance
    keys = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
    assert np.all(keys[:, 1:] > keys[:, :-1])            # rows ascend by (distance, index)
    other = ref + np.diag(np.full(n, np.inf))
    kth = np.sort(other, axis=1)[:, k - 1:k]
    assert np.all(other[rows, idx] <= kth * (1 + 2 * rtol))
    must = other < kth * (1 - 2 * rtol)
    got = np.zeros((n, n), bool)
    got[rows, idx] = True
    assert np.all(got[must]) and not got.diagonal().any()


def test_self_exclusion_offsets_tails_and_nan_rows():
    y = int_points(200, 5, 11)
    y[50] = y[3]                                          # duplicates: distance 0 to another point
    for off in (0, 37):
        x = y[off:off + 70]
        idx, d2 = check_against_twin(x, y, 10, self_offset=off, what=off)
        assert not np.any(idx == np.arange(off, off + 70)[:, None])
    assert raw(t(y[3:4]), t(y), 2, self_offset=3)[0].tolist() == [[50, raw(t(y[3:4]), t(y), 3)[0][0, 2]]]
    idx, d2 = check_against_twin(y[:5], y[:5], 10, self_offset=0)       # n - 1 < k: the tail is -1 / +inf
    assert np.all(idx[:, 4:] == -1) and np.all(np.isposinf(d2[:, 4:])) and np.all(idx[:, :4] >= 0)
    z = y[:50].copy()
    z[7, 2] = np.nan
    idx, d2, rsum = raw(t(z), t(z), 10, self_offset=0)
    ridx, rd2, _ = knn_ref(z, z, 10, 0)
    assert np.array_equal(idx, ridx) and same_bits(d2, rd2)
    assert idx[7].tolist() == [0, 1, 2, 3, 4, 5, 6, 8, 9, 10] and np.isnan(d2[7]).all()      # every distance ties at NaN
    assert not np.any(np.delete(idx, 7, axis=0) == 7) and np.isnan(rsum).all()
    z = z[:9]
    z.view(np.uint32)[7, 2] |= 0x80000000                 # (the other sign bit)
    idx, d2, _ = raw(t(z), t(z), 8, self_offset=0)
    ridx, rd2, _ = knn_ref(z, z, 8, 0)
    assert np.array_equal(idx, ridx) and same_bits(d2, rd2)
    for i in range(9):                                    # as a candidate the NaN row ranks behind every number
        if i != 7:
            assert idx[i, 7] == 7 and np.isnan(d2[i, 7]) and not np.isnan(d2[i, :7]).any()


def test_empty_operands():
    x = t(int_points(70, 4, 1))
    idx, d2, rsum = raw(x, torch.empty((0, 4), dtype=torch.float32, device=DEV), 3, self_offset=0)
    assert np.all(idx == -1) and np.all(np.isposinf(d2)) and np.all(rsum == 0)
    idx, d2, rsum = raw(x[:0], x, 3)
    assert idx.shape == (0, 3)
    lib = _lib.load()
    assert lib.gcn_knn_f32(None, 4, _p(x), 4, 0, 70, 4, 3, -1, 0, None, None, None, None, 0, None) == 0


def _guarded_outputs(q, k):
    idx, fi = offset_view((q, k), 1, torch.int32, DEV)
    d2, fd = offset_view((q, k), 3, torch.float32, DEV)
    si, fs = offset_view((2 * q,), 2, torch.int32, DEV)  # fp64 sums behind int32 guards, 8-byte aligned
    return (idx, d2, si.view(torch.float64)), ((fi, idx), (fd, d2), (fs, si))


@pytest.mark.parametrize("side_stream", [False, True])
def test_offset_operands_strides_guards_and_streams(side_stream):
    q, n, d, k = 70, 150, 5, 12
    x, y = int_points(q, d, 21), int_points(n, d, 22)
    xp = np.full((q, 9), 99.0, np.float32)                # row strides larger than d; the padding would change every distance
    yp = np.full((n, 7), -99.0, np.float32)
    xp[:, :d], yp[:, :d] = x, y
    xv, _ = offset_view(xp, 1, torch.float32, DEV)        # 4-byte aligned, not 16
    yv, _ = offset_view(yp, 3, torch.float32, DEV)
    out, guards = _guarded_outputs(q, k)
    ridx, rd2, rsum = knn_ref(x, y, k)
    stream = torch.cuda.Stream() if side_stream else None
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    for splits in (1, 3):
        idx, d2, s = raw(xv, yv, k, splits=splits, ldx=9, ldy=7, d=d, out=out, stream=stream)
        assert np.array_equal(idx, ridx) and same_bits(d2, rd2) and sums_agree(s, rsum, n)
        assert all(guards_intact(flat, view) for flat, view in guards)
    xs = t(xp)[:, :d]                                     # the Python layer passes such a view by its stride
    assert not xs.is_contiguous()
    pidx, pd2 = gcn_amd.knn(xs, k, y=t(yp)[:, :d])
    assert np.array_equal(pidx.cpu().numpy(), ridx) and same_bits(pd2.cpu().numpy(), rd2)


def test_invalid_arguments_leave_the_outputs_untouched():
    q, n, d, k = 10, 20, 4, 3
    x, y = t(int_points(q, d, 1)), t(int_points(n, d, 2))
    out, guards = _guarded_outputs(q, k)
    before = [flat.clone() for flat, _ in guards]
    ws = torch.empty(_lib.knn_ws_bytes(q, n, k, 1), dtype=torch.uint8, device=DEV)
    good = [_p(x), d, _p(y), d, q, n, d, k, -1, 1, _p(out[0]), _p(out[1]), _p(out[2]), _p(ws), ws.numel(), None]
    lib = _lib.load()
    for i, bad in ((4, -1), (5, -1), (6, 0), (7, 0), (7, KMAX + 1), (1, d - 1), (3, d - 1), (8, -2), (9, -1), (0, None), (2, None),
                   (10, None), (13, None), (14, ws.numel() - 1)):
        args = list(good)
        args[i] = bad
        assert lib.gcn_knn_f32(*args) == INVALID, (i, bad)
    torch.cuda.synchronize()
    assert all(torch.equal(flat.view(torch.int32), b.view(torch.int32)) for (flat, _), b in zip(guards, before))   # (NaN sentinels)


def test_graph_capture_replays_on_changed_inputs():
    q, n, d, k, splits = 70, 300, 9, 10, 3
    x, y = t(int_points(q, d, 31)), t(int_points(n, d, 32))
    out = (torch.empty((q, k), dtype=torch.int32, device=DEV), torch.empty((q, k), dtype=torch.float32, device=DEV),
           torch.empty(q, dtype=torch.float64, device=DEV))
    ws = torch.empty(_lib.knn_ws_bytes(q, n, k, splits), dtype=torch.uint8, device=DEV)
    lib = _lib.load()

    def call(stream):
        _lib.check(lib.gcn_knn_f32(_p(x), d, _p(y), d, q, n, d, k, -1, splits, _p(out[0]), _p(out[1]), _p(out[2]), _p(ws),
                                   ws.numel(), ctypes.c_void_p(stream.cuda_stream)), "gcn_knn_f32")

    call(torch.cuda.current_stream())                     # (eager first: nothing is set up under capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(torch.cuda.current_stream())
    for seed in (41, 42):
        x.copy_(t(int_points(q, d, seed)))
        y.copy_(t(int_points(n, d, seed + 10)))
        for o in out:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        eager = raw(x, y, k, splits=splits)
        assert np.array_equal(out[0].cpu().numpy(), eager[0]) and same_bits(out[1].cpu().numpy(), eager[1])
        assert np.array_equal(out[2].cpu().numpy().view(np.int64), eager[2].view(np.int64))


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
def test_knn_matches_the_raw_call():
    x, y = int_points(130, 6, 51), int_points(300, 6, 52)
    xd, yd = t(x), t(y)
    for kwargs, off in (({}, -1), ({"exclude_self": True, "self_offset": 5}, 5), ({"splits": 4}, -1)):
        idx, d2 = gcn_amd.knn(xd, 7, y=yd, **kwargs)
        ridx, rd2, _ = raw(xd, yd, 7, self_offset=off)
        assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and idx.shape == (130, 7)
        assert np.array_equal(idx.cpu().numpy(), ridx) and same_bits(d2.cpu().numpy(), rd2)
    idx, d2 = gcn_amd.knn(yd, 7, exclude_self=True)
    ridx, rd2, _ = raw(yd, yd, 7, self_offset=0)
    assert np.array_equal(idx.cpu().numpy(), ridx) and same_bits(d2.cpu().numpy(), rd2)
    idx, _ = gcn_amd.knn(yd.t().contiguous().t(), 7)      # column-major rows are made contiguous
    assert np.array_equal(idx.cpu().numpy(), raw(yd, yd, 7)[0])
    assert gcn_amd.knn(yd[:0], 3, y=yd)[0].shape == (0, 3)


@pytest.mark.parametrize("loop", [False, True])
def test_knn_graph_rows_columns_and_values(loop):
    x = np.random.default_rng(61).standard_normal((150, 4)).astype(np.float32)
    x[20] = x[3]
    k = 6
    adj = gcn_amd.knn_graph(t(x), k, loop=loop, values="distance")
    ones = gcn_amd.knn_graph(t(x), k, loop=loop)
    rp, ci, va = adj.rowptr.cpu().numpy(), adj.col.cpu().numpy().reshape(150, k), adj.val.cpu().numpy().reshape(150, k)
    assert (adj.m, adj.n, adj.symmetric) == (150, 150, False) and np.array_equal(rp, np.arange(151) * k)
    assert torch.equal(ones.col, adj.col) and torch.all(ones.val == 1)
    assert np.all(ci[:, 1:] > ci[:, :-1])                # columns ascend
    ridx, rd2, _ = knn_ref(x, x, k, -1 if loop else 0)
    order = np.argsort(ridx, axis=1)
    assert np.array_equal(ci, np.take_along_axis(ridx, order, axis=1))
    want = np.sqrt(np.take_along_axis(rd2, order, axis=1))
    assert np.all(np.abs(va - want) <= 2 * U24 * want)   # (an fp32 square root, whoever takes it, is within an ulp)
    has_self = (ci == np.arange(150)[:, None]).any(axis=1)
    assert has_self.all() if loop else not has_self.any()
    few = gcn_amd.knn_graph(t(x[:4]), k, loop=loop)      # min(k, n - 1) or min(k, n) entries per row
    assert np.array_equal(few.rowptr.cpu().numpy(), np.arange(5) * (4 if loop else 3))


def test_knn_graph_feeds_the_spmm_through_the_existing_merge():
    rng = np.random.default_rng(71)
    n, k = 300, 8
    x = rng.standard_normal((n, 3)).astype(np.float32)
    adj = gcn_amd.normalize_csr(gcn_amd.symmetrize(gcn_amd.knn_graph(t(x), k)), "sym")
    ridx, _, _ = knn_ref(x, x, k, 0)
    A = np.zeros((n, n))
    A[np.arange(n)[:, None], ridx] = 1
    A = np.maximum(A, A.T)
    deg = A.sum(axis=1)
    ref_adj = A / np.sqrt(deg)[:, None] / np.sqrt(deg)[None, :]
    got = sp.csr_matrix((adj.val.cpu().numpy(), adj.col.cpu().numpy(), adj.rowptr.cpu().numpy()), shape=(n, n))
    assert np.array_equal(got.toarray() != 0, A != 0)
    B = rng.standard_normal((n, 16)).astype(np.float32)
    C = gcn_amd.spmm(adj, t(B)).cpu().numpy()
    assert rel_err(C, ref_adj @ B.astype(np.float64)) <= TOL


def _dense(adj):
    return sp.csr_matrix((adj.val.cpu().numpy().astype(np.float64), adj.col.cpu().numpy(), adj.rowptr.cpu().numpy()),
                         shape=(adj.m, adj.n)).toarray()


def _h_bound(d):
    """the relative bound of an entry of H: the value is exp(-a), a = d2 / avg^2.  d2 is within r = (d + 4) * 2^-24 of exact;
    a distance sqrt(d2) within r / 2, and so is their mean avg, so avg^2 within r: a is within 2 r, and exp(-a) within
    2 r * a <= 2 r, because a member of a hyperedge is nearer to the centre than the mean vertex (a <= 1, asserted).  The
    rounding of the value to fp32 (2^-24 <= r / 4) and the second-order terms fit into one more r, and one is spare: 4 r."""
    return 4 * (d + 4) * U24


@pytest.mark.parametrize("path", GOLDEN_FILES, ids=[os.path.basename(f)[:-4] for f in GOLDEN_FILES])
def test_knn_hypergraph_and_laplacian_against_the_recorded_reference(path):
    z = np.load(path)
    x, k, Href, Gref = z["x"], int(z["k"]), z["H"], z["G"]
    n, d = x.shape
    H = gcn_amd.knn_hypergraph(t(x), k)
    assert (H.m, H.n, H.symmetric) == (n, n, False)
    got = _dense(H)
    assert np.array_equal(got != 0, Href != 0) and H.nnz == n * k
    assert np.all(-np.log(Href[Href != 0]) <= 1)         # a <= 1: what _h_bound assumes
    rel = np.abs(got - Href)[Href != 0] / Href[Href != 0]
    print("H: largest relative error", rel.max(), "bound", _h_bound(d))
    assert rel.max() <= _h_bound(d) and np.all(got.diagonal() == 1)
    col = H.col.cpu().numpy()
    rp = H.rowptr.cpu().numpy()
    assert all(np.all(np.diff(col[rp[i]:rp[i + 1]]) > 0) for i in range(n))
    binary = gcn_amd.knn_hypergraph(t(x), k, prob=False)
    assert torch.equal(binary.col, H.col) and torch.all(binary.val == 1)
    # G on the device, end to end, against the recorded G: the summation bound of the product L · Lᵀ (L as the device
    # rounds it) plus what the error of H does to an entry — every factor h / sqrt(Dv) * sqrt(1 / De) moves by at most the H
    # bound (h itself; Dv and De are sums of such h, their roots move by half of it each), two factors per product
    g = gcn_amd.hypergraph_laplacian(H)
    gd = _dense(g)
    dv, de = got.sum(axis=1), got.sum(axis=0)
    L = sp.csr_matrix((got / np.sqrt(dv)[:, None] * np.sqrt(1 / de)[None, :]).astype(np.float32))
    L.sort_indices()
    Lt = L.T.tocsr()
    Lt.sort_indices()
    ref, bound = summation_bound((L.indptr, L.indices, L.data), (Lt.indptr, Lt.indices, Lt.data), (n, n), (n, n))
    assert np.array_equal(gd != 0, Gref != 0) and np.array_equal(ref.toarray() != 0, Gref != 0)
    total = np.zeros((n, n))
    total[Gref != 0] = bound + (4 * _h_bound(d) + 4 * U24) * Gref[Gref != 0]
    print("G: largest error / bound", (np.abs(gd - Gref)[Gref != 0] / total[Gref != 0]).max())
    assert np.all(np.abs(gd - Gref) <= total)
    gt, _ = gcn_amd.transpose_csr(g)
    assert torch.equal(gt.rowptr, g.rowptr) and torch.equal(gt.col, g.col)
    assert torch.equal(gt.val.view(torch.int32), g.val.view(torch.int32))          # G equals its transpose bit for bit


def test_knn_hypergraph_with_a_list_of_k_is_the_groups_side_by_side():
    x = np.load(GOLDEN_FILES[0])["x"]
    n = x.shape[0]
    both = _dense(gcn_amd.knn_hypergraph(t(x), [5, 10]))
    assert both.shape == (n, 2 * n)
    assert np.array_equal(both[:, :n], _dense(gcn_amd.knn_hypergraph(t(x), 5)))
    assert np.array_equal(both[:, n:], _dense(gcn_amd.knn_hypergraph(t(x), 10)))
    one = _dense(gcn_amd.knn_hypergraph(t(x), 1))         # k = 1: every hyperedge is its centre
    assert np.array_equal(one, np.eye(n))
