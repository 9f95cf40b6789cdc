"""fps, segmented knn, radius and the graph builders on the GPU against plain numpy loops in fp64, on integer coordinates in
[-512, 512] with d <= 8: every squared distance is below 2^24 and exact in fp32 in any order, so indices must be equal and
dist2 bit-equal.  One float-valued case goes against the fp32 chain of knn_ref.dist2_ref instead."""
import numpy as np
import pytest
import torch

import gcn_amd
from knn_ref import dist2_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = (0, 1, 2, 63, 64, 65, 1023, 1025)              # fps: one wave, its edges, the 256-thread route's top and beyond
KSIZES = (0, 1, 63, 64, 65, 130)                       # knn: query and candidate tiles of 64 straddle these


def _ptr(sizes):
    return [0] + np.cumsum(sizes).tolist()


def _points(n, d, seed, span=512):
    return np.random.default_rng(seed).integers(-span, span + 1, (n, d)).astype(np.float32)


def fps_ref(x, ptr, out_ptr, start=None, chain=False):
    """the contract as a loop: (idx, dist2) of every cloud's picks; chain=True takes the distances from dist2_ref"""
    idx, dist = [], []
    for b in range(len(ptr) - 1):
        pts = x[ptr[b]:ptr[b + 1]].astype(np.float64)
        table = dist2_ref(pts, pts).astype(np.float64) if chain else None
        dmin, alive = np.full(len(pts), np.inf), np.ones(len(pts), bool)
        w, wd = (0 if start is None else start[b] - ptr[b]), np.inf
        for _ in range(out_ptr[b + 1] - out_ptr[b]):
            idx.append(ptr[b] + w)
            dist.append(wd)
            alive[w] = False
            with np.errstate(invalid="ignore"):
                d2 = table[:, w] if chain else ((pts - pts[w]) ** 2).sum(axis=1)
            dmin = np.minimum(dmin, np.where(np.isnan(d2), 0.0, d2))
            cand = np.where(alive, dmin, -1.0)
            w = int(np.argmax(cand))                   # (the first of equal values: the smaller index)
            wd = cand[w]
    return np.array(idx, np.int32), np.array(dist, np.float32)


def _check_fps(x, ptr, start=None, chain=False, view=None, **how):
    xt = torch.from_numpy(x).to(DEV) if view is None else view
    st = start if start is None or view is None else torch.tensor(start, dtype=torch.int32, device=DEV)    # (both forms)
    idx, out_ptr, d2 = gcn_amd.fps(xt, ptr, start=st, return_dist2=True, **how)
    ridx, rd2 = fps_ref(x, ptr, out_ptr, start, chain)
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    assert np.array_equal(idx, ridx) and np.array_equal(d2.view(np.uint32), rd2.view(np.uint32))
    return idx, d2, out_ptr


@pytest.mark.parametrize("ratio", [0.25, 1.0])
@pytest.mark.parametrize("d", [1, 3, 4, 5, 8])
def test_fps_of_a_batch_of_every_segment_size(d, ratio):
    ptr = _ptr(SIZES)
    idx, d2, out_ptr = _check_fps(_points(ptr[-1], d, 10 + d), ptr, ratio=ratio)
    assert np.diff(out_ptr).tolist() == [int(np.ceil(ratio * s)) for s in SIZES]
    for b in range(len(SIZES)):
        seg, dd = idx[out_ptr[b]:out_ptr[b + 1]], d2[out_ptr[b]:out_ptr[b + 1]]
        assert len(set(seg.tolist())) == len(seg) and np.all(dd[2:] <= dd[1:-1])
        if ratio == 1.0:
            assert np.array_equal(np.sort(seg), np.arange(ptr[b], ptr[b + 1]))


@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("d", [1, 3, 4, 5, 8])
def test_fps_at_the_route_boundary_the_library_reports(d, extra):
    n = gcn_amd.load_library().gcn_fps_resident_points(d) + extra
    _check_fps(_points(n, d, 20 + d), [0, n], ratio=0.25)


def test_fps_routes_agree_on_the_same_points():
    """row L repeats the start row, so it sits at distance 0 from the first pick on and is chosen after every other row: the
    first picks of the cloud [0, L] (streamed: L + 1 rows) are those of the cloud [0, L) (resident), split off at L"""
    L = gcn_amd.load_library().gcn_fps_resident_points(3)
    x = _points(L + 1, 3, 30)
    x[L] = x[0]
    xt = torch.from_numpy(x).to(DEV)
    whole, _, dw = gcn_amd.fps(xt, [0, L + 1], count=300, return_dist2=True)
    split, out_ptr, ds = gcn_amd.fps(xt, [0, L, L + 1], count=300, return_dist2=True)
    assert out_ptr == [0, 300, 301] and torch.equal(whole, split[:300]) and torch.equal(dw.view(torch.int32), ds[:300].view(torch.int32))


def test_fps_on_a_lattice_with_repeats_from_explicit_starts_through_a_row_stride():
    g = np.stack(np.meshgrid(*[np.arange(4.0)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    x = np.concatenate([g, g, g[:37]])                   # 165 rows: only the index decides among equals
    wide = torch.full((len(x), 6), 7.0, device=DEV)
    wide[:, 1:4] = torch.from_numpy(x).to(DEV)
    _check_fps(x, [0, 64, 165], start=[63, 100], view=wide[:, 1:4], ratio=1.0)
    _check_fps(x, [0, 64, 165], start=[0, 164], count=50)


def test_fps_picks_a_row_with_a_nan_last_unless_it_starts():
    x = _points(200, 3, 40)
    x[77, 1] = np.nan
    idx, _, out_ptr = _check_fps(x, [0, 65, 200], ratio=1.0)
    assert idx[out_ptr[2] - 1] == 77
    idx, _, _ = _check_fps(x, [0, 65, 200], start=[0, 77], ratio=1.0)
    assert idx[65] == 77


def test_fps_on_float_points_follows_the_fp32_chain():
    x = np.random.default_rng(50).standard_normal((300, 3)).astype(np.float32)
    _check_fps(x, [0, 100, 300], chain=True, ratio=0.5)


def seg_ref(x, y, px, py, k, r2=np.inf, exclude_self=False):
    """per segment: dist2_ref, the admissible candidates, a sort by (distance bits, index)"""
    idx, out = np.full((len(x), k), -1, np.int32), np.full((len(x), k), np.inf, np.float32)
    for s in range(len(px) - 1):
        d2 = dist2_ref(x[px[s]:px[s + 1]], y[py[s]:py[s + 1]])
        js = np.arange(py[s], py[s + 1])
        for i in range(d2.shape[0]):
            ok = (d2[i] <= r2) & ~(exclude_self & (js == px[s] + i))
            order = np.lexsort((js[ok], d2[i][ok].view(np.uint32)))[:k]
            idx[px[s] + i, :len(order)], out[px[s] + i, :len(order)] = js[ok][order], d2[i][ok][order]
    return idx, out


def _same(got, want):
    idx, d2 = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert np.array_equal(idx, want[0]) and np.array_equal(d2.view(np.uint32), want[1].view(np.uint32))
    return idx, d2


@pytest.mark.parametrize("exclude_self", [False, True])
@pytest.mark.parametrize("k", [1, 16, 64])
def test_knn_within_segments(k, exclude_self):
    ptr = _ptr(KSIZES)
    x = _points(ptr[-1], 3, 60, span=4)                  # a small span: ties and duplicates everywhere
    got = gcn_amd.knn(torch.from_numpy(x).to(DEV), k, exclude_self=exclude_self, ptr_x=ptr)
    _same(got, seg_ref(x, x, ptr, ptr, k, exclude_self=exclude_self))


def test_knn_between_two_differently_cut_sets():
    px, py = _ptr((3, 0, 70, 1, 64, 5)), _ptr(KSIZES)
    x, y = _points(px[-1], 5, 61, span=6), _points(py[-1], 5, 62, span=6)
    xt, yt = torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)
    want = seg_ref(x, y, px, py, 16)
    _same(gcn_amd.knn(xt, 16, y=yt, ptr_x=px, ptr_y=py), want)
    dev_ptrs = [torch.tensor(p, dtype=torch.int32, device=DEV) for p in (px, py)]
    _same(gcn_amd.knn(xt, 16, y=yt, ptr_x=dev_ptrs[0], ptr_y=dev_ptrs[1]), want)


@pytest.mark.parametrize("r, k", [(2.0, 16), (0.0, 16), (3.0, 1), (100.0, 64)])
def test_radius_is_inclusive_and_keeps_the_nearest(r, k):
    ptr = _ptr(KSIZES)
    x = _points(ptr[-1], 3, 63, span=3)
    idx, d2 = _same(gcn_amd.radius(torch.from_numpy(x).to(DEV), r, k, ptr_x=ptr), seg_ref(x, x, ptr, ptr, k, r2=np.float32(r) ** 2))
    assert np.all(d2[idx >= 0] <= r * r) and np.all(np.isinf(d2[idx < 0]))
    if r == 2.0:
        assert np.any(d2 == 4.0)                         # lattice points at distance exactly r are kept
    if r == 0.0:
        assert np.any(idx[:, 1] >= 0) and np.all(d2[idx >= 0] == 0)      # duplicates, and nothing else


def test_one_segment_without_a_radius_is_knn_bit_for_bit():
    x = torch.from_numpy(_points(323, 8, 64, span=5)).to(DEV)
    for k in (1, 16, 64):
        plain, seg = gcn_amd.knn(x, k, exclude_self=True), gcn_amd.knn(x, k, exclude_self=True, ptr_x=[0, 323])
        assert torch.equal(plain[0], seg[0]) and torch.equal(plain[1].view(torch.int32), seg[1].view(torch.int32))


@pytest.mark.parametrize("loop", [False, True])
def test_graph_builders_against_a_dense_adjacency(loop):
    ptr = _ptr((5, 0, 64, 30))
    x = _points(ptr[-1], 3, 65, span=3)
    xt = torch.from_numpy(x).to(DEV)
    for adj, (ridx, _) in ((gcn_amd.radius_graph(xt, 2.0, 8, ptr=ptr, loop=loop), seg_ref(x, x, ptr, ptr, 8, 4.0, not loop)),
                           (gcn_amd.knn_graph(xt, 8, loop=loop, ptr=ptr), seg_ref(x, x, ptr, ptr, 8, exclude_self=not loop))):
        dense = np.zeros((len(x), len(x)), bool)
        rows = np.repeat(np.arange(len(x)), 8)[ridx.reshape(-1) >= 0]
        dense[rows, ridx.reshape(-1)[ridx.reshape(-1) >= 0]] = True
        rowptr, col = adj.rowptr.cpu().numpy(), adj.col.cpu().numpy()
        assert np.array_equal(rowptr, np.concatenate([[0], np.cumsum(dense.sum(axis=1))]))
        assert np.array_equal(col, np.nonzero(dense)[1])         # (row-major nonzero: ascending columns within a row)
        assert np.all(np.searchsorted(ptr, col, "right") == np.searchsorted(ptr, np.repeat(np.arange(len(x)), np.diff(rowptr)), "right"))
        assert dense.diagonal().any() == loop and bool((adj.val == 1).all())


def test_fps_chains_into_a_ball_query_of_the_picks():
    ptr = _ptr((100, 300, 65))
    x = torch.from_numpy(_points(ptr[-1], 3, 66, span=20)).to(DEV)
    idx, out_ptr = gcn_amd.fps(x, ptr, ratio=0.25)
    nbr, d2 = gcn_amd.radius(x[idx.long()], 8.0, 16, y=x, ptr_x=out_ptr, ptr_y=ptr)
    nbr, cloud = nbr.cpu().numpy(), np.repeat(np.arange(3), np.diff(out_ptr))
    assert bool((d2[:, 0] == 0).all())                   # a pick finds itself (or a duplicate) first
    assert np.all((np.searchsorted(ptr, nbr, "right") - 1 == cloud[:, None]) | (nbr < 0))
