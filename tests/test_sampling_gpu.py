"""Device neighbour sampling (gcn_amd/csrc/sample.hip), the blocks built from it and the layers that consume them.  The
sample is a pure function of (seed, offset, entry index), so every comparison here is integer equality with the numpy
reference of tests/sampling_ref.py: row lengths on both sides of every threshold of the kernel, a row that is the whole
matrix, keys that tie, misaligned operands, the relabelling of sample_blocks, and a GraphSAGE forward on blocks that must
equal the full-graph forward bit for bit."""
import numpy as np
import pytest
import torch

import gcn_amd
from gcn_amd import _lib, graphgen
from sampling_ref import TIE_SEARCH, sample_blocks_ref, sample_neighbors_ref, tie_row, tied_pairs
from util import assert_exact_inputs, guards_intact, int_features, offset_view, random_rows_csr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LONG = _lib.SAMPLE_LONG_ROW
F0 = 5                                                 # the fanout the lengths f - 1, f, f + 1 are built around
LENS = [0, 1, F0 - 1, F0, F0 + 1, 63, 64, 65, 255, 256, 257, LONG - 1, LONG, LONG + 1, 3 * LONG, 0, 2, 66, 1000]

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pattern_adj(rp, ci, shape):
    return gcn_amd.CsrAdjacency(_t(rp), _t(ci), torch.ones(len(ci), device=DEV), shape)


def _lengths_matrix():
    def make():
        m, n = len(LENS), 5000
        rp, ci = random_rows_csr(m, n, LENS, seed=11)
        return rp, ci, _pattern_adj(rp, ci, (m, n))
    return _cached("lengths", make)


def _assert_sample(got, want, what=""):
    for name, g, w in zip(("rowptr", "col", "eid"), got, want):
        assert g.dtype == torch.int32 and g.is_cuda, (what, name)
        g = g.cpu().numpy()
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            at = int(np.nonzero(g != w)[0][0])
            raise AssertionError(f"{what}: {name} differs at {at}: got {g[at]}, want {w[at]}")


@pytest.mark.parametrize("fanout", [1, 2, F0, 64, 65, -1])
def test_every_row_length(fanout):
    rp, ci, adj = _lengths_matrix()
    m = adj.m
    rng = np.random.default_rng(100 + fanout)
    seed, offset = 12345 + fanout, (3 << 32) + 17         # (the high word of the offset is part of the counter)
    for seeds, dtype in ((rng.permutation(m), torch.int32), (rng.permutation(m), torch.int64), (np.array([m - 5]), torch.int64),
                         (np.array([11]), torch.int32), (np.array([14, 0, 9, 14, 3, 13, 1]), torch.int32),
                         (rng.permutation(m)[:7], torch.int64)):
        got = gcn_amd.sample_neighbors(adj, _t(seeds).to(dtype), fanout, seed=seed, offset=offset)
        want = sample_neighbors_ref(rp, ci, seeds, fanout, seed, offset)
        _assert_sample(got, want, f"fanout {fanout}, {len(seeds)} {dtype} seeds")


def test_no_seeds_and_seeds_out_of_range():
    rp, ci, adj = _lengths_matrix()
    for dtype in (torch.int32, torch.int64):
        r, c, e = gcn_amd.sample_neighbors(adj, torch.zeros(0, dtype=dtype, device=DEV), 3)
        assert r.tolist() == [0] and c.numel() == 0 and e.numel() == 0
        for bad in ([0, adj.m], [-1, 2]):
            with pytest.raises(ValueError, match="seeds must lie"):
                gcn_amd.sample_neighbors(adj, torch.tensor(bad, dtype=dtype, device=DEV), 3)
    with pytest.raises(ValueError, match="seeds must lie"):                           # (not folded into int32 first)
        gcn_amd.sample_neighbors(adj, torch.tensor([1 << 32], dtype=torch.int64, device=DEV), 3)


def test_one_row_that_is_the_whole_matrix():
    nnz, f = 1 << 18, 1000
    rp = np.array([0, nnz], np.int32)
    ci = np.random.default_rng(3).integers(0, 1 << 20, nnz).astype(np.int32)
    adj = _pattern_adj(rp, ci, (1, 1 << 20))
    seeds = np.array([0])
    _assert_sample(gcn_amd.sample_neighbors(adj, _t(seeds), f, seed=9, offset=4), sample_neighbors_ref(rp, ci, seeds, f, 9, 4))
    _assert_sample(gcn_amd.sample_neighbors(adj, _t(seeds), -1), sample_neighbors_ref(rp, ci, seeds, -1))


def _tie_pairs():
    """the nearest tied pair (its row fits a wave) and the nearest one whose row needs the workgroup kernel"""
    pairs = tied_pairs(1, 0, TIE_SEARCH)
    assert pairs, "no equal keys below 2^22: the tie rule would go untested"
    near = [p for p in pairs if p[1] - p[0] + 7 <= LONG]
    far = [p for p in pairs if p[1] - p[0] > LONG]
    assert near, "no tied pair nearer than the long-row limit"
    assert far, "no tied pair farther than the long-row limit"
    return {"near": near[0], "far": far[0]}


@pytest.mark.parametrize("which", ["near", "far"])
def test_tied_keys_go_to_the_lower_entry(which):
    e1, e2, key = _tie_pairs()[which]
    b, e, f = tie_row(e1, e2, key)
    assert (e - b <= LONG) == (which == "near")
    assert 3 <= b and e <= TIE_SEARCH
    rp = np.array([0, b, e, TIE_SEARCH], np.int32)         # the row covers exactly [e1 - 3, e2 + 4)
    ci = _cached("tie_cols", lambda: np.random.default_rng(5).integers(0, 1 << 20, TIE_SEARCH).astype(np.int32))
    adj = _pattern_adj(rp, ci, (3, 1 << 20))
    seeds = np.array([1])
    want = sample_neighbors_ref(rp, ci, seeds, f, 1, 0)
    assert e1 in want[2] and e2 not in want[2] and len(want[2]) == f
    got = gcn_amd.sample_neighbors(adj, _t(seeds), f, seed=1, offset=0)
    _assert_sample(got, want, which)
    # one entry more takes the second of the pair too
    _assert_sample(gcn_amd.sample_neighbors(adj, _t(seeds), f + 1, seed=1, offset=0), sample_neighbors_ref(rp, ci, seeds, f + 1, 1, 0))


def test_deterministic_and_independent_of_the_batch():
    rp, ci, adj = _lengths_matrix()
    m = adj.m
    a = gcn_amd.sample_neighbors(adj, _t(np.arange(m)), 7, seed=2, offset=5)
    b = gcn_amd.sample_neighbors(adj, _t(np.arange(m)), 7, seed=2, offset=5)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    v = LENS.index(1000)                                   # a row with d >> f, inside two different seed sets
    one = gcn_amd.sample_neighbors(adj, _t(np.array([3, v, 14])), 7, seed=2, offset=5)
    two = gcn_amd.sample_neighbors(adj, _t(np.array([v, 8, 10, 12])), 7, seed=2, offset=5)
    ra, rb = one[0].tolist(), two[0].tolist()
    for k in (1, 2):
        assert torch.equal(one[k][ra[1]:ra[2]], two[k][rb[0]:rb[1]])
        assert torch.equal(one[k][ra[1]:ra[2]], a[k][a[0][v]:a[0][v + 1]])
    other = gcn_amd.sample_neighbors(adj, _t(np.array([v])), 7, seed=2, offset=6)
    assert not torch.equal(other[2], one[2][ra[1]:ra[2]])  # (7 of 1000: the same subset has probability ~1e-17)
    other = gcn_amd.sample_neighbors(adj, _t(np.array([v])), 7, seed=3, offset=5)
    assert not torch.equal(other[2], one[2][ra[1]:ra[2]])


@pytest.mark.parametrize("off", [1, 3])
def test_misaligned_operands(off):
    """every array of the call 4 * off bytes past a 16-byte boundary, inside sentinel-filled buffers: through the C ABI,
    which is where a caller chooses the output addresses (the Python layer allocates its own)"""
    rp, ci, _ = _lengths_matrix()
    m = len(LENS)
    seeds = np.random.default_rng(8).permutation(m).astype(np.int32)
    fanout, seed, offset = 6, 4, 2
    want = sample_neighbors_ref(rp, ci, seeds, fanout, seed, offset)
    total = len(want[1])
    ins = [offset_view(a, off, torch.int32, DEV) for a in (rp, ci, seeds, want[0])]
    outs = [offset_view(total, off, torch.int32, DEV) for _ in range(2)]
    ws = torch.empty(_lib.SAMPLE_WS_BYTES, dtype=torch.uint8, device=DEV)
    ptr = lambda t: t.data_ptr()
    for view, _ in ins + outs:
        assert view.data_ptr() % 16 == (4 * off) % 16
    st = _lib.load().gcn_sample_neighbors_csr(ptr(ins[0][0]), ptr(ins[1][0]), m, len(ci), ptr(ins[2][0]), m, fanout, seed, offset,
                                              ptr(ins[3][0]), ptr(outs[0][0]), ptr(outs[1][0]), ptr(ws), ws.numel(),
                                              torch.cuda.current_stream(DEV).cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    _assert_sample((ins[3][0], outs[0][0], outs[1][0]), want, f"offset {off}")
    for view, flat in ins + outs:
        assert guards_intact(flat, view)
    for (view, _), src in zip(ins, (rp, ci, seeds, want[0])):     # inputs unchanged
        assert np.array_equal(view.cpu().numpy(), src)
    # the Python layer on a misaligned col and misaligned seeds gives the same
    adj = gcn_amd.CsrAdjacency(_t(rp), ins[1][0], torch.ones(len(ci), device=DEV), (m, 5000))
    assert adj.col.data_ptr() == ins[1][0].data_ptr()
    _assert_sample(gcn_amd.sample_neighbors(adj, ins[2][0], fanout, seed=seed, offset=offset), want, "python")


# ---- blocks -------------------------------------------------------------------------------------------------------------------
def _graph300():
    def make():
        n = 300
        lens = np.random.default_rng(21).integers(0, 12, n)
        rp, ci = random_rows_csr(n, n, lens, seed=22)
        va = (np.arange(len(ci)) % 97 + 1).astype(np.float32)
        return rp, ci, va, gcn_amd.CsrAdjacency(_t(rp), _t(ci), _t(va), (n, n))
    return _cached("g300", make)


def _check_blocks(blocks, input_ids, seeds, parent, rp=None, ci=None):
    """the structure every batch must have; rp / ci: the parent's arrays on the host (then entries are checked too)"""
    frontier = torch.as_tensor(seeds).to(DEV).long()
    for blk in reversed(blocks):                           # from the seeds outwards
        assert blk.num_dst == frontier.numel() == blk.adj.m and blk.adj.n == blk.src_ids.numel()
        assert torch.equal(blk.src_ids[:blk.num_dst], frontier)
        assert blk.src_ids.unique().numel() == blk.src_ids.numel()
        tail = blk.src_ids[blk.num_dst:]
        assert bool((tail[1:] > tail[:-1]).all())
        assert blk.eid.dtype == torch.int32 and blk.adj.nnz == blk.eid.numel()
        eid = blk.eid.long()
        assert torch.equal(blk.adj.val, parent.val[eid])
        assert torch.equal(blk.src_ids[blk.adj.col.long()], parent.col[eid].long())
        rows = torch.repeat_interleave(frontier, (blk.adj.rowptr[1:] - blk.adj.rowptr[:-1]).long())
        assert bool((parent.rowptr[rows] <= blk.eid).all()) and bool((blk.eid < parent.rowptr[rows + 1]).all())
        frontier = blk.src_ids
    assert torch.equal(input_ids, blocks[0].src_ids)


def _assert_blocks_equal_ref(blocks, input_ids, ref_blocks, ref_ids):
    assert len(blocks) == len(ref_blocks)
    assert np.array_equal(input_ids.cpu().numpy(), ref_ids)
    for blk, ref in zip(blocks, ref_blocks):
        assert blk.num_dst == ref["num_dst"]
        assert np.array_equal(blk.src_ids.cpu().numpy(), ref["src_ids"])
        assert np.array_equal(blk.eid.cpu().numpy(), ref["eid"])
        assert np.array_equal(blk.adj.rowptr.cpu().numpy(), ref["rowptr"])
        assert np.array_equal(blk.adj.col.cpu().numpy(), ref["col"])
        assert np.array_equal(blk.adj.val.cpu().numpy(), ref["val"])


def test_sample_blocks_equal_the_reference_and_leave_the_map_clear():
    rp, ci, va, adj = _graph300()
    rng = np.random.default_rng(30)
    for seeds, dtype, offset in ((rng.permutation(300)[:40], torch.int64, 0), (rng.permutation(300)[:25], torch.int32, 7)):
        blocks, input_ids = gcn_amd.sample_blocks(adj, _t(seeds).to(dtype), [3, 2], seed=6, offset=offset)
        ref_blocks, ref_ids = sample_blocks_ref(rp, ci, va, seeds, [3, 2], 6, offset)
        _assert_blocks_equal_ref(blocks, input_ids, ref_blocks, ref_ids)
        _check_blocks(blocks, input_ids, seeds, adj)
        assert bool((adj._sample_map == -1).all())          # the second call starts from the cleared state
    with pytest.raises(ValueError, match="distinct"):
        gcn_amd.sample_blocks(adj, torch.tensor([4, 9, 4], device=DEV), [3, 2])
    assert bool((adj._sample_map == -1).all())


@pytest.mark.parametrize("aggr", ["sum", "max"])
def test_graphsage_on_blocks_equals_the_full_graph(aggr):
    """fanouts [-1, -1]: a block row holds every neighbour in the parent's order, so the two forwards do the same integer
    arithmetic — every intermediate is an integer below 2^24, exact in fp32 in any order"""
    rp, ci, va, adj = _graph300()
    n, k, hidden, out = 300, 6, 5, 4
    x = int_features(n, k, seed=40, top=2)
    torch.manual_seed(0)
    model = gcn_amd.GraphSAGE(k, hidden, out, num_layers=2, aggr=aggr, dropout=0.5).to(DEV).eval()
    rng = np.random.default_rng(41)
    with torch.no_grad():
        for p in model.parameters():                       # integer weights in [-1, 1]
            p.copy_(_t(rng.integers(-1, 2, tuple(p.shape)).astype(np.float32)))
    # the bound, layer by layer: |h1| <= (deg + 1) * k * 2 + 1, |out| <= (deg * |h1| + |h1|) * hidden + 1
    deg = int(np.diff(rp).max())
    ones = np.ones(len(ci), np.float32)
    assert_exact_inputs(rp, ci, ones, np.abs(x))
    h1 = (deg + 1) * k * 2 + 1
    assert (deg + 1) * h1 * hidden + 1 < 2 ** 24
    seeds = rng.permutation(n)[:50]
    xd = _t(x)
    with torch.no_grad():
        full = model(xd, adj)
        blocks, input_ids = gcn_amd.sample_blocks(adj, _t(seeds), [-1, -1])
        part = model(xd[input_ids], blocks)
    assert part.shape == (50, out)
    assert torch.equal(part.view(torch.int32), full[_t(seeds)].view(torch.int32))
    assert float(full.abs().max()) > 0 and float(full.abs().max()) < 2 ** 24
    assert torch.equal(full, full.round())


# ---- the loader and a training run ---------------------------------------------------------------------------------------------
def _planted():
    def make():
        rp, ci, va, n = graphgen.make_sbm(3072, block=512, deg_in=20, deg_out=4, device="cpu", seed=3, relabel=False)
        adj = gcn_amd.CsrAdjacency(rp.to(DEV), ci.to(DEV), va.to(DEV), (n, n))
        labels = (torch.arange(n) // 512).to(DEV)
        gen = torch.Generator().manual_seed(4)
        x = torch.randn((n, 16), generator=gen) + 1.5 * torch.nn.functional.one_hot(labels.cpu(), 16)
        return adj, x.to(DEV), labels
    return _cached("planted", make)


def test_neighbor_loader_covers_an_epoch_and_repeats_with_its_seed():
    adj, _, _ = _planted()
    idx = torch.arange(0, adj.m, 3)
    a = gcn_amd.NeighborLoader(adj, idx, [3, 2], batch_size=200, seed=5)
    b = gcn_amd.NeighborLoader(adj, idx, [3, 2], batch_size=200, seed=5)
    assert len(a) == (idx.numel() + 199) // 200
    seen, offsets, first_epoch = [], [], []
    for (blocks, input_ids, batch), (blocks_b, input_ids_b, batch_b) in zip(a, b):
        assert torch.equal(batch, batch_b) and torch.equal(input_ids, input_ids_b)
        for x, y in zip(blocks, blocks_b):
            assert torch.equal(x.eid, y.eid) and torch.equal(x.adj.col, y.adj.col) and torch.equal(x.src_ids, y.src_ids)
        seen.append(batch.cpu())
        offsets.extend(range(a.last_offset, a.last_offset + 2))
        first_epoch.append(batch.cpu())
    assert len(seen) == len(a) and seen[-1].numel() == idx.numel() % 200
    assert torch.equal(torch.cat(seen).sort().values, idx)  # every index exactly once
    assert len(set(offsets)) == len(offsets) == 2 * len(a)
    second = [batch.cpu() for _, _, batch in a]
    offsets.extend(range(a.last_offset, a.last_offset + 2))
    assert len(set(offsets)) == len(offsets)                # (the offset runs on into the next epoch)
    assert torch.equal(torch.cat(second).sort().values, idx) and not torch.equal(torch.cat(second), torch.cat(first_epoch))
    plain = gcn_amd.NeighborLoader(adj, idx, [2], batch_size=500, shuffle=False)
    assert torch.equal(torch.cat([batch.cpu() for _, _, batch in plain]), idx)


def test_training_on_sampled_batches_lowers_the_loss():
    adj, x, labels = _planted()
    torch.manual_seed(1)
    model = gcn_amd.GraphSAGE(16, 32, 6, num_layers=2, aggr="mean", dropout=0.1).to(DEV).train()
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    loader = gcn_amd.NeighborLoader(adj, torch.arange(adj.m), [5, 5], batch_size=256, seed=2)
    losses = []
    while len(losses) < 30:
        for blocks, input_ids, batch in loader:
            _check_blocks(blocks, input_ids, batch, adj)
            for blk in blocks:
                assert int((blk.adj.rowptr[1:] - blk.adj.rowptr[:-1]).max()) <= 5
            opt.zero_grad()
            loss = torch.nn.functional.cross_entropy(model(x[input_ids], blocks), labels[batch])
            loss.backward()
            opt.step()
            losses.append(float(loss))
            if len(losses) == 30:
                break
    assert all(np.isfinite(losses))
    assert np.mean(losses[-5:]) < np.mean(losses[:5]), losses
