"""Link prediction on the device (gcn_amd/csrc/lookup.hip and gcn_amd/linkpred.py).  The lookup and the negatives are pure
integer functions of their arguments, so every comparison is integer equality with the numpy twin of tests/linkpred_ref.py:
rows of every length around the probe counts of the search (0 .. 5000, a full row, a row lacking one column), repeated
columns, queries off both ends of a row and of the matrix, both launch shapes, misaligned operands, a captured graph; the
split, the edge subgraph and every batch of the loader against the twin; pair scores against fp64 autograd on the exact
grid the sddmm_heads tests use; and a short training run."""
import numpy as np
import pytest
import torch

import gcn_amd
from gcn_amd import _lib, graphgen
from linkpred_ref import (TEST, TRAIN, VAL, edge_subgraph_ref, find_entries_ref, link_batch_ref, lookup_fixture, lookup_queries,
                          negative_sample_ref, split_parts_ref)
from util import guards_intact, offset_view

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SMALL = 1 << 16                                        # lookup.hip's kLookupSmall: more queries get 256-thread workgroups

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _fixture(shape=(6000, 6000)):
    def make():
        rp, ci, full_row, almost_row, missing = lookup_fixture(*shape)
        adj = gcn_amd.CsrAdjacency(_t(rp), _t(ci), torch.ones(len(ci), device=DEV), shape)
        q_rows, q_cols = lookup_queries(rp, ci, shape[1])
        return dict(rp=rp, ci=ci, adj=adj, full=full_row, almost=almost_row, missing=missing, q_rows=q_rows, q_cols=q_cols,
                    want=find_entries_ref(rp, ci, q_rows, q_cols))
    return _cached(("fixture",) + shape, make)


def _same(got, want, what=""):
    assert got.dtype == torch.int32 and got.is_cuda, what
    g = got.cpu().numpy()
    assert g.shape == want.shape, (what, g.shape, want.shape)
    if not np.array_equal(g, want):
        at = np.argwhere(g != want)[0]
        raise AssertionError(f"{what}: differs at {tuple(at)}: got {g[tuple(at)]}, want {want[tuple(at)]}")


# ---- the lookup -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(6000, 6000), (40, 300)])
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_find_edges_equals_the_twin(shape, dtype):
    f = _fixture(shape)
    got = gcn_amd.find_edges(f["adj"], _t(f["q_rows"]).to(dtype), _t(f["q_cols"]).to(dtype))
    _same(got, f["want"], f"{shape} {dtype}")
    nnz = len(f["ci"])
    assert (f["want"][:nnz] < np.arange(nnz)).sum() > 10                       # (repeats: the lowest index, not the entry's own)
    assert gcn_amd.find_edges(f["adj"], _t(f["q_rows"][:0]), _t(f["q_cols"][:0])).shape == (0,)
    if dtype == torch.int64:                                                   # ids beyond int32 are not rows or columns
        far = torch.tensor([2 ** 32, 0, -2 ** 40], device=DEV)
        assert gcn_amd.find_edges(f["adj"], far, torch.zeros_like(far)).tolist()[::2] == [-1, -1]
        in_full = gcn_amd.find_edges(f["adj"], torch.full_like(far, f["full"]), far + 1).tolist()
        assert in_full == [-1, int(f["rp"][f["full"]]) + 1, -1]


def test_find_edges_with_more_queries_than_the_small_launch_takes():
    f = _fixture()
    reps = SMALL // len(f["q_rows"]) + 2
    assert len(f["q_rows"]) <= SMALL < reps * len(f["q_rows"])
    got = gcn_amd.find_edges(f["adj"], _t(np.tile(f["q_rows"], reps)), _t(np.tile(f["q_cols"], reps)))
    _same(got, np.tile(f["want"], reps))


# ---- the negatives ----------------------------------------------------------------------------------------------------------------
def _neg_queries(f):
    """every fixture row a few times (consecutive slots of one row, and the same row in different waves), empty rows, and
    rows -1 and m"""
    m = f["adj"].m
    special = np.arange(f["almost"] + 1)
    extra = np.random.default_rng(12).integers(0, m, 150)
    return np.concatenate([special, [-1, m], extra, special[::-1], [m + 7, -5]]).astype(np.int64)


@pytest.mark.parametrize("seed", [0, 1, 2 ** 63 + 5])
@pytest.mark.parametrize("offset", [0, 2 ** 32 + 1])
@pytest.mark.parametrize("num_neg, max_tries", [(1, 1), (1, 4), (1, 5), (1, 32), (1, 64), (3, 1), (3, 4), (3, 5), (3, 32), (3, 64)])
def test_negative_sample_equals_the_twin(seed, offset, num_neg, max_tries):
    for shape in ((6000, 6000), (40, 300)):
        f = _fixture(shape)
        rows = _neg_queries(f)
        lens = np.diff(f["rp"])
        for exclude_self in (True, False):
            want = negative_sample_ref(f["rp"], f["ci"], shape[1], rows, num_neg, seed, offset, max_tries, exclude_self)
            for dtype in (torch.int32, torch.int64):
                got = gcn_amd.negative_sample(f["adj"], _t(rows).to(dtype), num_neg, seed, offset, max_tries, exclude_self)
                _same(got, want, f"{shape} exclude_self={exclude_self} {dtype}")
            usable = (rows >= 0) & (rows < shape[0])
            assert (want[~usable] == -1).all() and (want[rows == f["full"]] == -1).all()
            almost = want[rows == f["almost"]]
            assert set(almost.ravel().tolist()) <= {-1, f["missing"]}
            for r, out in zip(rows[usable], want[usable]):                     # no drawn column is stored in its row
                kept = out[out >= 0]
                assert not np.isin(kept, f["ci"][f["rp"][r]:f["rp"][r + 1]]).any() and (kept < shape[1]).all()
                assert not (exclude_self and (kept == r).any())
                if lens[r] == 0 and max_tries >= 4 and shape[1] == 6000:
                    assert (out >= 0).all()                                    # an empty row refuses only itself


def test_negative_sample_with_more_slots_than_the_small_launch_takes():
    f = _fixture()
    rows = np.random.default_rng(13).integers(0, f["almost"] + 40, SMALL // 2 + 100)
    want = negative_sample_ref(f["rp"], f["ci"], 6000, rows, 2, 3, 4, 4, True)
    assert want.size > SMALL
    _same(gcn_amd.negative_sample(f["adj"], _t(rows), 2, seed=3, offset=4, max_tries=4), want)


def test_a_slot_does_not_depend_on_the_other_queries():
    """the slots of a query are the same bits alone and among 10 000 others, as long as the flat position is the same"""
    f = _fixture()
    rng = np.random.default_rng(14)
    rows = rng.integers(0, f["almost"] + 40, 10001)
    at, r = 7777, 15                                       # the row of 1023 entries
    rows[at] = r
    many = gcn_amd.negative_sample(f["adj"], _t(rows), 3, seed=9, offset=2)
    again = gcn_amd.negative_sample(f["adj"], _t(rows), 3, seed=9, offset=2)
    assert torch.equal(many, again)
    others = rng.integers(0, 40, 10001)
    others[at] = r
    alone = gcn_amd.negative_sample(f["adj"], _t(others[:at + 1]), 3, seed=9, offset=2)
    assert torch.equal(alone[at], many[at]) and not torch.equal(alone[:at], many[:at])
    for kw in (dict(seed=10, offset=2), dict(seed=9, offset=3)):
        assert not torch.equal(gcn_amd.negative_sample(f["adj"], _t(rows), 3, **kw), many)


@pytest.mark.parametrize("off", [1, 3])
def test_misaligned_operands(off):
    """rowptr, col, the queries and the outputs 4 * off bytes past a 16-byte boundary, inside sentinel-filled buffers:
    through the C ABI, which is where a caller chooses the output addresses"""
    f = _fixture((40, 300))
    m, n, nnz = 40, 300, len(f["ci"])
    q_rows, q_cols = f["q_rows"].astype(np.int32), f["q_cols"].astype(np.int32)
    q = len(q_rows)
    ins = [offset_view(a, off, torch.int32, DEV) for a in (f["rp"], f["ci"], q_rows, q_cols)]
    out_eid, out_neg = offset_view(q, off, torch.int32, DEV), offset_view(2 * q, off, torch.int32, DEV)
    for view, _ in ins + [out_eid, out_neg]:
        assert view.data_ptr() % 16 == (4 * off) % 16
    ptr = lambda pair: pair[0].data_ptr()
    lib, stream = _lib.load(), torch.cuda.current_stream(DEV).cuda_stream
    assert lib.gcn_csr_find_entries(ptr(ins[0]), ptr(ins[1]), m, nnz, ptr(ins[2]), ptr(ins[3]), q, ptr(out_eid), stream) == 0
    assert lib.gcn_negative_sample_csr(ptr(ins[0]), ptr(ins[1]), m, n, nnz, ptr(ins[2]), q, 2, 8, 1, 6, 7, ptr(out_neg), stream) == 0
    torch.cuda.synchronize()
    _same(out_eid[0], f["want"], f"find, offset {off}")
    _same(out_neg[0].view(q, 2), negative_sample_ref(f["rp"], f["ci"], n, q_rows, 2, 6, 7, 8, True), f"negatives, offset {off}")
    for view, flat in ins + [out_eid, out_neg]:
        assert guards_intact(flat, view)
    for (view, _), src in zip(ins, (f["rp"], f["ci"], q_rows, q_cols)):          # inputs unchanged
        assert np.array_equal(view.cpu().numpy(), src)
    # the Python layer on a misaligned pattern and misaligned queries gives the same
    adj = gcn_amd.CsrAdjacency(ins[0][0], ins[1][0], torch.ones(nnz, device=DEV), (m, n))
    assert adj.col.data_ptr() == ins[1][0].data_ptr() and adj.rowptr.data_ptr() == ins[0][0].data_ptr()
    _same(gcn_amd.find_edges(adj, ins[2][0], ins[3][0]), f["want"], "python")


def test_the_two_calls_are_captured_and_replayed():
    """negative_sample then find_edges on one stream inside torch.cuda.graph, after one eager call (which makes the
    column-order check, the only synchronisation): two replays give the eager bits"""
    f = _fixture()
    adj = f["adj"]
    rows = _t(_neg_queries(f))
    rows3 = rows.repeat_interleave(3)
    q_rows, q_cols = _t(f["q_rows"]), _t(f["q_cols"])

    def step():
        neg = gcn_amd.negative_sample(adj, rows, 3, seed=4, offset=9, max_tries=8)
        return neg, gcn_amd.find_edges(adj, rows3, neg.reshape(-1)), gcn_amd.find_edges(adj, q_rows, q_cols)
    eager = [t.clone() for t in step()]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for _ in range(2):
        for t in captured:
            t.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(captured, eager):
            assert torch.equal(got, want)
    _same(eager[2], f["want"])
    assert bool((eager[1] == -1).all()) and bool((eager[0] >= 0).any())          # no negative is a stored pair


# ---- edge_subgraph, split_edges, reverse_entries ---------------------------------------------------------------------------------
def _sbm():
    def make():
        rp, ci, va, n = graphgen.make_sbm(2000, block=500, deg_in=20, deg_out=4, device="cpu", seed=3, relabel=False)
        adj = gcn_amd.CsrAdjacency(rp.to(DEV), ci.to(DEV), va.to(DEV), (n, n), symmetric=True)
        return rp.numpy(), ci.numpy(), va.numpy(), adj
    return _cached("sbm", make)


def test_edge_subgraph_equals_the_twin():
    f = _fixture((40, 300))
    va = (np.arange(len(f["ci"])) % 89 + 1).astype(np.float32)
    adj = gcn_amd.CsrAdjacency(_t(f["rp"]), _t(f["ci"]), _t(va), (40, 300))
    for keep in (np.random.default_rng(15).random(len(va)) < 0.6, np.zeros(len(va), bool), np.ones(len(va), bool)):
        sub, eid = gcn_amd.edge_subgraph(adj, _t(keep))
        rp, ci, v, e = edge_subgraph_ref(f["rp"], f["ci"], va, keep)
        assert (sub.m, sub.n, sub.nnz) == (40, 300, int(keep.sum()))
        _same(sub.rowptr, rp), _same(sub.col, ci), _same(eid, e)
        assert np.array_equal(sub.val.cpu().numpy(), v)
    gcn_amd.find_edges(adj, adj.col[:1], adj.col[:1])                          # (the parent's order is known from here on)
    sub, eid = gcn_amd.edge_subgraph(adj, _t(np.arange(len(va)) % 3 != 0))
    _same(gcn_amd.find_edges(sub, _t(f["q_rows"]), _t(f["q_cols"])),
          find_entries_ref(sub.rowptr.cpu().numpy(), sub.col.cpu().numpy(), f["q_rows"], f["q_cols"]))


@pytest.mark.parametrize("undirected", [True, False])
def test_split_edges_equals_the_twin(undirected):
    rp, ci, va, adj = _sbm()
    nnz = len(ci)
    rows = np.repeat(np.arange(adj.m), np.diff(rp))
    rev = gcn_amd.reverse_entries(adj)
    rev_np = rev.cpu().numpy()
    assert (rev_np >= 0).all() and np.array_equal(rev_np[rev_np], np.arange(nnz))      # an involution ...
    assert np.array_equal(ci[rev_np], rows) and np.array_equal(rows[rev_np], ci)       # ... onto the mirrored pair
    train_adj, train_eid, val_eid, test_eid = gcn_amd.split_edges(adj, 0.1, 0.2, seed=11, undirected=undirected)
    part = split_parts_ref(rp, ci, 0.1, 0.2, 11, undirected)
    listed = rows < ci if undirected else np.ones(nnz, bool)
    _same(train_eid, np.nonzero(part == TRAIN)[0].astype(np.int32), "train")
    _same(val_eid, np.nonzero((part == VAL) & listed)[0].astype(np.int32), "val")
    _same(test_eid, np.nonzero((part == TEST) & listed)[0].astype(np.int32), "test")
    assert len(val_eid) > 100 and len(test_eid) > 200
    # the parts are disjoint and cover every entry (undirected: with the mirrors of the listed direction)
    held = torch.cat([val_eid, test_eid]).long()
    every = torch.cat([train_eid.long(), held] + ([rev[held].long()] if undirected else []))
    assert torch.equal(every.sort().values, torch.arange(nnz, device=DEV))
    if undirected:
        assert np.array_equal(part[rev_np], part) and (part[rows == ci] == TRAIN).all()
    else:
        assert (part[rev_np] != part).any()
    want_adj, want_eid = gcn_amd.edge_subgraph(adj, _t(part == TRAIN))
    assert torch.equal(want_eid, train_eid)
    for name in ("rowptr", "col", "val"):
        assert torch.equal(getattr(train_adj, name), getattr(want_adj, name)), name
    same = gcn_amd.split_edges(adj, 0.1, 0.2, seed=11, undirected=undirected)
    other = gcn_amd.split_edges(adj, 0.1, 0.2, seed=12, undirected=undirected)
    assert torch.equal(same[2], val_eid) and not torch.equal(other[2], val_eid)


def test_split_edges_needs_the_reverse_of_every_entry():
    f = _fixture((40, 300))
    square = gcn_amd.CsrAdjacency(_t(np.array([0, 1, 1, 2], np.int32)), _t(np.array([1, 0], np.int32)), torch.ones(2, device=DEV), (3, 3))
    with pytest.raises(ValueError, match="reverse"):
        gcn_amd.split_edges(square, 0.1, 0.1)
    assert gcn_amd.reverse_entries(square).tolist() == [-1, -1]
    with pytest.raises(ValueError, match="square"):
        gcn_amd.split_edges(f["adj"], 0.1, 0.1)
    parts = gcn_amd.split_edges(f["adj"], 0.3, 0.3, undirected=False)
    assert sum(int(p.numel()) for p in parts[1:]) == f["adj"].nnz
    unsorted = gcn_amd.CsrAdjacency(_t(np.array([0, 2], np.int32)), _t(np.array([1, 0], np.int32)), torch.ones(2, device=DEV), (1, 2))
    with pytest.raises(ValueError, match="coalesce_csr"):
        gcn_amd.find_edges(unsorted, _t(np.array([0])), _t(np.array([0])))


# ---- pair scores -------------------------------------------------------------------------------------------------------------------
def _ints(shape, seed, top, scale=1.0):
    return _t(np.random.default_rng(seed).integers(-top, top + 1, shape).astype(np.float32) * scale)


@pytest.mark.parametrize("heads, F", [(1, 8), (4, 8), (1, 5), (4, 5)])
def test_pair_scores_match_fp64_autograd_exactly(heads, F):
    """operands on the integer grids of the sddmm_heads cases of test_autograd_forms_gpu.py (entries in [-3, 3], the incoming
    gradient in eighths up to 7/8), where every sum is exact in fp32 in any order: the tolerance is that file's, equality"""
    m, n, q = 37, 53, 400
    rng = np.random.default_rng(20 + heads + F)
    rows, cols = rng.integers(0, m, q), rng.integers(0, n, q)
    rows[100:110], cols[100:110] = rows[5], cols[5]                             # repeated pairs
    a, b = _ints((m, heads * F), 21, 3).requires_grad_(True), _ints((n, heads * F), 22, 3).requires_grad_(True)
    g = _ints((q, heads), 23, 7, 0.125)
    for dtype in (torch.int64, torch.int32):
        r, c = _t(rows).to(dtype), _t(cols).to(dtype)
        out = gcn_amd.pair_scores(a, b, r, c, heads)
        ga, gb = torch.autograd.grad(out, (a, b), g)
        a64, b64 = a.detach().double().requires_grad_(True), b.detach().double().requires_grad_(True)
        ref = (a64[r.long()].view(q, heads, F) * b64[c.long()].view(q, heads, F)).sum(-1)
        ra, rb = torch.autograd.grad(ref, (a64, b64), g.double())
        for what, got, want in (("scores", out.detach(), ref.detach()), ("grad z_rows", ga, ra), ("grad z_cols", gb, rb)):
            assert torch.equal(want.float().double(), want), f"{what}: the fp64 result is not on the fp32 grid"
            assert got.shape == want.shape and torch.equal(got, want.float()), what
        again = gcn_amd.pair_scores(a, b, r, c, heads)
        assert torch.equal(again.detach().view(torch.int32), out.detach().view(torch.int32))
    # one table for both ends: the two gradients add
    z = _ints((n, heads * F), 24, 3).requires_grad_(True)
    u, v = _t(rng.integers(0, n, q)), _t(rng.integers(0, n, q))
    gz, = torch.autograd.grad(gcn_amd.pair_scores(z, z, u, v, heads), z, g)
    z64 = z.detach().double().requires_grad_(True)
    rz, = torch.autograd.grad((z64[u].view(q, heads, F) * z64[v].view(q, heads, F)).sum(-1), z64, g.double())
    assert torch.equal(gz, rz.float())
    # no pairs
    none = torch.zeros(0, dtype=torch.int64, device=DEV)
    empty = gcn_amd.pair_scores(a, b, none, none, heads)
    assert empty.shape == (0, heads) and empty.dtype == torch.float32
    for grad in torch.autograd.grad(empty.sum(), (a, b), allow_unused=True):
        assert grad is None or not bool(grad.any())
    with pytest.raises(ValueError):
        gcn_amd.pair_scores(a, b, _t(np.array([m])), _t(np.array([0])), heads)


# ---- the loader and a training run -------------------------------------------------------------------------------------------------
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


def test_link_neighbor_loader_equals_the_twin_batch_for_batch():
    rp, ci, va, adj = _sbm()
    assert len(ci) / adj.m <= adj.m / 2                                         # (mean degree: a negative is found at once)
    eids = np.sort(np.random.default_rng(16).permutation(len(ci))[:500])
    fanouts, num_neg, seed, batch = [3, 2], 2, 6, 128
    loader = gcn_amd.LinkNeighborLoader(adj, torch.from_numpy(eids), fanouts, batch, num_neg=num_neg, seed=seed, max_tries=32)
    assert len(loader) == 4
    gen = torch.Generator().manual_seed(seed)
    epochs = []
    for epoch in range(2):
        order = eids[torch.randperm(500, generator=gen).numpy()]
        seen = []
        for k, (blocks, input_ids, pair_rows, pair_cols, labels) in enumerate(loader):
            offset = (epoch * 4 + k) * (1 + len(fanouts))
            assert loader.last_offset == offset
            e = order[k * batch:(k + 1) * batch]
            assert np.array_equal(loader.last_eids.cpu().numpy(), e)
            ref_blocks, ref_ids, pr, pc, lab, nodes, neg = link_batch_ref(rp, ci, va, e, fanouts, num_neg, seed, offset, 32)
            assert (neg >= 0).all()                                            # the twin itself: no slot fails on this graph
            _assert_blocks_equal_ref(blocks, input_ids, ref_blocks, ref_ids)
            assert np.array_equal(blocks[-1].src_ids[:blocks[-1].num_dst].cpu().numpy(), nodes)
            assert pair_rows.dtype == pair_cols.dtype == torch.int64 and labels.dtype == torch.float32
            assert np.array_equal(pair_rows.cpu().numpy(), pr) and np.array_equal(pair_cols.cpu().numpy(), pc)
            assert np.array_equal(labels.cpu().numpy(), lab) and lab.sum() == len(e) and len(lab) == len(e) * (1 + num_neg)
            assert np.array_equal(nodes[pc[:len(e)]], ci[e])                   # the positives are the batch's entries
            seen.append(e)
        assert k == 3 and len(seen[-1]) == 500 - 3 * batch
        epochs.append(np.concatenate(seen))
    assert np.array_equal(np.sort(epochs[0]), eids) and np.array_equal(np.sort(epochs[1]), eids)
    assert not np.array_equal(epochs[0], epochs[1]) and loader.last_offset == 7 * 3
    plain = gcn_amd.LinkNeighborLoader(adj, torch.from_numpy(eids), [2], 200, shuffle=False)
    got = [plain.last_eids.cpu().numpy() for _ in plain]
    assert np.array_equal(np.concatenate(got), eids) and plain.last_offset == 4 and len(plain) == 3


def test_training_on_link_batches_lowers_the_loss():
    rp, ci, va, adj = _sbm()
    n = adj.m
    gen = torch.Generator().manual_seed(4)
    community = torch.arange(n) // 500
    x = (torch.randn((n, 16), generator=gen) + 1.5 * torch.nn.functional.one_hot(community, 16)).to(DEV)
    train_adj, train_eid, val_eid, test_eid = gcn_amd.split_edges(adj, 0.05, 0.1, seed=1)
    torch.manual_seed(1)
    model = gcn_amd.GraphSAGE(16, 32, 16, num_layers=2, aggr="mean", dropout=0.0).to(DEV).train()
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    loader = gcn_amd.LinkNeighborLoader(train_adj, torch.arange(train_adj.nnz), [5, 5], batch_size=512, num_neg=1, seed=2)
    assert train_eid.numel() == train_adj.nnz and len(loader) >= 20
    losses = []
    for blocks, input_ids, pair_rows, pair_cols, labels in loader:
        opt.zero_grad()
        z = model(x[input_ids], blocks)
        assert z.shape[0] == blocks[-1].num_dst
        loss = torch.nn.functional.binary_cross_entropy_with_logits(gcn_amd.pair_scores(z, z, pair_rows, pair_cols).squeeze(1), labels)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        if len(losses) == 20:
            break
    assert len(losses) == 20 and all(np.isfinite(losses))
    print("losses", [round(v, 4) for v in losses])
    assert np.mean(losses[-5:]) < np.mean(losses[:5]), losses
