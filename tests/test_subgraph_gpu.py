"""Induced subgraphs and random walks on the device (gcn_amd/csrc/subgraph.hip), the Python layer and the two loaders.
Both primitives are pure integer functions of their arguments, so every comparison is integer equality with the numpy twin
of tests/subgraph_ref.py: row lengths on both sides of every threshold of the kernel (a wave's 64 entries per pass, the four
passes kept in registers, the long-row limit), a row that is the whole matrix, misaligned operands inside guarded buffers,
the error paths and the state of the shared vertex map after them, and the walks at every Philox group boundary."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import gcn_amd
from gcn_amd import _lib, graphgen
from sampling_ref import sample_blocks_ref
from subgraph_ref import induced_subgraph_ref, random_walk_ref, walk_graph
from util import guards_intact, offset_view, random_rows_csr, rel_err, sym_norm_graph

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LONG = _lib.SAMPLE_LONG_ROW
LENS = [0, 1, 63, 64, 65, 255, 256, 257, LONG - 1, LONG, LONG + 1, 5000]
N = 6000

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _adj(rp, ci, n, va=None, symmetric=None):
    va = (np.arange(len(ci)) % 97 + 1).astype(np.float32) if va is None else va
    return va, gcn_amd.CsrAdjacency(_t(rp), _t(ci), _t(va), (n, n), symmetric=symmetric)


def _lengths_matrix():
    """6000 x 6000: rows 0 .. 11 have the lengths LENS, the others 0 .. 8 entries; columns repeat"""
    def make():
        lens = np.random.default_rng(10).integers(0, 9, N)
        lens[:len(LENS)] = LENS
        rp, ci = random_rows_csr(N, N, lens, seed=11)
        va, adj = _adj(rp, ci, N)
        return rp, ci, va, adj
    return _cached("lengths", make)


def _half(seed):
    """a random half of the vertices with the rows of LENS among them, ascending"""
    pick = np.random.default_rng(seed).permutation(N)[:N // 2]
    return np.union1d(pick, np.arange(len(LENS)))


def _assert_subgraph(sub, want, nodes, parent_val, what=""):
    assert isinstance(sub, gcn_amd.Subgraph) and sub.adj.m == sub.adj.n == len(nodes), what
    assert sub.node_ids.dtype == torch.int64 and np.array_equal(sub.node_ids.cpu().numpy(), nodes), what
    for name, g, w in zip(("rowptr", "col", "eid"), (sub.adj.rowptr, sub.adj.col, sub.eid), want):
        assert g.dtype == torch.int32 and g.is_cuda, (what, name)
        g = g.cpu().numpy()
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            at = int(np.nonzero(g != w)[0][0])
            raise AssertionError(f"{what}: {name} differs at {at}: got {g[at]}, want {w[at]}")
    assert np.array_equal(sub.adj.val.cpu().numpy(), parent_val[want[2]]), what


@pytest.mark.parametrize("order", ["ascending", "permuted"])
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_every_row_length(order, dtype):
    rp, ci, va, adj = _lengths_matrix()
    nodes = _half(1)
    if order == "permuted":
        nodes = np.random.default_rng(2).permutation(nodes)
    want = _cached(("want", order), lambda: induced_subgraph_ref(rp, ci, nodes, N))
    assert np.diff(want[0])[np.argsort(nodes)[:len(LENS)]].max() > LONG // 4          # (the long rows keep many entries)
    sub = gcn_amd.induced_subgraph(adj, _t(nodes).to(dtype))
    _assert_subgraph(sub, want, nodes, va, f"{order} {dtype}")
    assert bool((adj._sample_map == -1).all())
    again = gcn_amd.induced_subgraph(adj, _t(nodes).to(dtype))                        # the same bits at every call
    for x, y in ((sub.adj.rowptr, again.adj.rowptr), (sub.adj.col, again.adj.col), (sub.eid, again.eid), (sub.adj.val, again.adj.val)):
        assert torch.equal(x, y)
    ones = gcn_amd.induced_subgraph(adj, _t(nodes).to(dtype), values="pattern")
    assert torch.equal(ones.adj.col, sub.adj.col) and bool((ones.adj.val == 1).all())


def test_one_row_that_is_the_whole_matrix():
    n, nnz = 4096, 1 << 16
    lens = np.zeros(n, np.int64)
    lens[7] = nnz
    rp, ci = random_rows_csr(n, n, lens, seed=3)
    va, adj = _adj(rp, ci, n)
    nodes = np.union1d(np.random.default_rng(4).permutation(n)[:n // 2], [7])
    want = induced_subgraph_ref(rp, ci, nodes, n)
    assert len(want[1]) > nnz // 3
    _assert_subgraph(gcn_amd.induced_subgraph(adj, _t(nodes)), want, nodes, va)
    one = np.array([7])                                    # the row alone: only its own column survives
    _assert_subgraph(gcn_amd.induced_subgraph(adj, _t(one)), induced_subgraph_ref(rp, ci, one, n), one, va)


def _graph300():
    def make():
        n = 300
        lens = np.random.default_rng(21).integers(0, 12, n)
        rp, ci = random_rows_csr(n, n, lens, seed=22)
        va, adj = _adj(rp, ci, n)
        return rp, ci, va, adj
    return _cached("g300", make)


def test_all_vertices_none_and_a_vertex_without_a_self_loop():
    rp, ci, va, adj = _graph300()
    sub = gcn_amd.induced_subgraph(adj, torch.arange(300, device=DEV))
    assert torch.equal(sub.adj.rowptr, adj.rowptr) and torch.equal(sub.adj.col, adj.col) and torch.equal(sub.adj.val, adj.val)
    assert torch.equal(sub.eid, torch.arange(adj.nnz, dtype=torch.int32, device=DEV))
    for dtype in (torch.int32, torch.int64):
        none = gcn_amd.induced_subgraph(adj, torch.zeros(0, dtype=dtype, device=DEV), values="gcn")
        assert (none.adj.m, none.adj.n, none.adj.nnz) == (0, 0, 0) and none.adj.rowptr.tolist() == [0]
        assert none.eid.numel() == 0 and none.node_ids.numel() == 0 and none.eid.dtype == torch.int32
    v = next(v for v in range(300) if rp[v + 1] > rp[v] and v not in ci[rp[v]:rp[v + 1]])
    for values in ("parent", "gcn", "pattern"):
        lone = gcn_amd.induced_subgraph(adj, torch.tensor([v], device=DEV), values=values)
        assert (lone.adj.m, lone.adj.n, lone.adj.nnz) == (1, 1, 0) and lone.adj.rowptr.tolist() == [0, 0]
        assert lone.adj.val.numel() == 0 and lone.node_ids.tolist() == [v]


def test_bad_nodes_raise_and_leave_the_shared_map_clear():
    rp, ci, va, adj = _graph300()
    for dtype in (torch.int32, torch.int64):
        for bad in ([0, 300], [-1, 2]):
            with pytest.raises(ValueError, match="nodes must lie"):
                gcn_amd.induced_subgraph(adj, torch.tensor(bad, dtype=dtype, device=DEV))
        with pytest.raises(ValueError, match="distinct"):
            gcn_amd.induced_subgraph(adj, torch.tensor([4, 9, 4], dtype=dtype, device=DEV))
        assert bool((adj._sample_map == -1).all())
    with pytest.raises(ValueError, match="nodes must lie"):                           # (not folded into int32 first)
        gcn_amd.induced_subgraph(adj, torch.tensor([1 << 32], dtype=torch.int64, device=DEV))
    assert bool((adj._sample_map == -1).all())
    seeds = np.random.default_rng(30).permutation(300)[:40]
    blocks, input_ids = gcn_amd.sample_blocks(adj, _t(seeds), [3, 2], seed=6, offset=1)
    ref_blocks, ref_ids = sample_blocks_ref(rp, ci, va, seeds, [3, 2], 6, 1)
    assert np.array_equal(input_ids.cpu().numpy(), ref_ids)
    for blk, ref in zip(blocks, ref_blocks):
        assert np.array_equal(blk.adj.col.cpu().numpy(), ref["col"]) and np.array_equal(blk.eid.cpu().numpy(), ref["eid"])
        assert np.array_equal(blk.src_ids.cpu().numpy(), ref["src_ids"])
    nodes = np.sort(seeds)
    _assert_subgraph(gcn_amd.induced_subgraph(adj, _t(nodes)), induced_subgraph_ref(rp, ci, nodes, 300), nodes, va, "after blocks")
    assert bool((adj._sample_map == -1).all())


@pytest.mark.parametrize("off", [1, 3])
def test_misaligned_operands_of_the_subgraph_calls(off):
    """every array of the two calls 4 * off bytes past a 16-byte boundary, inside sentinel-filled buffers: through the C ABI,
    which is where a caller chooses the addresses"""
    rp, ci, _, _ = _lengths_matrix()
    nodes = np.random.default_rng(2).permutation(_half(1)).astype(np.int32)
    want = _cached(("want", "permuted"), lambda: induced_subgraph_ref(rp, ci, nodes, N))
    vmap = np.full(N, -1, np.int32)
    vmap[nodes] = np.arange(len(nodes), dtype=np.int32)
    ins = [offset_view(a, off, torch.int32, DEV) for a in (rp, ci, nodes, vmap, want[0])]
    out_len, out_col, out_eid = (offset_view(k, off, torch.int32, DEV) for k in (len(nodes), len(want[1]), len(want[1])))
    ws = torch.empty(_lib.SUBGRAPH_WS_BYTES, dtype=torch.uint8, device=DEV)
    ptr = lambda t: t.data_ptr()
    for view, _ in ins + [out_len, out_col, out_eid]:
        assert view.data_ptr() % 16 == (4 * off) % 16
    lib, stream = _lib.load(), torch.cuda.current_stream(DEV).cuda_stream
    st = lib.gcn_induced_subgraph_count_csr(ptr(ins[0][0]), ptr(ins[1][0]), N, len(ci), ptr(ins[2][0]), len(nodes), ptr(ins[3][0]),
                                            ptr(out_len[0]), ptr(ws), ws.numel(), stream)
    assert st == 0
    st = lib.gcn_induced_subgraph_fill_csr(ptr(ins[0][0]), ptr(ins[1][0]), N, len(ci), ptr(ins[2][0]), len(nodes), ptr(ins[3][0]),
                                           ptr(ins[4][0]), ptr(out_col[0]), ptr(out_eid[0]), ptr(ws), ws.numel(), stream)
    assert st == 0
    torch.cuda.synchronize()
    assert np.array_equal(out_len[0].cpu().numpy(), np.diff(want[0]))
    assert np.array_equal(out_col[0].cpu().numpy(), want[1]) and np.array_equal(out_eid[0].cpu().numpy(), want[2])
    for view, flat in ins + [out_len, out_col, out_eid]:
        assert guards_intact(flat, view)
    for (view, _), src in zip(ins, (rp, ci, nodes, vmap, want[0])):                   # inputs unchanged
        assert np.array_equal(view.cpu().numpy(), src)
    # a slot of another length is left alone: one entry less for the longest row (the fill writes nothing there)
    short = want[0].copy()
    i = int(np.argmax(np.diff(want[0])))
    short[i + 1:] -= 1
    rp_short = offset_view(short, off, torch.int32, DEV)
    col2, eid2 = (offset_view(len(want[1]), off, torch.int32, DEV) for _ in range(2))
    st = lib.gcn_induced_subgraph_fill_csr(ptr(ins[0][0]), ptr(ins[1][0]), N, len(ci), ptr(ins[2][0]), len(nodes), ptr(ins[3][0]),
                                           ptr(rp_short[0]), ptr(col2[0]), ptr(eid2[0]), ptr(ws), ws.numel(), stream)
    assert st == 0
    torch.cuda.synchronize()
    got, sentinel = eid2[0].cpu().numpy(), eid2[1][0].item()
    assert np.all(got[short[i]:short[i + 1]] == sentinel) and got[-1] == sentinel
    assert np.array_equal(got[:short[i]], want[2][:want[0][i]]) and np.array_equal(got[short[i + 1]:-1], want[2][want[0][i + 1]:])
    assert guards_intact(col2[1], col2[0]) and guards_intact(eid2[1], eid2[0])


def _sym_graph():
    def make():
        n = 2000
        rp, ci, va = sym_norm_graph(n, 12000, seed=6)
        return rp, ci, va, gcn_amd.CsrAdjacency(_t(rp), _t(ci), _t(va), (n, n), symmetric=True)
    return _cached("sym", make)


def test_gcn_values_are_the_scipy_normalisation_of_the_extracted_pattern():
    rp, ci, va, adj = _sym_graph()
    nodes = np.random.default_rng(7).permutation(2000)[:900]
    sub = gcn_amd.induced_subgraph(adj, _t(nodes), values="gcn")
    srp, sci = sub.adj.rowptr.cpu().numpy().copy(), sub.adj.col.cpu().numpy().copy()     # (arrays numpy owns: scipy indexes with them)
    assert np.array_equal(srp, induced_subgraph_ref(rp, ci, nodes, 2000)[0])
    S = sp.csr_matrix((np.ones(len(sci)), sci, srp), shape=(900, 900))
    d = np.asarray(S.sum(1)).ravel() ** -0.5                   # (every row holds its self-loop: no zero degree)
    M = (sp.diags(d) @ S @ sp.diags(d)).tocsr()
    rows = np.repeat(np.arange(900), np.diff(srp))
    want = np.asarray(M[rows, sci]).ravel()                    # (looked up by position: scipy may have sorted its rows)
    assert sub.adj.val.dtype == torch.float32 and want.min() > 0
    assert np.abs(sub.adj.val.cpu().numpy().astype(np.float64) / want - 1).max() <= 1e-6


def test_symmetric_is_inherited_and_the_backward_equals_the_dense_formulation():
    rp, ci, va, adj = _sym_graph()
    assert gcn_amd.induced_subgraph(_graph300()[3], torch.arange(5, device=DEV)).adj.symmetric is None
    nodes = np.sort(np.random.default_rng(8).permutation(2000)[:700])
    sub = gcn_amd.induced_subgraph(adj, _t(nodes), values="gcn")
    assert sub.adj.symmetric is True
    dense = torch.zeros((700, 700), dtype=torch.float64, device=DEV)
    rows = torch.repeat_interleave(torch.arange(700, device=DEV), (sub.adj.rowptr[1:] - sub.adj.rowptr[:-1]).long())
    dense[rows, sub.adj.col.long()] = sub.adj.val.double()
    assert torch.equal(dense, dense.t())                       # a principal submatrix in one vertex order
    gen = torch.Generator().manual_seed(9)
    x = torch.randn((700, 24), generator=gen).to(DEV).requires_grad_(True)
    w = torch.randn((700, 24), generator=gen).to(DEV)
    y = gcn_amd.spmm(sub.adj, x)
    (y * w).sum().backward()
    assert sub.adj._transpose is None                          # (no transpose was built)
    # fp32 sums of at most a few dozen products against fp64: the parity metric and tolerance of the SpMM tests
    assert rel_err(y.detach().cpu().numpy(), (dense @ x.detach().double()).cpu().numpy()) <= 1e-5
    assert rel_err(x.grad.cpu().numpy(), (dense.t() @ w.double()).cpu().numpy()) <= 1e-5


# ---- random walks --------------------------------------------------------------------------------------------------------------
def _walks():
    def make():
        rp, ci = walk_graph()
        return rp, ci, _adj(rp, ci, 300)[1]
    return _cached("walks", make)


@pytest.mark.parametrize("length", [0, 1, 3, 4, 5, 8])
def test_walks_equal_the_twin(length):
    rp, ci, adj = _walks()
    seed, offset = 12345 + length, (3 << 32) + 17             # (the high word of the offset is part of the counter)
    for n_walks, dtype in ((0, torch.int64), (1, torch.int32), (63, torch.int64), (64, torch.int32), (65, torch.int64), (1000, torch.int32)):
        starts = np.random.default_rng(n_walks).integers(0, 300, n_walks)
        got = gcn_amd.random_walk(adj, _t(starts).to(dtype), length, seed=seed, offset=offset)
        assert got.dtype == torch.int32 and got.shape == (n_walks, length + 1)
        assert got.t().is_contiguous()                         # the step-major buffer, transposed
        want = random_walk_ref(rp, ci, starts, length, seed, offset)
        assert np.array_equal(got.cpu().numpy(), want), (n_walks, length)
    assert length < 4 or (np.diff(want[:, -3:], axis=1) == 0).all(1).any()            # some walk sits at a dead end


def test_walk_errors_prefix_independence_and_determinism():
    rp, ci, adj = _walks()
    for bad in ([0, 300], [-1, 2], [1 << 32]):
        with pytest.raises(ValueError, match="starts must lie"):
            gcn_amd.random_walk(adj, torch.tensor(bad, dtype=torch.int64, device=DEV), 3)
    starts = _t(np.random.default_rng(1).integers(0, 300, 500))
    full = gcn_amd.random_walk(adj, starts, 6, seed=2, offset=5)
    assert torch.equal(full, gcn_amd.random_walk(adj, starts, 6, seed=2, offset=5))
    for k in (1, 64, 130):
        assert torch.equal(gcn_amd.random_walk(adj, starts[:k], 6, seed=2, offset=5), full[:k])
    assert not torch.equal(gcn_amd.random_walk(adj, starts, 6, seed=2, offset=6), full)
    assert not torch.equal(gcn_amd.random_walk(adj, starts, 6, seed=3, offset=5), full)
    moved = (full[:, 1:] != full[:, :-1]).any(1)
    assert bool(moved.any()) and not bool(moved.all())         # (walks from isolated vertices never move)


@pytest.mark.parametrize("off", [1, 3])
def test_misaligned_operands_of_the_walk(off):
    rp, ci, _ = _walks()
    n_walks, length, seed, offset = 200, 5, 4, 2
    starts = np.random.default_rng(8).integers(0, 300, n_walks).astype(np.int32)
    starts[[3, 77]] = [300, -1]                                # through the C ABI a start out of range fills its walk with -1
    want = random_walk_ref(rp, ci, starts, length, seed, offset)
    assert np.all(want[[3, 77]] == -1)
    ins = [offset_view(a, off, torch.int32, DEV) for a in (rp, ci, starts)]
    out = offset_view((length + 1, n_walks), off, torch.int32, DEV)
    st = _lib.load().gcn_random_walk_csr(ins[0][0].data_ptr(), ins[1][0].data_ptr(), 300, len(ci), ins[2][0].data_ptr(), n_walks,
                                         length, seed, offset, out[0].data_ptr(), torch.cuda.current_stream(DEV).cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy().T, want)
    for view, flat in ins + [out]:
        assert guards_intact(flat, view)


# ---- the loaders and a training run ------------------------------------------------------------------------------------------------
def _planted():
    def make():
        rp, ci, va, n = graphgen.make_sbm(3072, block=512, deg_in=20, deg_out=4, device="cpu", seed=3, relabel=False)
        adj = gcn_amd.CsrAdjacency(rp.to(DEV), ci.to(DEV), va.to(DEV), (n, n), symmetric=True)
        labels = (torch.arange(n) // 512).to(DEV)
        gen = torch.Generator().manual_seed(4)
        x = torch.randn((n, 16), generator=gen) + 1.5 * torch.nn.functional.one_hot(labels.cpu(), 16)
        return adj, x.to(DEV), labels
    return _cached("planted", make)


def _check_subgraph(sub, parent):
    """the structure every batch must have"""
    k = sub.node_ids.numel()
    assert sub.adj.m == sub.adj.n == k and sub.adj.symmetric == parent.symmetric
    eid = sub.eid.long()
    assert torch.equal(sub.node_ids[sub.adj.col.long()], parent.col[eid].long())
    rows = torch.repeat_interleave(sub.node_ids, (sub.adj.rowptr[1:] - sub.adj.rowptr[:-1]).long())
    assert bool((parent.rowptr[rows] <= sub.eid).all()) and bool((sub.eid < parent.rowptr[rows + 1]).all())


def test_cluster_loader_covers_an_epoch_and_repeats_with_its_seed():
    adj, _, _ = _planted()
    parts = (torch.arange(adj.m) * 7919 % adj.m) // 128        # 24 clusters of 128 vertices, interleaved
    a = gcn_amd.ClusterLoader(adj, parts, 5, seed=5, values="parent")
    b = gcn_amd.ClusterLoader(adj, parts.to(DEV), 5, seed=5, values="parent")
    assert len(a) == 5 and a.num_clusters == 24
    first = []
    for sub, sub_b in zip(a, b):
        assert torch.equal(sub.node_ids, sub_b.node_ids) and torch.equal(sub.eid, sub_b.eid) and torch.equal(sub.adj.col, sub_b.adj.col)
        assert bool((sub.node_ids[1:] > sub.node_ids[:-1]).all())
        assert parts[sub.node_ids.cpu()].unique().numel() == sub.node_ids.numel() // 128
        assert torch.equal(sub.adj.val, adj.val[sub.eid.long()])
        _check_subgraph(sub, adj)
        first.append(sub.node_ids.cpu())
    assert [t.numel() for t in first] == [640, 640, 640, 640, 512]
    assert torch.equal(torch.cat(first).sort().values, torch.arange(adj.m))           # every vertex exactly once
    second = [sub.node_ids.cpu() for sub in a]
    assert torch.equal(torch.cat(second).sort().values, torch.arange(adj.m)) and not torch.equal(torch.cat(second), torch.cat(first))
    plain = [sub.node_ids.cpu() for sub in gcn_amd.ClusterLoader(adj, parts, 24, shuffle=False)]
    assert len(plain) == 1 and torch.equal(plain[0], torch.arange(adj.m))
    assert bool((adj._sample_map == -1).all())


def test_random_walk_loader_repeats_with_its_seed_and_advances_its_offset():
    adj, _, _ = _planted()
    idx = torch.arange(0, adj.m, 3)
    a = gcn_amd.RandomWalkLoader(adj, idx, 50, 3, 4, seed=5)
    b = gcn_amd.RandomWalkLoader(adj, idx, 50, 3, 4, seed=5)
    assert len(a) == 4
    offsets, batches = [], []
    for sub, sub_b in zip(a, b):
        assert torch.equal(sub.node_ids, sub_b.node_ids) and torch.equal(sub.eid, sub_b.eid) and torch.equal(sub.adj.val, sub_b.adj.val)
        assert bool((sub.node_ids[1:] > sub.node_ids[:-1]).all()) and 1 <= sub.node_ids.numel() <= 200
        _check_subgraph(sub, adj)
        offsets.append(a.last_offset)
        batches.append(sub.node_ids.cpu())
    assert offsets == [0, 1, 2, 3] and b.last_offset == 3
    more = [sub.node_ids.cpu() for sub in a]
    assert a.last_offset == 7 and len(more) == 4              # (the offset runs on into the next epoch)
    assert not all(torch.equal(x, y) for x, y in zip(batches, more))
    # the batch is what its parts give: the roots of the generator, the walks at the batch's offset, the induced subgraph
    gen = torch.Generator().manual_seed(5)
    roots = idx[torch.randint(idx.numel(), (50,), generator=gen)].to(DEV)
    walks = gcn_amd.random_walk(adj, roots, 3, seed=5, offset=0)
    assert torch.equal(torch.unique(walks), batches[0].to(DEV))


def test_training_a_gcn_on_cluster_batches_lowers_the_full_graph_loss():
    adj, x, labels = _planted()
    torch.manual_seed(1)
    l1, l2 = gcn_amd.GraphConvolution(16, 32).to(DEV), gcn_amd.GraphConvolution(32, 6).to(DEV)

    def model(feat, a):
        return l2(torch.relu(l1(feat, a)), a)

    def full_loss():
        with torch.no_grad():
            return float(torch.nn.functional.cross_entropy(model(x, adj), labels))

    opt = torch.optim.Adam(list(l1.parameters()) + list(l2.parameters()), lr=0.01)
    parts = (torch.arange(adj.m) * 7919 % adj.m) // 128
    loader = gcn_amd.ClusterLoader(adj, parts, 4, seed=2, values="gcn")
    before, steps = full_loss(), 0
    while steps < 30:
        for sub in loader:
            opt.zero_grad()
            loss = torch.nn.functional.cross_entropy(model(x[sub.node_ids], sub.adj), labels[sub.node_ids])
            loss.backward()
            opt.step()
            assert np.isfinite(float(loss))
            steps += 1
            if steps == 30:
                break
    after = full_loss()
    print(f"full-graph loss {before:.4f} -> {after:.4f}")
    assert after < before, (before, after)
