"""The long-row dispatch of gcn_amd/csrc/row_dispatch.h beyond its first step, for every op that goes through it: the
neighbour sample, the induced subgraph (count and fill), the merge (count and fill), the degrees and the normalisation.
The matrices of the other tests have at most a few thousand rows, so there the long kernel's workgroup b sees one item, one
screening window and at most one long row.  Here one matrix of 257 * G + 3 rows (G = 1024, the long kernel's grid) has its
rows of more than LONG entries where the screening loop takes its other branches:
  5, 5 + G            one workgroup, one window, two long rows served one after the other
  7 + 255 * G         the last slot of the first window of 256 items
  7 + 256 * G, 9 + 256 * G    the second window
  m - 1               the last item, the last of its workgroup's items
and a row of exactly LONG entries at 5 + 2 * G, which belongs to the wave kernel.  Every other row is empty, except one in
fifty with 3 entries.  Seeds, nodes and rows are all m items.  A second call of every op takes the rows 6 + G .. 5 + 2 * G
(QUIET): more than LONG entries in all and no row over LONG, the exactly-LONG row last — the long kernel is launched and
leaves on the flag (or, for the ops without a flag, screens and finds nothing).  A prefix of the matrix cannot serve for
this: the rows before the first long one hold next to no entries.  Everything is compared with the host twins, integer for
integer and (values in eighths: every sum is exact in any order) bit for bit; the normalisation by the twin's own measure,
one ulp of the rounded fp64 product."""
import numpy as np
import pytest
import torch

import gcn_amd
from gcn_amd import _lib
from coalesce_ref import coalesce_ref, degree_ref, normalize_ref, within_one_ulp
from sampling_ref import sample_neighbors_ref
from subgraph_ref import induced_subgraph_ref
from test_coalesce_gpu import check_coalesce, raw_degree, raw_normalize
from test_sampling_gpu import _assert_sample
from test_subgraph_gpu import _assert_subgraph

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
G = 1024
LONG = _lib.SAMPLE_LONG_ROW
M = 257 * G + 3
NV = M + M // 9                                        # vertices: the last tenth has no row and is in no node set
LONG_AT = [5, 5 + G, 7 + 255 * G, 7 + 256 * G, 9 + 256 * G, M - 1]
EXACT_AT = 5 + 2 * G
QUIET = (6 + G, EXACT_AT + 1)                          # a stretch of rows with more than LONG entries and no long row

_CACHE = {}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _matrix():
    """(rowptr [M + 1], col, val), column-sorted: the columns of a long row are multiples of a step that spreads 1.3 x its
    length over [0, NV), drawn with replacement — about a third of its entries repeat a column and a tenth point at a vertex
    without a row; a short row is (c, c, c') ; values are eighths"""
    if "matrix" not in _CACHE:
        rng = np.random.default_rng(20)
        lens = np.where(rng.random(M) < 0.02, 3, 0)
        lens[LONG_AT] = LONG + 1 + np.arange(len(LONG_AT)) * 37
        lens[EXACT_AT] = LONG
        rp = np.zeros(M + 1, np.int64)
        rp[1:] = np.cumsum(lens)
        ci = np.empty(rp[-1], np.int64)
        for r in np.flatnonzero(lens):
            L = lens[r]
            if L == 3:
                c = np.sort(rng.integers(0, NV, 2))
                ci[rp[r]:rp[r + 1]] = [c[0], c[0], c[1]]
            else:
                K = int(1.3 * L)
                ci[rp[r]:rp[r + 1]] = np.sort(rng.integers(0, K, L)) * (NV // K)
        va = (rng.integers(1, 9, len(ci)) / 8).astype(np.float32)
        assert 25000 < len(ci) < 32000 and ci.max() < NV and lens.max() == LONG + 1 + 5 * 37
        assert 0.05 < np.mean(ci >= M) < 0.15
        _CACHE["matrix"] = (rp.astype(np.int32), ci.astype(np.int32), va)
    return _CACHE["matrix"]


def _square():
    """the matrix as an NV x NV adjacency (the rows past M empty) and its row pointer"""
    if "square" not in _CACHE:
        rp, ci, va = _matrix()
        rps = np.concatenate([rp, np.full(NV - M, rp[-1], np.int32)])
        _CACHE["square"] = (rps, gcn_amd.CsrAdjacency(_t(rps), _t(ci), _t(va), (NV, NV)))
    return _CACHE["square"]


def _quiet_matrix():
    rp, ci, va = _matrix()
    a, b = QUIET
    lo, hi = rp[a], rp[b]
    assert hi - lo > LONG and np.diff(rp[a:b + 1]).max() == LONG
    return rp[a:b + 1] - lo, ci[lo:hi], va[lo:hi], b - a


def test_shape_reaches_every_branch_of_the_screening_loop():
    rp, _, _ = _matrix()
    long_rows = np.flatnonzero(np.diff(rp) > LONG)
    assert long_rows.tolist() == LONG_AT and M > 256 * G
    q = long_rows // G                                   # a row's place among its workgroup's items
    assert q.tolist() == [0, 1, 255, 256, 256, 257] and (long_rows % G).tolist() == [5, 5, 7, 7, 9, 2]
    assert rp[EXACT_AT + 1] - rp[EXACT_AT] == LONG


@pytest.mark.parametrize("fanout", [10, -1])
def test_sample_neighbors(fanout):
    rp, ci, _ = _matrix()
    _, adj = _square()
    for seeds in (np.arange(M), np.arange(*QUIET)):
        got = gcn_amd.sample_neighbors(adj, _t(seeds), fanout, seed=77, offset=5)
        _assert_sample(got, sample_neighbors_ref(rp, ci, seeds, fanout, 77, 5), f"fanout {fanout}, {len(seeds)} seeds")


def test_induced_subgraph():
    _, ci, va = _matrix()
    rps, adj = _square()
    for nodes in (np.arange(M), np.arange(*QUIET)):
        want = induced_subgraph_ref(rps, ci, nodes, NV)
        if len(nodes) == M:                              # (the long rows lose entries, and keep most)
            kept = np.diff(want[0])[LONG_AT]
            assert np.all(kept < LONG) and np.all(kept > LONG // 2)
        _assert_subgraph(gcn_amd.induced_subgraph(adj, _t(nodes)), want, nodes, va, f"{len(nodes)} nodes")


@pytest.mark.parametrize("diagonal", ["keep", "fill"])
def test_coalesce(diagonal):
    rp, ci, va = _matrix()
    out, _ = check_coalesce(rp, ci, va, M, NV, "sum", diagonal, 0.5)
    assert diagonal != "keep" or out.nnz < 0.85 * len(ci)                        # (repeated pairs were merged)
    qrp, qci, qva, qm = _quiet_matrix()
    check_coalesce(qrp, qci, qva, qm, NV, "sum", diagonal, 0.5)


def test_degree_and_normalize():
    for rp, ci, va, m in (_matrix() + (M,), _quiet_matrix()):
        rpd, cid, vad = _t(rp), _t(ci), _t(va)
        want = degree_ref(rp, va)
        deg = raw_degree(rpd, vad, m)
        assert np.array_equal(deg.cpu().numpy(), want)    # (sums of eighths: exact)
        assert np.array_equal(raw_degree(rpd, None, m).cpu().numpy(), degree_ref(rp, None))
        # the scales of the columns: a square matrix's degrees.  Here any positive table of NV entries serves
        table = np.concatenate([want, np.ones(NV - m)]) + 1.0
        out = raw_normalize(rpd, cid, vad, m, NV, _t(table), "row").cpu().numpy()
        assert np.all(np.isfinite(out)) and np.all(within_one_ulp(out, normalize_ref(rp, ci, va, table, "row")))
        sq = np.concatenate([rp, np.full(NV - m, rp[-1], np.int32)])         # "sym" takes a square matrix: empty rows behind
        out = raw_normalize(_t(sq), cid, vad, NV, NV, _t(table), "sym").cpu().numpy()
        assert np.all(np.isfinite(out)) and np.all(within_one_ulp(out, normalize_ref(sq, ci, va, table, "sym")))
