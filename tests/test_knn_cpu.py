"""k nearest neighbours without a GPU: the numpy twin against the reference's recorded hypergraph construction and against
brute force, the binding's limits and workspace rule against the header, and the checks that run before any native call."""
import ctypes
import glob
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import gcn_amd
from gcn_amd import _lib
from knn_ref import dist2_ref, keys_ref, knn_hypergraph_ref, knn_ref, laplacian_dense_ref, select_ref
from util import GOLDEN, ROOT

INVALID = 1                                            # GCN_ERR_INVALID_ARG
GOLDEN_FILES = sorted(glob.glob(os.path.join(GOLDEN, "knn_hypergraph_*.npz")))


def test_new_symbols_exported_and_bound():
    lib = ctypes.CDLL(gcn_amd.LIB_PATH)
    for name, nargs in (("gcn_knn_splits", 3), ("gcn_knn_ws_bytes", 5), ("gcn_knn_f32", 16)):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        fn = getattr(gcn_amd.load_library(), name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs
    assert gcn_amd.load_library().gcn_knn_f32.argtypes[-1] is ctypes.c_void_p
    assert callable(gcn_amd.knn) and callable(gcn_amd.knn_graph) and callable(gcn_amd.knn_hypergraph)
    assert gcn_amd.KNN_K_MAX == _lib.KNN_K_MAX


def test_limits_of_the_binding_are_the_headers_and_the_workspace_rule_is_the_librarys():
    text = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    for macro, value in (("GCN_KNN_K_MAX", _lib.KNN_K_MAX), ("GCN_KNN_TILE_Q", _lib.KNN_TILE_Q), ("GCN_KNN_TILE_C", _lib.KNN_TILE_C)):
        m = re.search(r"#define\s+" + macro + r"\s+(\d+)\b", text)
        assert m and int(m.group(1)) == value, macro
    lib = gcn_amd.load_library()
    cus = lib.gcn_device_cu_count()
    cus = cus if cus > 0 else 256                        # (no device: the library assumes 256 CUs, as its plans do)
    for q, n, k, splits in ((0, 0, 1, 0), (1, 1, 1, 1), (1, 0, 3, 0), (65, 1000, 10, 0), (65, 1000, 10, 3), (65, 1000, 64, 1000),
                            (12000, 12311, 10, 0), (1024, 10 ** 6, 32, 0), (1000, 10 ** 6, 64, 0), (10 ** 5, 10 ** 5, 16, 0),
                            (64, 63, 5, 7), (64, 65, 5, 7), (2 ** 31 - 1, 1, 1, 1)):
        out = ctypes.c_size_t(0)
        assert lib.gcn_knn_ws_bytes(q, n, k, splits, ctypes.byref(out)) == 0, (q, n, k, splits)
        s = lib.gcn_knn_splits(q, n, splits)
        tiles = -(-n // _lib.KNN_TILE_C)
        assert s == _lib.knn_splits(q, n, splits, cus) and 1 <= s <= max(tiles, 1)
        if splits >= 1:
            assert s == max(1, min(splits, tiles))       # taken as given, clamped to the tiles
        assert out.value == _lib.knn_ws_bytes(q, n, k, splits, cus) == 16 + (8 * q * s * (k + 1) + 15) // 16 * 16
    # the rule the header states for splits = 0, in plain numbers: 12 000 queries are 188 workgroups, 1 024 are 16
    assert _lib.knn_splits(12000, 12311, 0, 256) == 3 and _lib.knn_splits(1024, 10 ** 6, 0, 256) == 32
    assert _lib.knn_splits(10 ** 5, 10 ** 5, 0, 256) == 1 and _lib.knn_splits(1, 200, 0, 256) == 1


def test_bad_arguments_are_rejected_before_any_launch():
    lib = gcn_amd.load_library()
    buf = (ctypes.c_int64 * 64)()                        # a host array stands in for pointers only looked at, never followed
    p = ctypes.cast(buf, ctypes.c_void_p)
    out = ctypes.c_size_t(0)
    for bad in ((-1, 5, 3, 0), (5, -1, 3, 0), (5, 5, 0, 0), (5, 5, _lib.KNN_K_MAX + 1, 0), (5, 5, 3, -1)):
        assert lib.gcn_knn_ws_bytes(*bad, ctypes.byref(out)) == INVALID, bad
    assert lib.gcn_knn_ws_bytes(5, 5, 3, 0, None) == INVALID
    assert lib.gcn_knn_ws_bytes(2 ** 31 - 1, 2 ** 31 - 1, 1, 2 ** 31 - 1, ctypes.byref(out)) == INVALID     # 2^31 workgroups or more
    ws = _lib.knn_ws_bytes(5, 7, 3, 0)
    # knn(x, ldx, y, ldy, q, n, d, k, self_offset, splits, out_idx, out_dist2, out_sum, ws, ws_bytes, stream)
    good = [p, 4, p, 6, 5, 7, 4, 3, -1, 0, p, p, p, p, ws, None]
    for i, bad in ((0, None), (2, None), (10, None), (13, None), (4, -1), (5, -1), (6, 0), (6, -1), (7, 0), (7, _lib.KNN_K_MAX + 1),
                   (1, 3), (3, 3), (8, -2), (9, -1), (14, ws - 1), (14, 0), (13, ctypes.c_void_p(p.value + 4))):
        args = list(good)
        args[i] = bad
        assert lib.gcn_knn_f32(*args) == INVALID, (i, bad)
    none = [None, 4, None, 6, 0, 7, 4, 3, -1, 0, None, None, None, None, 0, None]
    assert lib.gcn_knn_f32(*none) == 0                   # no queries: nothing is looked at
    none[7] = 0
    assert lib.gcn_knn_f32(*none) == INVALID             # ... but the sizes are


def test_python_checks_come_in_the_documented_order():
    cpu = torch.zeros((4, 3))
    for fn in (gcn_amd.knn, gcn_amd.knn_graph, gcn_amd.knn_hypergraph):
        with pytest.raises(TypeError):                   # the type comes before everything, a bad k included
            fn(np.zeros((4, 3), np.float32), 0)
        with pytest.raises(TypeError):
            fn(cpu.double(), 0)
        with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):    # the device comes before the shape and before k
            fn(torch.zeros(4), 0)
        with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):
            fn(cpu, 2)
    with pytest.raises(TypeError):
        gcn_amd.knn(cpu, 2, y=cpu.half())
    with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):
        gcn_amd.knn(cpu, 2, y=torch.zeros((4, 5)))

    class _Dev(torch.Tensor):
        """a CPU tensor that claims to live on a device: enough to reach the checks behind the device check"""
        is_cuda = True

    x = torch.zeros((4, 3)).as_subclass(_Dev)
    with pytest.raises(ValueError, match="2-D"):
        gcn_amd.knn(torch.zeros(4).as_subclass(_Dev), 2)
    with pytest.raises(ValueError, match="columns"):
        gcn_amd.knn(x, 2, y=torch.zeros((4, 5)).as_subclass(_Dev))
    for bad in (0, -1, gcn_amd.KNN_K_MAX + 1, 2.0, True):
        for fn in (gcn_amd.knn, gcn_amd.knn_graph, gcn_amd.knn_hypergraph):
            with pytest.raises(ValueError, match="k must be"):
                fn(x, bad)
    with pytest.raises(ValueError, match="exclude_self"):
        gcn_amd.knn(x, 2, y=x, exclude_self=True)
    with pytest.raises(ValueError, match="values"):
        gcn_amd.knn_graph(x, 2, values="weights")
    with pytest.raises(ValueError, match="m_prob"):
        gcn_amd.knn_hypergraph(x, 2, m_prob=0.0)
    assert "No host synchronisation" in gcn_amd.knn.__doc__ and "normalize_csr(symmetrize(knn_graph(x, k))" in gcn_amd.knn_graph.__doc__


# ---- the numpy twin ------------------------------------------------------------------------------------------------------------
def _fl32(v):
    """a positive Fraction rounded to the nearest fp32, ties to even (normal range)"""
    e = math.floor(math.log2(v))
    while Fraction(2) ** e > v:
        e -= 1
    while Fraction(2) ** (e + 1) <= v:
        e += 1
    quantum = Fraction(2) ** (e - 23)
    return float(round(v / quantum) * quantum)          # (round() of a Fraction rounds halves to even)


def test_twin_distance_is_the_stated_chain_with_one_rounding_per_step():
    rng = np.random.default_rng(5)
    a = (rng.standard_normal((12, 9)) * np.exp2(rng.integers(-6, 7, (12, 1)))).astype(np.float32)
    b = (rng.standard_normal((14, 9)) * np.exp2(rng.integers(-6, 7, (14, 1)))).astype(np.float32)
    got = dist2_ref(a, b)
    for i in range(12):
        for j in range(14):
            acc = Fraction(0)
            for c in range(9):
                diff = Fraction(float(np.float32(a[i, c] - b[j, c])))
                v = diff * diff + acc
                acc = Fraction(_fl32(v)) if v > 0 else Fraction(0)
            assert float(acc) == float(got[i, j]), (i, j)
    assert np.array_equal(dist2_ref(a, a).diagonal(), np.zeros(12, np.float32))
    assert np.array_equal(dist2_ref(a, b).view(np.uint32), dist2_ref(b, a).T.view(np.uint32))


@pytest.mark.parametrize("k, self_offset", [(1, -1), (7, -1), (7, 0), (30, 3), (64, -1)])
def test_twin_selection_on_an_integer_grid_with_massive_ties(k, self_offset):
    g = np.stack(np.meshgrid(np.arange(7), np.arange(6), indexing="ij"), axis=-1).reshape(-1, 2).astype(np.float32)   # 42 points
    y = np.concatenate([g, g[::-1][:15]])                 # ... and 15 duplicates: 57 candidates
    x = y[max(self_offset, 0):max(self_offset, 0) + 20]
    idx, d2, rsum = knn_ref(x, y, k, self_offset)
    for i in range(len(x)):                               # brute force: a Python sort of (distance, index) pairs
        pairs = sorted((float(((x[i] - y[j]) ** 2).sum()), j) for j in range(len(y)) if self_offset < 0 or j != self_offset + i)
        want = pairs[:k] + [(np.inf, -1)] * (k - len(pairs[:k]))
        assert [p[1] for p in want] == idx[i].tolist() and [p[0] for p in want] == d2[i].tolist()
        assert rsum[i] == pytest.approx(sum(math.sqrt(((x[i] - y[j]) ** 2).sum()) for j in range(len(y))), rel=1e-14)


def test_twin_keys_put_nan_of_either_sign_behind_infinity_and_tie_them():
    d2 = np.array([[np.inf, np.nan, 0.0, -np.nan, 3.0]], np.float32)
    d2.view(np.uint32)[0, 3] |= 0x80000000
    idx, out = select_ref(keys_ref(d2), 5)
    assert idx.tolist() == [[2, 4, 0, 1, 3]] and np.isnan(out[0, 3:]).all() and out[0, 2] == np.inf


@pytest.mark.parametrize("path", GOLDEN_FILES, ids=[os.path.basename(f)[:-4] for f in GOLDEN_FILES])
def test_twin_hypergraph_rule_is_the_references_construction(path):
    """the recorded H and G are the reference's Eu_dis + construct_H_with_KNN_from_distance + generate_G_from_H in fp64 on
    inputs whose smallest relative gap between the last member and the first non-member is at least 1e-4
    (tools/make_knn_golden.py refuses others)"""
    z = np.load(path)
    x, k, Href, Gref = z["x"], int(z["k"]), z["H"], z["G"]
    assert float(z["gap"]) >= 1e-4 and x.dtype == np.float32
    H = knn_hypergraph_ref(x, k)
    assert np.array_equal(H != 0, Href != 0) and np.all((Href != 0).sum(axis=0) == k)
    rel = np.abs(H - Href)[Href != 0] / Href[Href != 0]
    print("H: largest relative difference", rel.max())
    assert rel.max() <= 1e-12 and np.all(H.diagonal() == 1.0)
    G = laplacian_dense_ref(H)
    print("G: largest difference", np.abs(G - Gref).max(), "of", np.abs(Gref).max())
    assert np.all(np.abs(G - Gref) <= 1e-12 * np.abs(Gref).max()) and np.array_equal(G != 0, Gref != 0)
    assert np.array_equal(knn_hypergraph_ref(x, k, prob=False), (Href != 0).astype(np.float64))


def test_there_are_three_golden_hypergraphs():
    assert len(GOLDEN_FILES) == 3
