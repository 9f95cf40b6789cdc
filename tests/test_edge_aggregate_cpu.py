"""Edge-feature aggregation without a GPU: the three entry points are declared, exported, bound and built; bad arguments are
refused and empty problems accepted before a pointer is read (a problem whose edge_feat has 2^31 elements or more is
ACCEPTED by the argument check); gcn_amd.edge_aggregate raises the documented error types; the numpy twins of
tests/edge_aggregate_ref.py agree with a dense torch fp64 autograd formulation; GINEConv / GINConv construct with stable
state-dict keys; and a 32-bit offset into edge_feat or its gradient changes what tests/test_edge_aggregate_large_gpu.py
compares."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import edge_aggregate_large_ref as big
import edge_aggregate_ref as ref
import gcn_amd
from gcn_amd import _lib, build, edgefeat
from util import ROOT

NEW = {"gcn_edge_aggregate_csr_f32": 16, "gcn_edge_aggregate_backward_x_csr_f32": 16, "gcn_edge_aggregate_backward_e_csr_f32": 15}
INVALID = 1                                            # GCN_ERR_INVALID_ARG
ADD, MUL, NONE, RELU, MAX, MIN, SUM = 0, 1, 0, 1, 0, 1, 2
OPS = [("add", None), ("add", "relu"), ("mul", None), ("mul", "relu")]
REDUCES = ["sum", "mean", "max", "min"]


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(NEW))
def test_new_symbols_declared_exported_and_bound(name):
    lib = ctypes.CDLL(gcn_amd.LIB_PATH)
    assert hasattr(lib, name)
    assert name in _lib.SIGNATURES
    fn = getattr(gcn_amd.load_library(), name)
    assert fn.restype is ctypes.c_int
    assert fn.argtypes == _lib.SIGNATURES[name][1]
    assert len(fn.argtypes) == NEW[name]
    assert fn.argtypes[-1] is ctypes.c_void_p          # (void* stream last)
    assert fn.argtypes[-2] is ctypes.c_size_t          # (the workspace's size before it)
    header = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    assert re.search(r"\bint " + name + r"\(", header)


def test_unit_is_built_and_exported_from_the_package():
    assert "edge_message.hip" in build.SOURCES and "edge_message.h" in build.HEADERS
    assert os.path.exists(os.path.join(build.CSRC, "edge_message.hip"))
    assert gcn_amd.edge_aggregate is edgefeat.edge_aggregate
    assert gcn_amd.GINEConv.__module__ == gcn_amd.GINConv.__module__ == "gcn_amd.layers"


def test_header_constants_match_the_binding():
    text = open(os.path.join(ROOT, "include", "gcn_spmm.h")).read()
    for name, value in (("GCN_EDGE_OP_ADD", _lib.EDGE_OP_ADD), ("GCN_EDGE_OP_MUL", _lib.EDGE_OP_MUL),
                        ("GCN_EDGE_ACT_NONE", _lib.EDGE_ACT_NONE), ("GCN_EDGE_ACT_RELU", _lib.EDGE_ACT_RELU),
                        ("GCN_REDUCE_MAX", _lib.REDUCE_MAX), ("GCN_REDUCE_MIN", _lib.REDUCE_MIN), ("GCN_REDUCE_SUM", _lib.REDUCE_SUM)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", text), name
    assert (_lib.REDUCE_MAX, _lib.REDUCE_MIN, _lib.REDUCE_SUM) == (0, 1, 2)
    m = re.search(r"#define\s+GCN_EDGE_AGGREGATE_WS_BYTES\(nnz, k\)\s+\(16 \+ 16 \* \(size_t\)\(k\) \* \(\(\(size_t\)\(nnz\) \+ (\d+)\) / (\d+)\)\)",
                  text)
    assert m and int(m.group(1)) + 1 == int(m.group(2)) == edgefeat._CHUNK
    for nnz, k in ((0, 1), (1, 1), (4096, 128), (4097, 128), (114_848_857, 64)):
        assert edgefeat._ws_bytes(nnz, k) == 16 + 16 * k * ((nnz + 4095) // 4096)


def _calls():
    """the three functions with a full argument list each (p: a pointer only looked at) and the positions of its pointers"""
    lib = gcn_amd.load_library()
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)              # a host array stands in for pointers only looked at, never followed
    huge = 1 << 40
    fwd = (lib.gcn_edge_aggregate_csr_f32, [p, p, 3, 3, 4, p, p, 8, ADD, RELU, MAX, p, p, p, huge, None],
           (0, 1, 5, 6, 11, 12, 13), {"m": 2, "nnz": 4, "k": 7, "op": 8, "act": 9, "ws_bytes": 14})
    bx = (lib.gcn_edge_aggregate_backward_x_csr_f32, [p, p, p, 3, 3, 4, p, p, p, 8, MUL, RELU, p, p, huge, None],
          (0, 1, 2, 6, 7, 8, 12, 13), {"m": 3, "nnz": 5, "k": 9, "op": 10, "act": 11, "ws_bytes": 14})
    be = (lib.gcn_edge_aggregate_backward_e_csr_f32, [p, p, 3, 3, 4, p, p, p, 8, ADD, NONE, p, p, huge, None],
          (0, 1, 5, 6, 7, 11, 12), {"m": 2, "nnz": 4, "k": 8, "op": 9, "act": 10, "ws_bytes": 13})
    return fwd, bx, be


def test_bad_arguments_are_rejected_before_a_pointer_is_read():
    """every refusal happens on the sizes, the constants, a null pointer or the workspace's size: the pointers handed in are
    a 256-byte host array, which no call may follow (a full list of them is never passed)"""
    for fn, args, pointers, at in _calls():
        for i in pointers:                                          # each pointer in turn
            a = list(args)
            a[i] = None
            assert fn(*a) == INVALID, (fn.__name__, i)
        for key, bad in (("m", -1), ("nnz", -4), ("k", 0), ("k", -8), ("k", 16 * 65535 + 1), ("op", 2), ("op", -1), ("act", 2)):
            a = list(args)
            a[at[key]] = bad
            assert fn(*a) == INVALID, (fn.__name__, key, bad)
        a = list(args)
        a[at["ws_bytes"]] = edgefeat._ws_bytes(4, 8) - 1            # a workspace one byte short
        assert fn(*a) == INVALID, fn.__name__
    fwd, args, _, _ = _calls()[0]
    for reduce in (3, -1):
        a = list(args)
        a[10] = reduce
        assert fwd(*a) == INVALID
    # an unknown constant or k < 1 is refused on an empty problem too
    assert fwd(None, None, 0, 0, 0, None, None, 8, 5, NONE, SUM, None, None, None, 0, None) == INVALID
    assert fwd(None, None, 0, 0, 0, None, None, 0, ADD, NONE, SUM, None, None, None, 0, None) == INVALID
    assert fwd(None, None, 0, 0, 0, None, None, 8, ADD, NONE, 7, None, None, None, 0, None) == INVALID


def test_problems_without_output_rows_are_ok_and_launch_nothing():
    lib = gcn_amd.load_library()
    assert lib.gcn_edge_aggregate_csr_f32(None, None, 0, 0, 0, None, None, 8, ADD, NONE, SUM, None, None, None, 0, None) == 0
    assert lib.gcn_edge_aggregate_csr_f32(None, None, 0, 7, 0, None, None, 3, MUL, RELU, MIN, None, None, None, 0, None) == 0
    assert lib.gcn_edge_aggregate_backward_x_csr_f32(None, None, None, 0, 5, 0, None, None, None, 8, ADD, RELU, None, None, 0, None) == 0
    assert lib.gcn_edge_aggregate_backward_e_csr_f32(None, None, 0, 5, 0, None, None, None, 8, ADD, RELU, None, None, 0, None) == 0
    # rows but no entry: the gradient in edge_feat has no element
    assert lib.gcn_edge_aggregate_backward_e_csr_f32(None, None, 4, 5, 0, None, None, None, 8, MUL, NONE, None, None, 0, None) == 0


def test_edge_feat_of_2_31_elements_and_more_is_accepted():
    """nnz * k >= 2^31 is no bound of the ABI: with m == 0 (n == 0 for the walk of the transposed pattern) nothing runs,
    and the argument check answers GCN_OK for the Reddit-shaped size and for the largest nnz an int32 holds"""
    lib = gcn_amd.load_library()
    for nnz, k in ((114_848_857, 64), (2 ** 31 - 1, 512), (2 ** 25, 64), (2 ** 22 + 16_000, 512)):
        assert nnz * k >= 2 ** 31
        for reduce in (SUM, MAX, MIN):
            assert lib.gcn_edge_aggregate_csr_f32(None, None, 0, 5, nnz, None, None, k, ADD, RELU, reduce, None, None, None, 0, None) == 0
        assert lib.gcn_edge_aggregate_backward_x_csr_f32(None, None, None, 0, 5, nnz, None, None, None, k, MUL, NONE, None, None, 0,
                                                         None) == 0
        assert lib.gcn_edge_aggregate_backward_e_csr_f32(None, None, 0, 5, nnz, None, None, None, k, MUL, NONE, None, None, 0, None) == 0
        assert edgefeat._ws_bytes(nnz, k) == 16 + 16 * k * ((nnz + 4095) // 4096)      # (Python integers: no wrap)


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------
class _FakeAdj(gcn_amd.CsrAdjacency):
    """a CsrAdjacency shell with host arrays (the constructor refuses CPU tensors): enough to reach the checks that run
    before any native call"""

    def __init__(self):
        self.m, self.n = 3, 5
        self.nnz = 4
        self.rowptr = torch.tensor([0, 2, 3, 4], dtype=torch.int32)
        self.col = torch.tensor([0, 1, 4, 0], dtype=torch.int32)
        self.val = torch.ones(4)
        self.device = torch.device("cpu")
        self.mutable_values = False
        self._plan = None
        self._transpose = None


def test_edge_aggregate_raises_the_documented_errors():
    adj, x, w = _FakeAdj(), torch.ones(5, 2), torch.ones(4, 2)
    with pytest.raises(TypeError):
        gcn_amd.edge_aggregate(torch.eye(3).to_sparse(), x, w)
    with pytest.raises(ValueError, match="op"):
        gcn_amd.edge_aggregate(adj, x, w, op="sub")
    with pytest.raises(ValueError, match="act"):
        gcn_amd.edge_aggregate(adj, x, w, act="gelu")
    with pytest.raises(ValueError, match="reduce"):
        gcn_amd.edge_aggregate(adj, x, w, reduce="median")
    for reduce in ("sum", "mean"):
        with pytest.raises(ValueError, match="return_arg"):
            gcn_amd.edge_aggregate(adj, x, w, reduce=reduce, return_arg=True)
    for bad_x in (torch.ones(3, 2), torch.ones(5), torch.ones(5, 2, 1), torch.ones(5, 0), [[1.0, 1.0]] * 5):
        with pytest.raises(ValueError):                # the shape comes before the device: a ValueError, CPU tensor or not
            gcn_amd.edge_aggregate(adj, bad_x, w)
    for bad_w in (torch.ones(3, 2), torch.ones(4, 3), torch.ones(4), torch.ones(4, 2, 1), None):
        with pytest.raises(ValueError, match="edge_feat"):
            gcn_amd.edge_aggregate(adj, x, bad_w)
    for reduce in REDUCES:
        with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):
            gcn_amd.edge_aggregate(adj, x.clone().requires_grad_(), w, reduce=reduce)
    with pytest.raises(gcn_amd.GcnAmdError):           # (the device comes before the dtype)
        gcn_amd.edge_aggregate(adj, x.double(), w.double())


def test_route_follows_the_documented_rule():
    class At:
        def __init__(self, address):
            self.address = address

        def data_ptr(self):
            return self.address

    for k, lps, tiles in ((4, 16, 1), (64, 16, 1), (68, 32, 1), (128, 32, 1), (132, 64, 1), (256, 64, 1), (260, 64, 2)):
        assert edgefeat.route(k, At(256), At(512)) == (4, lps, tiles), k
    for k, lps, tiles in ((1, 16, 1), (3, 16, 1), (5, 16, 1), (17, 32, 1), (33, 64, 1), (65, 64, 2)):
        assert edgefeat.route(k, At(256)) == (1, lps, tiles), k
    assert edgefeat.route(64, At(256), At(516)) == (1, 64, 1)       # one operand off a 16-byte boundary


# ---- the twins against dense torch fp64 autograd ---------------------------------------------------------------------------------------
def _small_problem(seed):
    """a graph with empty rows and duplicates; operands with 11 significant bits, so that the float32 message (a sum or a
    product of two of them) is exact and the fp64 formulation sees the same numbers"""
    rng = np.random.default_rng(seed)
    m, n, k = 23, 17, 5
    lens = rng.integers(0, 9, m)
    lens[[2, 11]] = 0
    rowptr = np.zeros(m + 1, np.int64)
    rowptr[1:] = np.cumsum(lens)
    col = rng.integers(0, n, rowptr[-1])
    x = (rng.integers(-1023, 1024, (n, k)) / 256.0).astype(np.float32)
    w = (rng.integers(-1023, 1024, (len(col), k)) / 256.0).astype(np.float32)
    g = (rng.integers(-1023, 1024, (m, k)) / 256.0).astype(np.float32)
    return rowptr, col, n, x, w, g


def _torch_formulation(rowptr, col, x, w, g, op, act, reduce):
    """out, gx, ge in fp64: messages as an [nnz, k] tensor reduced with index_add_ / scatter_reduce"""
    m, k = len(rowptr) - 1, x.shape[1]
    rows = torch.from_numpy(ref.entry_rows(rowptr))
    xt = torch.from_numpy(x).double().requires_grad_()
    wt = torch.from_numpy(w).double().requires_grad_()
    msg = xt[torch.from_numpy(col)] * wt if op == "mul" else xt[torch.from_numpy(col)] + wt
    if act == "relu":
        msg = msg.relu()
    if reduce in ("sum", "mean"):
        out = torch.zeros(m, k, dtype=torch.float64).index_add_(0, rows, msg)
        if reduce == "mean":
            out = out / torch.from_numpy(np.maximum(np.diff(rowptr), 1)).double()[:, None]
    else:
        out = torch.zeros(m, k, dtype=torch.float64).scatter_reduce(0, rows[:, None].expand(-1, k), msg,
                                                                    "amax" if reduce == "max" else "amin", include_self=False)
    out.backward(torch.from_numpy(g).double())
    return out.detach().numpy(), xt.grad.numpy(), wt.grad.numpy()


@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("op,act", OPS)
def test_twins_agree_with_dense_torch_fp64_autograd(op, act, reduce):
    rowptr, col, n, x, w, g = _small_problem(seed=3)
    want_out, want_gx, want_ge = _torch_formulation(rowptr, col, x, w, g, op, act, reduce)
    if reduce in ("max", "min"):
        out, arg = ref.forward(rowptr, col, x, w, op, act, reduce)
        msg = ref.messages(col, x, w, op, act)
        for r in range(len(rowptr) - 1):               # torch splits a gradient among ties: the comparison needs a unique
            seg = msg[rowptr[r]:rowptr[r + 1]]         # winner wherever a gradient flows
            if len(seg):
                best = seg.max(0) if reduce == "max" else seg.min(0)
                tied = (seg == best).sum(0) > 1
                assert not np.any(tied & ~((act == "relu") & (best == 0))), "choose another seed: a tie carries a gradient"
        gx, _mag, ge = ref.backward_select(rowptr, col, n, x, w, g, arg, op, act)
    else:
        out, _mag = ref.forward(rowptr, col, x, w, op, act, reduce)
        if reduce == "mean":                           # the mean's backward is the sum's on g / len: hand torch g * len, so
            lens = np.maximum(np.diff(rowptr), 1)[:, None]        # that the float32 quotient the twin is given is exact
            _, want_gx, want_ge = _torch_formulation(rowptr, col, x, w, (g * lens).astype(np.float32), op, act, reduce)
        gx, _mag, ge = ref.backward_sum(rowptr, col, n, x, w, g, op, act)
    np.testing.assert_allclose(np.asarray(out, np.float64), want_out, rtol=1e-12, atol=0)
    np.testing.assert_allclose(gx, want_gx, rtol=1e-12, atol=0)
    np.testing.assert_allclose(ge.astype(np.float64), want_ge, rtol=1e-12, atol=0)


def test_twin_selection_follows_the_nan_and_tie_rules():
    rowptr = np.array([0, 4, 4, 7, 9])
    col = np.array([0, 1, 2, 3, 0, 1, 2, 3, 0])
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    x = np.array([[1.0], [1.0], [nan], [nan]], np.float32)                      # row 0: a tie, then two NaN
    x = np.concatenate([x, np.array([[-0.0], [0.0], [-inf], [inf], [-inf]], np.float32)])[:4]
    w = np.zeros((9, 1), np.float32)
    out, arg = ref.forward(rowptr, col, x, w, "add", None, "max")
    assert np.isnan(out[0, 0]) and arg[0, 0] == 2                               # the first NaN, not the tie before it
    assert out[1, 0] == 0 and arg[1, 0] == -1                                   # an empty row
    x2, w = np.array([[-0.0], [0.0], [-inf], [inf]], np.float32), np.ones((9, 1), np.float32)
    for reduce, row2, row3 in (("max", (0, 4), (inf, 7)), ("min", (-inf, 6), (-0.0, 8))):
        out, arg = ref.forward(rowptr, col, x2, w, "mul", None, reduce)
        assert (out[2, 0], arg[2, 0]) == row2 and (out[3, 0], arg[3, 0]) == row3
    out, arg = ref.forward(rowptr, col, x2, w, "mul", None, "max")
    assert np.signbit(out[2, 0]) and arg[2, 0] == 4                             # -0.0 first among -0.0, +0.0, -inf: its bits
    out, arg = ref.forward(rowptr, col, x2, w, "mul", "relu", "min")
    assert out[2, 0] == 0 and np.signbit(out[2, 0]) and arg[2, 0] == 4          # relu keeps -0.0, relu(-inf) = +0: a tie of three
    assert out[0, 0] == 0 and arg[0, 0] == 0 and np.isinf(ref.activate(inf, "relu"))
    assert np.isnan(ref.activate(nan, "relu")) and ref.passes(nan, "relu") and not ref.passes(np.float32(0), "relu")


# ---- the layers -------------------------------------------------------------------------------------------------------------------------
def test_gin_layers_construct_with_stable_state_dict_keys():
    net = torch.nn.Sequential(torch.nn.Linear(6, 8), torch.nn.ReLU(), torch.nn.Linear(8, 4))
    gine = gcn_amd.GINEConv(net)
    assert list(gine.state_dict()) == ["eps", "nn.0.weight", "nn.0.bias", "nn.2.weight", "nn.2.bias"]
    assert gine.lin is None and not isinstance(gine.eps, torch.nn.Parameter) and float(gine.eps) == 0.0
    trained = gcn_amd.GINEConv(net, eps=0.25, train_eps=True, edge_dim=3)
    assert list(trained.state_dict()) == ["eps", "nn.0.weight", "nn.0.bias", "nn.2.weight", "nn.2.bias", "lin.weight", "lin.bias"]
    assert isinstance(trained.eps, torch.nn.Parameter) and float(trained.eps.detach()) == 0.25
    assert trained.lin.weight.shape == (6, 3)          # (in_features read off the network's first layer)
    assert gcn_amd.GINEConv(torch.nn.ReLU(), edge_dim=3, in_features=5).lin.weight.shape == (5, 3)
    with pytest.raises(ValueError, match="in_features"):
        gcn_amd.GINEConv(torch.nn.ReLU(), edge_dim=3)
    other = gcn_amd.GINEConv(torch.nn.Sequential(torch.nn.Linear(6, 8), torch.nn.ReLU(), torch.nn.Linear(8, 4)), train_eps=True,
                             edge_dim=3)
    other.load_state_dict(trained.state_dict())
    assert float(other.eps.detach()) == 0.25
    gin = gcn_amd.GINConv(torch.nn.Linear(6, 4), eps=0.5, train_eps=False)
    assert list(gin.state_dict()) == ["eps", "nn.weight", "nn.bias"] and float(gin.eps) == 0.5
    assert list(gcn_amd.GINConv(torch.nn.Linear(6, 4), 0.0, True).state_dict()) == ["eps", "nn.weight", "nn.bias"]
    adj = _FakeAdj()                                   # 3 x 5: not square
    with pytest.raises(ValueError, match="pair"):
        gin(torch.ones(5, 6), adj)
    with pytest.raises(ValueError):
        gine((torch.ones(5, 6), torch.ones(4, 6)), adj, torch.ones(4, 6))
    with pytest.raises(ValueError, match="edge_attr"):
        gine((torch.ones(5, 6), torch.ones(3, 6)), adj, torch.ones(4, 5))


# ---- what the large test proves ----------------------------------------------------------------------------------------------------------
def test_large_problem_passes_both_thresholds():
    rp = big.rowptr()
    nnz = int(rp[-1])
    assert 2 ** 22 < nnz < 2 ** 31 and nnz * big.K > 2 ** 31 and nnz * big.K * 4 > 2 ** 33
    assert big.E32 * big.K * 4 == 2 ** 32 and big.E31 * big.K == 2 ** 31
    assert rp[-1] - rp[-2] == big.LAST > 2 * 4096      # the last row: chunk partials, and entries past 2^22
    assert rp[-2] > big.E31                            # ... and short rows past 2^22 too
    rows, ents = big.compared_rows(rp), big.compared_entries(rp)
    for e in (big.E32, big.E31):
        r = np.searchsorted(rp, e, side="right") - 1
        assert r in rows and r - big.BAND in rows and r + big.BAND in rows and e in ents
    assert len(rows) < 600 and len(ents) < 700


def test_large_inputs_are_on_the_exact_grid():
    e = np.arange(0, 5_000_000, 37, dtype=np.int64)[:, None]
    j = np.arange(big.K, dtype=np.int64)[None, :]
    w, x, g = big.w_of(e, j), big.x_table(), big.g_of(e, j)
    assert np.array_equal(w * 8, np.round(w * 8)) and np.abs(w).max() <= 1 and len(np.unique(w)) == 17
    assert np.array_equal(x, np.round(x)) and np.abs(x).max() <= 3 and np.abs(g).max() <= 3
    # every message and every gradient term is a multiple of 1/8 of magnitude <= 4; the longest sums (the last row, a
    # column's 1 100 entries) stay below 2^24 eighths
    col = big.col_of(np.arange(int(big.rowptr()[-1]), dtype=np.int64))
    assert max(big.LAST, int(np.bincount(col).max())) * 4 * 8 < 2 ** 24


@pytest.mark.parametrize("trunc", ["byte32", "elem31"])
def test_a_32_bit_offset_changes_what_the_large_test_compares(trunc):
    rp = big.rowptr()
    first_bad = big.E32 if trunc == "byte32" else big.E31
    # the gather side: every compared row past the threshold gets another sum, another max and another arg
    rows = big.compared_rows(rp)
    past = rp[rows + 1] > first_bad                    # (the row holds an entry at or past the threshold)
    assert past.sum() >= big.BAND and (~past).sum() >= big.BAND
    good, bad = big.forward_rows(rp, rows, "add", "relu", "sum"), big.forward_rows(rp, rows, "add", "relu", "sum", trunc)
    assert np.array_equal(good[~past], bad[~past])
    assert np.all(np.any(good[past] != bad[past], axis=1))
    (gv, ga), (bv, ba) = big.forward_rows(rp, rows, "mul", None, "max"), big.forward_rows(rp, rows, "mul", None, "max", trunc)
    assert np.array_equal(ga[~past], ba[~past])
    assert np.all(np.any((gv[past] != bv[past]) | (ga[past] != ba[past]), axis=1))
    # ... and every compared column of the gradient in x that has an entry past the threshold
    cols = big.compared_cols(rp)
    col = big.col_of(np.arange(first_bad, int(rp[-1]), dtype=np.int64))
    hit = np.isin(cols, col)
    assert hit.sum() >= 12
    gx_good, gx_bad = big.grad_x_cols(rp, cols, "mul", None), big.grad_x_cols(rp, cols, "mul", None, trunc)
    assert np.all(np.any(gx_good[hit] != gx_bad[hit], axis=1)) and np.array_equal(gx_good[~hit], gx_bad[~hit])
    # the store side: a truncated offset writes a compared row of the gradient in edge_feat somewhere below the threshold
    # and nothing writes the row itself, which keeps the NaN the test filled it with
    ents = big.compared_entries(rp)
    late = ents[ents >= first_bad]
    assert len(late) >= 64
    landed, _ = big.trunc_entry_col(late[:, None], np.arange(big.K)[None, :], trunc)
    assert np.all(landed < first_bad) and np.all(landed != late[:, None])
    everyone, _ = big.trunc_entry_col(np.arange(first_bad, int(rp[-1]), dtype=np.int64), 0, trunc)
    assert everyone.max() < first_bad
