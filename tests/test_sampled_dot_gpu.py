"""The sampled sparse product on the GPU against the numpy twin of tests/sampled_dot_ref.py: every value bit for bit (the fold
order is the contract's), a NaN matching any NaN.  The shapes are the smallest that reach every path: X rows on both sides of
the group width (16), of the wave width and the group bound (64), of two wave steps (128) and of GCN_SAMPLE_LONG_ROW; Y rows
from empty to the whole width; P rows on both sides of the wave's four entries a pass, of 64 and of the long-row bound; both
modes.  Because the twin is plain Python, the long P rows point at short X rows and the long X rows are sampled by short P
rows (and by a few entries of the long ones): the twin visits about half a million entries of X in all."""
import ctypes

import numpy as np
import pytest
import torch

from gcn_amd import _lib
from sampled_dot_ref import sampled_dot_ref
from util import SENTINEL, guards_intact, offset_view

pytestmark = pytest.mark.gpu
DEV = "cuda"
LONG = _lib.SAMPLE_LONG_ROW
WIDTH = 6000                                            # the common column range of the main case
X_LENS = [0, 1, 15, 16, 17, 63, 64, 65, 128, 129, LONG, LONG + 1, 5000]
Y_LENS = [0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 1000, WIDTH]
P_LENS = [0, 1, 64, 65, LONG, LONG + 1, 3 * LONG]
BIG = np.float32(2.0 ** 24)
_cache = {}


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def same_values(got, want):
    """bit for bit, except that a NaN matches any NaN (which NaN an operation returns is not part of the contract)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(want[~nan]))


def _ptr(x):
    return ctypes.c_void_p(x.data_ptr()) if x is not None and x.numel() > 0 else None


def raw(p, x, y, np_cols, w, by_col=False, offsets=None, stream=None):
    """the raw call for numpy operands p = (rowptr, col), x / y = (rowptr, col, val or None) -> (out numpy with the sentinel
    where nothing was written, guards intact?).  offsets: element offsets past a 16-byte boundary, one per array in the order
    p, x, y, out (util.offset_view); None: plain tensors (out still sits between guards)."""
    arrays = [p[0], p[1], x[0], x[1], x[2], y[0], y[1], y[2]]
    offsets = list(offsets) if offsets is not None else [0] * 9
    dev = []
    for a, off in zip(arrays, offsets):
        if a is None or a.size == 0:                    # (an operand without entries hands over no array)
            dev.append(None)
        else:
            dtype = torch.float32 if a.dtype == np.float32 else torch.int32
            dev.append(offset_view(a, off, dtype, DEV)[0])
    out, flat = offset_view(len(p[1]), offsets[8], torch.float32, DEV)
    ws = torch.empty(_lib.SAMPLED_DOT_WS_BYTES, dtype=torch.uint8, device=DEV)
    st = ctypes.c_void_p(stream.cuda_stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    prp, pci, xrp, xci, xva, yrp, yci, yva = dev
    status = _lib.load().gcn_csr_sampled_dot_f32(_ptr(prp), _ptr(pci), len(p[0]) - 1, np_cols, len(p[1]), _ptr(xrp), _ptr(xci),
                                                 _ptr(xva), len(x[1]), _ptr(yrp), _ptr(yci), _ptr(yva), len(y[1]), w,
                                                 1 if by_col else 0, _ptr(out), _ptr(ws), ws.numel(), st)
    _lib.check(status, "gcn_csr_sampled_dot_f32")
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return out.cpu().numpy(), guards_intact(flat, out)


def twin(p, x, y, np_cols, w, by_col=False):
    """the twin's values, with the sentinel's bits where nothing is written"""
    out = np.full(len(p[1]), SENTINEL[4], np.int32).view(np.float32)
    return sampled_dot_ref(p[0], p[1], np_cols, *x, *y, w, x_by_col=by_col, out=out)


def same_with_unwritten(got, want):
    """same_values, the sentinel (a NaN payload) compared as bits"""
    s = bits(want) == SENTINEL[4]
    return np.array_equal(bits(got) == SENTINEL[4], s) and same_values(got[~s], want[~s])


def check(p, x, y, np_cols, w, by_col=False, **kw):
    got, intact = raw(p, x, y, np_cols, w, by_col, **kw)
    want = twin(p, x, y, np_cols, w, by_col)
    assert intact and same_with_unwritten(got, want)
    return got


def csr_of(rows, dtype=np.int32):
    rp = np.zeros(len(rows) + 1, np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    return rp, (np.concatenate([np.asarray(r, dtype) for r in rows]) if rp[-1] else np.zeros(0, dtype)).astype(dtype)


def values(rng, n):
    return (rng.standard_normal(n) * 0.5).astype(np.float32)


# ---- the main case -------------------------------------------------------------------------------------------------------------
def main_case(by_col):
    """X: a row of every length of X_LENS, columns drawn with replacement (unsorted, repeats).  Y: a row of every length of
    Y_LENS, ascending.  P: a row of every length of P_LENS, and short rows besides, so that every X row and every Y row is
    sampled; the rows of more than 65 entries point (almost only) at X rows of at most 17 entries.
    -> (p, x, y, np_cols, the twin's values), built once per mode"""
    if by_col in _cache:
        return _cache[by_col]
    rng = np.random.default_rng([3, int(by_col)])
    x_rows = [rng.integers(0, WIDTH, n) for n in X_LENS]
    y_rows = [np.sort(rng.choice(WIDTH, n, replace=False)) for n in Y_LENS]
    nx, ny = len(X_LENS), len(Y_LENS)
    short_x = [i for i, n in enumerate(X_LENS) if n <= 17]
    if not by_col:
        # P row i uses X's row i: the long P rows are rows of their own with short X rows; X has as many rows as P
        p_rows = [np.arange(ny) for _ in range(nx)]                             # every (X row, Y row) pair
        for n, xl in zip(P_LENS, (5, 0, 16, 17, 1, 15, 16)):
            p_rows.append(rng.integers(0, ny, n))
            x_rows.append(rng.integers(0, WIDTH, xl))
        np_cols = ny
    else:
        # P row i uses Y's row i and its columns choose the X rows: the long rows choose short X rows, one entry in 97 any
        p_rows = [np.arange(nx) for _ in range(ny)]
        for n in P_LENS:
            cols = rng.choice(short_x, n)
            any_row = np.arange(n) % 97 == 50
            cols[any_row] = rng.integers(0, nx, int(any_row.sum()))
            p_rows.append(cols)
            y_rows.append(np.sort(rng.choice(WIDTH, 700, replace=False)))
        np_cols = nx
    (xrp, xci), (yrp, yci), (prp, pci) = csr_of(x_rows), csr_of(y_rows), csr_of(p_rows)
    x, y, p = (xrp, xci, values(rng, len(xci))), (yrp, yci, values(rng, len(yci))), (prp, pci)
    assert sorted(set(np.diff(prp))) == sorted(set(P_LENS) | {len(p_rows[0])})
    want = twin(p, x, y, np_cols, WIDTH, by_col)
    _cache[by_col] = (p, x, y, np_cols, want)
    return _cache[by_col]


@pytest.mark.parametrize("by_col", [False, True])
def test_every_row_length_against_the_twin(by_col):
    p, x, y, np_cols, want = main_case(by_col)
    got, intact = raw(p, x, y, np_cols, WIDTH, by_col)
    print("entries of P", len(p[1]), "non-zero values", int(np.count_nonzero(want)))
    assert intact and same_values(got, want) and np.count_nonzero(want) > 1000
    again, _ = raw(p, x, y, np_cols, WIDTH, by_col)                             # the same bits at every call
    assert np.array_equal(bits(again), bits(got))


@pytest.mark.parametrize("by_col", [False, True])
def test_operands_at_four_byte_alignment_and_a_side_stream(by_col):
    p, x, y, np_cols, want = main_case(by_col)
    got, intact = raw(p, x, y, np_cols, WIDTH, by_col, offsets=(1, 3, 2, 1, 3, 3, 2, 1, 1))
    assert intact and same_values(got, want)
    side = torch.cuda.Stream()
    got, intact = raw(p, x, y, np_cols, WIDTH, by_col, offsets=(3, 1, 1, 2, 1, 2, 3, 3, 2), stream=side)
    assert intact and same_values(got, want)


@pytest.mark.parametrize("by_col", [False, True])
def test_patterns_count_common_columns(by_col):
    p, x, y, np_cols, _ = main_case(by_col)
    for xv, yv in ((None, None), (x[2], None), (None, y[2])):
        got = check(p, (x[0], x[1], xv), (y[0], y[1], yv), np_cols, WIDTH, by_col)
    counts = check(p, (x[0], x[1], None), (y[0], y[1], None), np_cols, WIDTH, by_col)
    assert counts.max() == 5000 and np.all(counts == np.round(counts))          # the long X row against the whole width


# ---- hand-made rows ------------------------------------------------------------------------------------------------------------
def _one_entry(x_cols, x_vals, y_cols, y_vals, w, by_col):
    """P = [[0]], one row of X, one of Y -> the value of the entry"""
    x = (np.array([0, len(x_cols)], np.int32), np.asarray(x_cols, np.int32), None if x_vals is None else np.asarray(x_vals, np.float32))
    y = (np.array([0, len(y_cols)], np.int32), np.asarray(y_cols, np.int32), None if y_vals is None else np.asarray(y_vals, np.float32))
    p = (np.array([0, 1], np.int32), np.array([0], np.int32))
    return check(p, x, y, 1, w, by_col)[0]


@pytest.mark.parametrize("by_col", [False, True])
@pytest.mark.parametrize("length, where", [(50, (5, 20, 40)), (64, (0, 15, 63)), (130, (10, 70, 129)), (300, (63, 64, 299)),
                                           (LONG + 5, (3, 1000, LONG + 4))])
def test_the_fold_order_is_xs_entry_order_across_chunks(length, where, by_col):
    """products 2^24, 1, -2^24 at three entries of X on either side of a chunk boundary: (2^24 + 1) - 2^24 = 0 in fp32, and
    any other association gives 1"""
    x_cols = np.random.default_rng(length).permutation(length) * 3             # unsorted, distinct
    x_vals = np.ones(length, np.float32)
    x_vals[list(where)] = [BIG, 1, -BIG]
    y_cols = np.sort(x_cols[list(where)])
    v = _one_entry(x_cols, x_vals, y_cols, np.ones(3, np.float32), 3 * length, by_col)
    assert bits([v])[0] == 0
    x_vals[list(where)] = [1, BIG, -BIG]                                        # 1 + 2^24 rounds to 2^24 as well
    v = _one_entry(x_cols, x_vals, y_cols, np.ones(3, np.float32), 3 * length, by_col)
    assert v == 0
    x_vals[list(where)] = [BIG, -BIG, 1]
    assert _one_entry(x_cols, x_vals, y_cols, np.ones(3, np.float32), 3 * length, by_col) == 1


@pytest.mark.parametrize("by_col", [False, True])
def test_special_values_first_and_last_entries_and_repeats(by_col):
    f = np.float32
    inf, nan = f(np.inf), f(np.nan)
    y_cols, y_vals = [2, 5, 9, 11, 40], [1, 2, 3, 4, 5]
    assert _one_entry([9], [-0.0], y_cols, y_vals, 50, by_col) == 0 and np.signbit(_one_entry([9], [-0.0], y_cols, y_vals, 50, by_col))
    assert bits([_one_entry([3, 4, 10], [1, 1, 1], y_cols, y_vals, 50, by_col)])[0] == 0        # no match: +0.0
    assert bits([_one_entry([], [], y_cols, y_vals, 50, by_col)])[0] == 0                       # an empty X row
    assert bits([_one_entry([2, 5], [1, 1], [], [], 50, by_col)])[0] == 0                       # an empty Y row
    assert _one_entry([2], [7], y_cols, y_vals, 50, by_col) == 7                                # Y's first entry
    assert _one_entry([40], [7], y_cols, y_vals, 50, by_col) == 35                              # Y's last entry
    assert _one_entry([0, 1, 41, 49, 40, 2], [1] * 6, y_cols, y_vals, 50, by_col) == 6          # below the first, above the last
    assert _one_entry([5, 5, 5, 11, 5], [1, 2, 3, 4, 5], y_cols, y_vals, 50, by_col) == 38      # repeated columns are more products
    assert np.isnan(_one_entry([2, 5], [inf, 1], [2, 5], [0, 1], 50, by_col))                   # inf * 0
    assert np.isnan(_one_entry([2, 5], [inf, -inf], [2, 5], [1, 1], 50, by_col))                # inf - inf
    assert _one_entry([2, 5], [inf, 1], [2, 5], [1, 1], 50, by_col) == inf
    assert _one_entry([2, 5], [1, 1], [2, 5], [-inf, 1], 50, by_col) == -inf
    assert np.isnan(_one_entry([2, 5, 9], [1, nan, 1], y_cols, y_vals, 50, by_col))
    # X columns outside [0, w) contribute nothing, even where Y (wrongly) holds them
    assert _one_entry([-1, 50, 2, 77, -5], [9, 9, 1, 9, 9], [-5, -1, 2, 50, 77], [1] * 5, 50, by_col) == 1
    # both values absent: the number of common columns, above 64 too
    assert _one_entry(np.arange(100)[::-1], None, np.arange(0, 200), None, 200, by_col) == 100
    assert _one_entry(np.arange(0, 200, 2), None, np.arange(0, 200, 3), None, 200, by_col) == 34


@pytest.mark.parametrize("by_col", [False, True])
def test_columns_out_of_range_and_unusable_row_pointers(by_col):
    rng = np.random.default_rng(17)
    m, n, w = 6, 6, 40                                   # square, so that one set of operands fits both modes
    x_rows = [rng.integers(0, w, k) for k in (5, 20, 0, 70, 9, 12)]
    y_rows = [np.sort(rng.choice(w, k, replace=False)) for k in (10, 40, 3, 0, 25, 7)]
    p_rows = [[0, 1, 2, 3, 4, 5], [5, -1, 6, 0, 2 ** 30, 3], [], [1, 1, 4], [2], [0, 5, 3, 1]]
    (xrp, xci), (yrp, yci), (prp, pci) = csr_of(x_rows), csr_of(y_rows), csr_of(p_rows)
    x, y, p = (xrp, xci, values(rng, len(xci))), (yrp, yci, values(rng, len(yci))), (prp, pci)
    got = check(p, x, y, n, w, by_col)
    assert np.all(bits(got[[7, 8, 10]]) == 0)            # the P columns -1, 6 and 2^30: +0.0
    for which, at, value in (("x", 1, -3), ("x", 4, len(xci) + 1), ("x", 2, int(xrp[3]) + 1), ("y", 2, -1), ("y", 5, len(yci) + 9),
                             ("y", 1, int(yrp[2]) + 2), ("p", 1, -2), ("p", 6, len(pci) + 1), ("p", 3, len(pci) + 5),
                             ("p", 0, 1)):
        bad = {"x": xrp, "y": yrp, "p": prp}[which].copy()
        bad[at] = value
        xx = (bad, x[1], x[2]) if which == "x" else x
        yy = (bad, y[1], y[2]) if which == "y" else y
        pp = (bad, p[1]) if which == "p" else p
        got = check(pp, xx, yy, n, w, by_col)
        if which == "p":
            assert np.any(bits(got) == SENTINEL[4])      # nothing was written for the rows of that pair
    # a Y row that does not ascend: unspecified values, but every search ends and nothing is accessed out of bounds
    scrambled = (yrp, yci[::-1].copy(), y[2])
    got, intact = raw(p, x, scrambled, n, w, by_col)
    assert intact and got.shape == (len(pci),)
    # no rows / no entries: nothing written, no pointer looked at
    lib = _lib.load()
    args = [None, None, 0, 5, 0, None, None, None, 0, None, None, None, 0, 9, int(by_col), None, None, 0, None]
    assert lib.gcn_csr_sampled_dot_f32(*args) == 0
    args[2] = 4
    assert lib.gcn_csr_sampled_dot_f32(*args) == 0


def test_seeded_sweep_of_small_random_shapes():
    rng = np.random.default_rng(2024)
    for case in range(50):
        by_col = bool(case % 2)
        mp, np_cols, w = (int(v) for v in rng.integers(1, 40, 3))
        xm, ym = (np_cols, mp) if by_col else (mp, np_cols)
        top = int(rng.choice([4, 20, 90]))
        x_rows = [rng.integers(0, w, int(rng.integers(0, top + 1))) for _ in range(xm)]
        y_rows = [np.sort(rng.choice(w, int(rng.integers(0, min(w, top) + 1)), replace=False)) for _ in range(ym)]
        p_rows = [rng.integers(0, np_cols, int(rng.integers(0, top + 1))) for _ in range(mp)]
        (xrp, xci), (yrp, yci), (prp, pci) = csr_of(x_rows), csr_of(y_rows), csr_of(p_rows)
        xv = values(rng, len(xci)) if case % 5 else None
        yv = values(rng, len(yci)) if case % 7 else None
        if len(pci) == 0:
            continue
        check((prp, pci), (xrp, xci, xv), (yrp, yci, yv), np_cols, w, by_col, offsets=rng.integers(0, 4, 9).tolist())
