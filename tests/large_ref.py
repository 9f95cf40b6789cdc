"""Host twin of the sparse-touch tests (tests/test_large_operands_cpu.py proves its cases without a GPU,
tests/test_large_operands_gpu.py runs them): a tiny graph whose row or column count is large enough that the rows it touches
lie beyond the 32-bit thresholds of one big dense operand.  The big operand is never materialised on the host:
``feat(r, j)`` is a pure int64 hash of (row, column) -> an integer in [-8, 8], the same in numpy and in torch and exact in
bf16; the device fills the table from it in row chunks and the twin evaluates it only at the rows the graph touches.  Matrix
values are eighths, so every sum is exact in fp32 in any order and every comparison is bit for bit.

Thresholds of an element index e into a tensor of element size s: B32 (e * s >= 2^32: 32-bit byte offsets, buffer
addressing), E31 (e >= 2^31: a signed int element index), E32 (e >= 2^32: an unsigned element index, the dropout mask's
flat index).  A band is 64 consecutive rows; a big operand of R rows is touched in rows 0..63, in the band straddling the
first row at each threshold it reaches, and in rows R-64..R-1.

Every case can be re-evaluated with its row offsets truncated (``TRUNCATIONS``), on the gather side or on the store side: a
case is good only if every such mutant differs from the truth somewhere the GPU test compares."""
import numpy as np

BAND = 64
LIMIT = {"B32": 1 << 32, "E31": 1 << 31, "E32": 1 << 32}
# the truncations a case aimed at a threshold must refuse (the others leave its offsets as they are)
MUTANTS = {"B32": ("byte_u32",), "E31": ("elem_i32", "byte_u32"), "E32": ("elem_u32", "elem_i32", "byte_u32")}
ITEMSIZE = {"fp32": 4, "bf16": 2, "int32": 4}
_M31 = 0x7FFFFFFF


def feat(r, j, salt=0):
    """integer in [-8, 8] from (row, column): int64 arithmetic that never overflows (rows < 2^30, columns < 2^20), on
    numpy int64 arrays and on torch int64 tensors alike"""
    h = (r * 2654435761 + j * 40503 + (salt * 977 + 12345)) & _M31
    h = ((h ^ (h >> 15)) * 2246822519) & _M31
    h = ((h ^ (h >> 13)) * 3266489917) & _M31
    h = h ^ (h >> 16)
    return h % 17 - 8


def feat_rows(rows, k, salt=0, trunc=None, itemsize=4, numel=None):
    """feat at the rows `rows` -> int64 [len(rows), k]; trunc: the element offset r * k + j goes through that truncation
    first (what a kernel with a narrow offset would read)"""
    rows = np.asarray(rows, np.int64)
    off = rows[:, None] * k + np.arange(k, dtype=np.int64)[None, :]
    if trunc is not None:
        off = truncate(off, trunc, itemsize, numel)
    return feat(off // k, off % k, salt)


def truncate(off, kind, itemsize, numel):
    """element offsets as a 32-bit computation would form them: the element offset mod 2^32, the element offset through
    int32 sign wrap (clamped into the tensor), the byte offset mod 2^32"""
    off = np.asarray(off, np.int64)
    if kind == "elem_u32":
        return off & 0xFFFFFFFF
    if kind == "elem_i32":
        return np.clip(((off + (1 << 31)) & 0xFFFFFFFF) - (1 << 31), 0, numel - 1)
    if kind == "byte_u32":
        return ((off * itemsize) & 0xFFFFFFFF) // itemsize
    raise KeyError(kind)


TRUNCATIONS = ("elem_u32", "elem_i32", "byte_u32")


def rows_for(threshold, k, itemsize):
    """the smallest operand that reaches the threshold in its last band: ceil(limit / (k [* s])) + 64 rows"""
    per_row = k * (itemsize if threshold == "B32" else 1)
    return -(-LIMIT[threshold] // per_row) + BAND


def threshold_rows(R, k, itemsizes):
    """name -> the first row whose offset reaches the threshold, for the thresholds an [R, k] tensor reaches (itemsizes:
    of every tensor of that shape the case holds, e.g. a bf16 result and its int32 arg)"""
    out = {}
    for s in itemsizes:
        for name in ("B32", "E31", "E32"):
            t = -(-LIMIT[name] // (k * (s if name == "B32" else 1)))
            if 0 < t < R:
                out[f"{name}/{s}"] = t
    return out


def bands(R, k, itemsizes):
    """[(name, lo, hi)]: rows 0..63, the band straddling each threshold row, rows R-64..R-1"""
    assert R >= 2 * BAND
    b = [("low", 0, BAND)]
    for name, t in sorted(threshold_rows(R, k, itemsizes).items(), key=lambda kv: kv[1]):
        b.append((name, max(0, t - BAND // 2), min(R, t + BAND // 2)))
    b.append(("top", R - BAND, R))
    return b


def band_rows(R, k, itemsizes):
    """the rows of every band, ascending, each once"""
    return np.unique(np.concatenate([np.arange(lo, hi, dtype=np.int64) for _, lo, hi in bands(R, k, itemsizes)]))


# row lengths inside a band of an output-large case, by row % 32: empty rows, 1 entry, 64 entries, one long row (-1: longer
# than the unit's largest bound), short ones; the first row of a period is empty and the last one is not
_PATTERN = np.array([0, 1, 64, -1, 0, 3, 0, 7, 2, 0, 5, 0, 0, 65, 1, 0, 0, 4, 63, 0, 9, 0, 1, 0, 0, 2, 0, 6, 0, 0, 33, 5], np.int64)


def eighths(rng, count):
    return ((rng.integers(1, 9, count) * rng.choice([-1, 1], count)) / 8).astype(np.float32)


def out_graph(R, k, itemsizes, n, long_len, seed):
    """[R x n] matrix whose only non-empty rows lie in the bands of an [R, k] result -> (rowptr int32 [R + 1], col, val,
    the band rows)"""
    rng = np.random.default_rng(seed)
    rows = band_rows(R, k, itemsizes)
    lens = _PATTERN[rows % 32].copy()
    lens[lens < 0] = long_len
    rp = np.zeros(R + 1, np.int64)
    rp[rows + 1] = lens
    rp = np.cumsum(rp)
    ci = np.concatenate([np.sort(rng.integers(0, n, int(L))) for L in lens]).astype(np.int32)
    return rp.astype(np.int32), ci, eighths(rng, len(ci)), rows


def in_graph(R, k, itemsizes, m, long_len, seed):
    """[m x R] matrix whose columns all lie in the bands of an [R, k] table: every band is pointed at by short rows and by
    one long row (row 7 + 11 b for band b); rows 0, 1 and m - 1 are empty -> (rowptr, col, val, the touched rows)"""
    rng = np.random.default_rng(seed)
    bs = bands(R, k, itemsizes)
    assert m > 7 + 11 * len(bs)
    lens = rng.integers(0, 6, m)
    lens[rng.random(m) < 0.2] = 0
    lens[[0, 1, m - 1]] = 0
    which = rng.integers(0, len(bs), m)
    for b in range(len(bs)):
        lens[7 + 11 * b], which[7 + 11 * b] = long_len, b
    lens[5], which[5] = 64, len(bs) - 1
    cols = []
    for r in range(m):
        _, lo, hi = bs[which[r]]
        c = rng.integers(lo, hi, int(lens[r]))
        if lens[r] >= BAND:                               # a long row reaches every row of its band
            c[:hi - lo] = np.arange(lo, hi)
        cols.append(np.sort(c))
    rp = np.zeros(m + 1, np.int64)
    rp[1:] = np.cumsum(lens)
    ci = np.concatenate(cols).astype(np.int64)
    assert R < 2 ** 31
    return rp.astype(np.int32), ci.astype(np.int32), eighths(rng, len(ci)), np.unique(ci)


def stored(rows, values, k, compare_rows, fill, trunc=None, itemsize=4, numel=None):
    """what the rows `compare_rows` of an [R, k] result hold after `values` [len(rows), k] were stored at rows `rows` of a
    tensor prefilled with `fill`, the store's element offsets going through `trunc`"""
    rows, compare_rows = np.asarray(rows, np.int64), np.asarray(compare_rows, np.int64)
    j = np.arange(k, dtype=np.int64)[None, :]
    land = rows[:, None] * k + j
    if trunc is not None:
        land = truncate(land, trunc, itemsize, numel)
    cmp_off = (compare_rows[:, None] * k + j).reshape(-1)
    res = np.full(len(cmp_off), fill, np.asarray(values).dtype)
    at = np.searchsorted(cmp_off, land.reshape(-1))
    at = np.minimum(at, len(cmp_off) - 1)
    hit = cmp_off[at] == land.reshape(-1)
    res[at[hit]] = np.asarray(values).reshape(-1)[hit]
    return res.reshape(len(compare_rows), k)


def spmm_rows(rp, ci, va, xrows, rows):
    """(A . X)[rows] in fp64, X given by xrows(cols) -> [len(cols), k]"""
    out = []
    for r in rows:
        b, e = int(rp[r]), int(rp[r + 1])
        x = xrows(ci[b:e].astype(np.int64)).astype(np.float64)
        out.append((va[b:e].astype(np.float64)[:, None] * x).sum(0))
    return np.array(out)


def select_rows(rp, ci, xrows, rows, op, k):
    """row-wise max / min and the CSR entry that supplied it (ties: the lowest entry; an empty row: 0 and -1)"""
    out, arg = np.zeros((len(rows), k)), np.full((len(rows), k), -1, np.int64)
    pick, jj = (np.argmax if op == "max" else np.argmin), np.arange(k)
    for i, r in enumerate(rows):
        b, e = int(rp[r]), int(rp[r + 1])
        if e > b:
            slab = xrows(ci[b:e].astype(np.int64))
            a = pick(slab, axis=0)
            out[i], arg[i] = slab[a, jj], b + a
    return out, arg


# ---- the cases ---------------------------------------------------------------------------------------------------------------
# unit: what runs; side: which operand is big ("in": the gathered table, "out": the result); thr: the highest threshold aimed
# at, for the tensor of dtype `dtype`; k: its width; long: the long row's length (SpMM: more than one chunk of CHUNK_NNZ
# entries; aggregate: above its bound of 4096); knobs: (tile_cols, gather_width) of an unsliced SpMM, (0, 0) what the plan picks
# by itself; extra keys are the unit's own.
CHUNK_NNZ = 256
SMALL = 3001                                             # rows of the small side
CASES = {
    "spmm_in_f32_E31":            dict(unit="spmm", side="in", thr="E31", dtype="fp32", k=512, long=600),
    "spmm_in_bf16_E32":           dict(unit="spmm", side="in", thr="E32", dtype="bf16", k=512, long=600),
    # (forced slices narrower than 32 768 columns: the 15-bit group stream on a table past 4 GiB, the BIG slice bases; the
    # stream takes 256 slices at the most, fewer than 2^23 + 64 rows need: the bf16 table stops at E31, where it has 4 GiB)
    "spmm_in_f32_E31_group_big":  dict(unit="spmm", side="in", thr="E31", dtype="fp32", k=512, long=600, slices=129),
    "spmm_in_bf16_E31_group_big": dict(unit="spmm", side="in", thr="E31", dtype="bf16", k=512, long=600, slices=129),
    "spmm_out_f32_E31_vec4":      dict(unit="spmm", side="out", thr="E31", dtype="fp32", k=512, long=600, knobs=(256, 0)),
    "spmm_out_f32_E31_vec2":      dict(unit="spmm", side="out", thr="E31", dtype="fp32", k=512, long=600, knobs=(128, 0)),
    "spmm_out_f32_E31_vec1":      dict(unit="spmm", side="out", thr="E31", dtype="fp32", k=512, long=600, knobs=(0, 0)),
    "spmm_out_f32_E31_quad":      dict(unit="spmm", side="out", thr="E31", dtype="fp32", k=512, long=600, knobs=(64, 4)),
    # (the wide slice reduction takes widths up to 256: these two run at k = 256, so on twice the rows)
    "spmm_out_f32_B32_sliced_k256": dict(unit="spmm", side="out", thr="B32", dtype="fp32", k=256, long=600, slices=2),
    "spmm_out_bf16_E32":          dict(unit="spmm", side="out", thr="E32", dtype="bf16", k=512, long=600),
    "epilogue_out_f32_E31":       dict(unit="spmm", side="out", thr="E31", dtype="fp32", k=512, long=600, epilogue=True),
    "epilogue_out_f32_E31_sliced_k256": dict(unit="spmm", side="out", thr="E31", dtype="fp32", k=256, long=600, epilogue=True, slices=2),
    "epilogue_out_bf16_E32":      dict(unit="spmm", side="out", thr="E32", dtype="bf16", k=512, long=600, epilogue=True),
    # (a bf16 result behind the slice reduction past 4 GiB: at E32 the two fp32 planes would not fit beside it)
    "epilogue_out_bf16_E31_sliced_k256": dict(unit="spmm", side="out", thr="E31", dtype="bf16", k=256, long=600, epilogue=True, slices=2),
    # the value-free group pass on a pre-laid table past 4 GiB: rows of 8192 floats, 6 slices of 21 855 columns (R counts the
    # table's rows, a zero row behind every slice), 50 entries per column with values u_row[r] * u_col[c]
    "prelaid_table_B32":          dict(unit="prelaid", side="in", thr="B32", dtype="fp32", k=8192, slices=6, n=131130, row_len=2170),
    "spmm_backward_E31":          dict(unit="spmm_backward", side="out", thr="E31", dtype="fp32", k=512, long=600),
    "sddmm_A_f32_E31":            dict(unit="sddmm", side="A", thr="E31", dtype="fp32", k=512, long=300),
    "sddmm_B_f32_E31":            dict(unit="sddmm", side="in", thr="E31", dtype="fp32", k=512, long=300),
    "sddmm_B_bf16_E31":           dict(unit="sddmm", side="in", thr="E31", dtype="bf16", k=512, long=300),
    "aggregate_max_in_f32_E31":   dict(unit="aggregate", side="in", thr="E31", dtype="fp32", k=512, long=4100, op="max"),
    "aggregate_min_in_bf16_E32":  dict(unit="aggregate", side="in", thr="E32", dtype="bf16", k=512, long=4100, op="min"),
    "aggregate_max_out_bf16_E32": dict(unit="aggregate", side="out", thr="E32", dtype="bf16", k=512, long=4100, op="max", arg=True),
    "aggregate_min_out_f32_E31":  dict(unit="aggregate", side="out", thr="E31", dtype="fp32", k=512, long=4100, op="min", arg=True),
    "aggregate_backward_E31":     dict(unit="aggregate_backward", side="out", thr="E31", dtype="fp32", k=512, long=4100, op="max"),
    # all heads in one pass (H = 8, F = 64; one case with F = 63, no multiple of 4); GATv2 with slope 1/4 and eighths in att
    "spmm_heads_in_E31":          dict(unit="spmm_heads", side="in", thr="E31", dtype="fp32", k=512, heads=8, long=4100),
    "spmm_heads_in_E31_F63":      dict(unit="spmm_heads", side="in", thr="E31", dtype="fp32", k=504, heads=8, long=4100),
    "spmm_heads_out_E31":         dict(unit="spmm_heads", side="out", thr="E31", dtype="fp32", k=512, heads=8, long=4100),
    "spmm_heads_backward_E31":    dict(unit="spmm_heads_backward", side="out", thr="E31", dtype="fp32", k=512, heads=8, long=4100),
    "sddmm_heads_A_E31":          dict(unit="sddmm_heads", side="A", thr="E31", dtype="fp32", k=512, heads=8, long=1100),
    "sddmm_heads_B_E31":          dict(unit="sddmm_heads", side="in", thr="E31", dtype="fp32", k=512, heads=8, long=1100),
    "gatv2_src_E31":              dict(unit="gatv2", side="in", thr="E31", dtype="fp32", k=512, heads=8, long=1100),
    "gatv2_dst_E31_F63":          dict(unit="gatv2", side="A", thr="E31", dtype="fp32", k=504, heads=8, long=1100),
    "gatv2_grad_src_E31":         dict(unit="gatv2_backward", side="in", thr="E31", dtype="fp32", k=512, heads=8, long=4100),
    "gatv2_grad_dst_E31":         dict(unit="gatv2_backward", side="A", thr="E31", dtype="fp32", k=512, heads=8, long=4100),
    # a_dst / a_src [rows, H] with H = 64 and 2^25 + 64 rows; fp64 reference and the standing bounds of test_heads_gpu.py
    "gat_softmax_dst_E31":        dict(unit="gat_softmax", side="A", thr="E31", dtype="fp32", k=64, heads=64, long=8200),
    "gat_softmax_src_E31":        dict(unit="gat_softmax", side="in", thr="E31", dtype="fp32", k=64, heads=64, long=8200),
    "knn_y_E31":                  dict(unit="knn", side="in", thr="E31", dtype="fp32", k=256, q=64, knn_k=16),
    "gather_rows_src_E31":        dict(unit="gather_rows", side="in", thr="E31", dtype="fp32", k=512),
    "gather_rows_out_E31":        dict(unit="gather_rows", side="out", thr="E31", dtype="fp32", k=512),
    "dropout_rows_f32_E32":       dict(unit="dropout_rows", side="out", thr="E32", dtype="fp32", k=512),
    "dropout_rows_bf16_E32":      dict(unit="dropout_rows", side="out", thr="E32", dtype="bf16", k=512),
}
SLOPE = 0.25
GAT_SLOPE = 0.2                                          # (the softmax cases are compared within bounds: the usual slope)
FAR = 64.0                                               # every coordinate of a row of y that is not planted
DROPOUT = (0.5, 0x1234567, 11)                           # p (scale 2 exactly), seed, offset: util.EPILOGUE_DROPOUT
_BUILT, _TWINS = {}, {}


def itemsizes(c):
    """of every [R, k] tensor the case holds: the big operand, and the int32 arg of an aggregate result"""
    return (ITEMSIZE[c["dtype"]],) + ((4,) if c.get("arg") else ())


def build(name):
    """the case with its shapes and its graph: R rows of the big operand, m x n matrix (rp, ci, va), `touched`: the rows of
    the big operand the graph reaches (in) or the band rows (out).  Kept: the arrays are read, never written"""
    if name in _BUILT:
        return _BUILT[name]
    c = dict(CASES[name], name=name)
    k, s = c["k"], ITEMSIZE[c["dtype"]]
    seed = sorted(CASES).index(name)
    c["salt"] = seed
    R = c["R"] = rows_for(c["thr"], k, s)
    c["numel"] = R * k
    unit, side = c["unit"], c["side"]
    if unit in ("spmm", "aggregate", "sddmm", "spmm_heads", "sddmm_heads", "gatv2", "gatv2_backward", "gat_softmax") and side == "in":
        c["m"], c["n"] = SMALL, R
        c["rp"], c["ci"], c["va"], c["touched"] = in_graph(R, k, itemsizes(c), SMALL, c["long"], seed)
    elif unit in ("spmm", "aggregate", "spmm_heads") or side == "A":
        c["m"], c["n"] = R, SMALL
        c["rp"], c["ci"], c["va"], c["touched"] = out_graph(R, k, itemsizes(c), SMALL, c["long"], seed)
    elif unit in ("spmm_backward", "aggregate_backward", "spmm_heads_backward"):   # the gradient of x [R, k]: the forward's matrix is [m x R]
        c["m"], c["n"] = SMALL, R
        c["rp"], c["ci"], c["va"], c["touched"] = in_graph(R, k, itemsizes(c), SMALL, c["long"], seed)
    elif unit == "gather_rows":
        rng = np.random.default_rng(seed)
        if side == "in":                                  # src [R, k] big, a few thousand indices into its bands
            rows = band_rows(R, k, (s,))
            c["idx"] = rng.permutation(np.concatenate([rows, rows[::3]]))
            c["touched"] = rows
        else:                                             # out [R, k] big: every row of it gathers from a small src
            c["idx"] = rng.integers(0, SMALL, R).astype(np.int64)
            c["touched"] = band_rows(R, k, (s,))
    elif unit == "prelaid":
        _build_prelaid(c)
    elif unit in ("dropout_rows", "knn"):                  # (kNN: the planted rows of y)
        c["touched"] = band_rows(R, k, (s,))
    _BUILT[name] = c
    return c


def _build_prelaid(c):
    """[SMALL x n] row block: every row holds row_len random columns and 8 from each band of the TABLE (table row
    t = col + col // w: slice s at rows [s (w + 1), (s + 1)(w + 1)), the last of them zero), so every result row reads
    rows of the table past 4 GiB; compared: check_rows x check_cols of the result"""
    rng = np.random.default_rng(c["salt"])
    n, S, R, k, m = c["n"], c["slices"], c["R"], c["k"], SMALL
    w = c["w"] = -(-n // S)
    assert S * (w + 1) == R and w <= 32767
    t = band_rows(R, k, (4,))
    t = t[t % (w + 1) != w]                               # (the zero rows are no column's)
    c["touched"], band_cols = t, t - t // (w + 1)
    bs = [b for b in bands(R, k, (4,))]
    per_band = [band_cols[(t >= lo) & (t < hi)] for _, lo, hi in bs]
    cols = np.concatenate([rng.integers(0, n, (m, c["row_len"]))] + [rng.choice(b, (m, 8)) for b in per_band], axis=1)
    cols.sort(axis=1)
    c["m"] = m
    c["rp"] = (np.arange(m + 1, dtype=np.int64) * cols.shape[1]).astype(np.int32)
    c["ci"] = cols.reshape(-1).astype(np.int32)
    pow2 = lambda count: (2.0 ** -rng.integers(0, 4, count)).astype(np.float32)
    c["u_row"], c["u_col"], c["out_scale"] = pow2(m), pow2(n), pow2(m)
    c["va"] = (c["u_row"][np.repeat(np.arange(m), cols.shape[1])] * c["u_col"][c["ci"]]).astype(np.float32)
    c["check_rows"] = np.unique(np.concatenate([np.arange(8), rng.integers(0, m, 32), np.arange(m - 8, m)]))
    c["check_cols"] = np.unique(np.concatenate([np.arange(64), rng.integers(0, k, 128), np.arange(k - 64, k)]))
    c["out_gap"] = 1000


def table_content(c, off):
    """what the pre-laid table holds at flat element offsets: u_col[col] * feat(col, j), 0 in the row behind a slice"""
    w, k = c["w"], c["k"]
    t, j = off // k, off % k
    col = np.minimum(t - t // (w + 1), c["n"] - 1)
    return np.where(t % (w + 1) == w, 0.0, c["u_col"][col].astype(np.float64) * feat(col, j, c["salt"]))


def small_x(c, rows=SMALL):
    """the small dense operand of a case whose result is big: feat on `rows` rows"""
    return feat_rows(np.arange(rows), c["k"], c["salt"] + 1000)


def backward_arg(c):
    """the arg [m, k] the aggregation's backward is handed: that of the forward on x = feat"""
    if "arg_host" not in c:
        c["arg_host"] = select_rows(c["rp"], c["ci"], lambda cols: feat_rows(cols, c["k"], c["salt"]), np.arange(c["m"]), c["op"], c["k"])[1]
    return c["arg_host"]


def heads_vals(c):
    """values [nnz, H] of the heads calls: eighths"""
    return eighths(np.random.default_rng(c["salt"] + 500), len(c["ci"]) * c["heads"]).reshape(-1, c["heads"])


def att_of(c):
    return eighths(np.random.default_rng(c["salt"] + 600), c["k"]).reshape(c["heads"], -1)


def edge_grad(c):
    """the gradient [nnz, H] handed to a score kernel's backward: integers in [-8, 8]"""
    return np.random.default_rng(c["salt"] + 700).integers(-8, 9, (len(c["ci"]), c["heads"])).astype(np.float32)


def heads_rows(rp, idx, perm, vals, xrows, rows, heads, k):
    """spmm_heads on the rows `rows`: sum over a row's entries e of vals[perm[e], h] * x[idx[e], hF + j], in fp64"""
    out = np.zeros((len(rows), k))
    for i, r in enumerate(rows):
        b, e = int(rp[r]), int(rp[r + 1])
        if e > b:
            w = vals[perm[b:e] if perm is not None else slice(b, e)].astype(np.float64)
            out[i] = (w[:, :, None] * xrows(idx[b:e].astype(np.int64)).reshape(e - b, heads, -1)).sum(0).reshape(k)
    return out


def bias_of(c):
    return np.random.default_rng(c["k"] + c["salt"]).integers(-8, 9, c["k"]).astype(np.float32)


def softmax_reference(name, gather=None, p=None):
    """the fp64 twins of tests/heads_ref.py on the case's graph compacted to the rows of the big operand that it touches
    (a softmax is per row, a column sum per column: nothing else of the 2^25 rows takes part) -> dict: rp, col, n of the
    compact graph; s32 the fp32 scores; p; for both gradients the reference and the sum of magnitudes its bound is made of.
    p: the probabilities to differentiate at (the GPU's own, as in test_heads_gpu.py; default: the reference's)"""
    import heads_ref
    c = build(name)
    k, touched = c["k"], c["touched"]
    big = feat_rows(touched, k, c["salt"], gather, 4, c["numel"]) / 2.0
    small = small_x(c) / 2.0
    if c["side"] == "A":                                    # the rows outside the bands are empty
        rp, col, n = np.append(c["rp"][touched], c["rp"][-1]).astype(np.int64), c["ci"].astype(np.int64), SMALL
        a_dst, a_src = big, small
    else:
        rp, col, n = c["rp"].astype(np.int64), np.searchsorted(touched, c["ci"].astype(np.int64)), len(touched)
        a_dst, a_src = small, big
    s32 = heads_ref.gat_scores(rp, col, a_dst, a_src, GAT_SLOPE)
    pref = heads_ref.edge_softmax(rp, s32)
    g = edge_grad(c)
    ds, gd = heads_ref.gat_edge_softmax_backward(rp, col, a_dst, a_src, GAT_SLOPE, pref if p is None else p, g)
    trp, _trow, tperm = heads_ref.transpose_pattern(rp, col, n)
    return dict(rp=rp, col=col, n=n, s32=s32, p=pref, gd=gd, gd_mag=heads_ref.row_sums(rp, np.abs(ds)),
                gs=heads_ref.segment_sum(trp, ds, tperm), gs_mag=heads_ref.segment_sum(trp, np.abs(ds), tperm))


def knn_queries(c):
    return feat_rows(np.arange(c["q"]), c["k"], c["salt"] + 1000).astype(np.float32)


def keep_at(flat, trunc_mask=False):
    """the epilogue's dropout mask at flat element indices (trunc_mask: the index cut to 32 bits, the third mutant)"""
    from util import dropout_keep_at
    flat = np.asarray(flat, np.int64)
    return dropout_keep_at(flat & 0xFFFFFFFF if trunc_mask else flat, *DROPOUT)


def to_dtype(a, dtype):
    """fp64 values rounded to the result's type (round to nearest even), back as fp64"""
    a = np.asarray(a, np.float64)
    if dtype != "bf16":
        return a.astype(np.float32).astype(np.float64)
    import torch
    return torch.from_numpy(a.astype(np.float32)).to(torch.bfloat16).double().numpy()


def twin(name, gather=None, store=None, trunc_mask=False):
    """the values the GPU test compares for a case -> dict of arrays, every one over c["touched"] rows (or nnz entries
    for sddmm).  gather / store: one of TRUNCATIONS applied to the big operand's row offsets on that side; trunc_mask: the
    dropout mask's flat index cut to 32 bits.  An output is modelled as the NaN-filled (arg: -2) tensor the GPU test
    passes in, so a store that lands elsewhere leaves the fill where the value belongs."""
    if gather is None and store is None and not trunc_mask:
        if name not in _TWINS:
            _TWINS[name] = _twin(name)
        return _TWINS[name]
    return _twin(name, gather, store, trunc_mask)


def _twin(name, gather=None, store=None, trunc_mask=False):
    c = build(name)
    k, s, R, numel, unit, side = c["k"], ITEMSIZE[c["dtype"]], c["R"], c["numel"], c["unit"], c["side"]
    big = lambda rows: feat_rows(rows, k, c["salt"], gather, s, numel)
    put = lambda rows, vals, fill=np.nan, size=s: stored(rows, vals, k, c["touched"], fill, store, size, numel)
    if unit == "spmm" and side == "in":
        rows = np.arange(c["m"])
        return dict(out=spmm_rows(c["rp"], c["ci"], c["va"], big, rows))   # (an fp32 result, whatever the table's type)
    if unit == "spmm":
        x, rows = small_x(c), c["touched"]
        z = spmm_rows(c["rp"], c["ci"], c["va"], lambda cols: x[cols], rows)
        if c.get("epilogue"):
            flat = rows[:, None] * k + np.arange(k)[None, :]
            z = np.where(keep_at(flat, trunc_mask), 2.0 * np.maximum(z + bias_of(c)[None, :], 0.0), 0.0)
        return dict(out=put(rows, to_dtype(z, c["dtype"])))
    if unit == "spmm_backward":                             # gx = A^T . g, g [m, k] small
        from stress_units import transpose_host
        trp, trow, tva = transpose_host(c["rp"], c["ci"], c["va"], R)
        g, rows = small_x(c), c["touched"]
        return dict(gx=put(rows, to_dtype(spmm_rows(trp, trow, tva, lambda cols: g[cols], rows), "fp32")))
    if unit == "sddmm":
        rows_of = np.repeat(np.arange(c["m"]), np.diff(c["rp"])).astype(np.int64)
        cols = c["ci"].astype(np.int64)
        A = big(rows_of) if side == "A" else small_x(c)[rows_of]
        B = big(cols) if side == "in" else small_x(c)[cols]
        return dict(out=(A.astype(np.float64) * B).sum(1))
    if unit in ("sddmm_heads", "gatv2", "gatv2_backward"):
        H = c["heads"]
        rows_of = np.repeat(np.arange(c["m"]), np.diff(c["rp"])).astype(np.int64)
        cols = c["ci"].astype(np.int64)
        # (the backward reads the big operand and stores its gradient: the gather side is mutated here, the store side below)
        A = (big(rows_of) if side == "A" else small_x(c)[rows_of]).astype(np.float64).reshape(len(cols), H, -1)
        B = (big(cols) if side == "in" else small_x(c)[cols]).astype(np.float64).reshape(len(cols), H, -1)
        if unit == "sddmm_heads":
            return dict(out=(A * B).sum(2))
        t, att = A + B, att_of(c).astype(np.float64)
        if unit == "gatv2":
            return dict(out=(att[None] * np.where(t > 0, t, SLOPE * t)).sum(2))
        per_entry = (edge_grad(c).astype(np.float64)[:, :, None] * att[None] * np.where(t > 0, 1.0, SLOPE)).reshape(len(cols), k)
        own = rows_of if side == "A" else cols
        grad = np.zeros((len(c["touched"]), k))
        np.add.at(grad, np.searchsorted(c["touched"], own), per_entry)
        return dict(grad=put(c["touched"], grad))
    if unit == "spmm_heads" and side == "in":
        return dict(out=heads_rows(c["rp"], c["ci"], None, heads_vals(c), big, np.arange(c["m"]), c["heads"], k))
    if unit == "spmm_heads":
        x, rows = small_x(c), c["touched"]
        return dict(out=put(rows, heads_rows(c["rp"], c["ci"], None, heads_vals(c), lambda cols: x[cols], rows, c["heads"], k)))
    if unit == "spmm_heads_backward":                       # gx = the same walk over the transposed pattern, values through its permutation
        perm = np.argsort(c["ci"], kind="stable")
        trow = np.repeat(np.arange(c["m"]), np.diff(c["rp"]))[perm]
        trp = np.zeros(R + 1, np.int64)
        trp[1:] = np.cumsum(np.bincount(c["ci"], minlength=R))
        g, rows = small_x(c), c["touched"]
        return dict(gx=put(rows, heads_rows(trp, trow, perm, heads_vals(c), lambda cc: g[cc], rows, c["heads"], k)))
    if unit == "prelaid":                                   # u_row[r] * sum over the row of the table's rows, [* out_scale[r]]
        J, w, raw = c["check_cols"].astype(np.int64), c["w"], []
        for r in c["check_rows"]:
            cs = c["ci"][int(c["rp"][r]):int(c["rp"][r + 1])].astype(np.int64)
            off = (cs + cs // w)[:, None] * k + J[None, :]
            if gather is not None:
                off = truncate(off, gather, s, numel)
            raw.append(float(c["u_row"][r]) * table_content(c, off).sum(0))
        raw = np.array(raw)
        return dict(raw=raw, prelaid=raw * c["out_scale"][c["check_rows"]].astype(np.float64)[:, None])
    if unit == "gat_softmax":                               # (the gradient of the big operand is as big: stored)
        ref = softmax_reference(name, gather)
        key = "gd" if side == "A" else "gs"
        return {"p": ref["p"], "gd": ref["gd"], "gs": ref["gs"], key: put(c["touched"], ref[key])}
    if unit == "knn":                                       # y: feat on the planted rows, FAR everywhere else
        from knn_ref import knn_ref
        planted = c["touched"]
        off = planted[:, None] * k + np.arange(k, dtype=np.int64)[None, :]
        if gather is not None:
            off = truncate(off, gather, s, numel)
        at = np.minimum(np.searchsorted(planted, off // k), len(planted) - 1)
        y = np.where(planted[at] == off // k, feat(off // k, off % k, c["salt"]), FAR).astype(np.float32)
        x = knn_queries(c)
        idx, dist2, _ = knn_ref(x, y, c["knn_k"])
        far = ((x.astype(np.float64) - FAR) ** 2).sum(1)
        if gather is None:
            assert np.all(dist2.max(1) < far) and np.all(idx >= 0)   # every row that is not planted is farther than the k-th neighbour
        return dict(idx=planted[idx], dist2=dist2.astype(np.float64))
    if unit == "aggregate" and side == "in":
        out, arg = select_rows(c["rp"], c["ci"], big, np.arange(c["m"]), c["op"], k)
        return dict(out=out, arg=arg)
    if unit == "aggregate":
        x, rows = small_x(c), c["touched"]
        out, arg = select_rows(c["rp"], c["ci"], lambda cols: x[cols], rows, c["op"], k)
        return dict(out=put(rows, out), arg=put(rows, arg, fill=-2, size=4))
    if unit == "aggregate_backward":                        # gx[col[arg[r, j]], j] += g[r, j]
        arg = backward_arg(c)
        g, gx = small_x(c), np.zeros((len(c["touched"]), k))
        for r in range(c["m"]):
            if arg[r, 0] >= 0:
                np.add.at(gx, (np.searchsorted(c["touched"], c["ci"][arg[r]]), np.arange(k)), g[r])
        return dict(gx=put(c["touched"], gx))
    if unit == "gather_rows" and side == "in":
        return dict(out=big(c["idx"]).astype(np.float64))
    if unit == "gather_rows":
        rows = c["touched"]
        return dict(out=put(rows, small_x(c)[c["idx"][rows]].astype(np.float64)))
    if unit == "dropout_rows":                              # in place on feat: the element's own value, doubled or dropped
        rows = c["touched"]
        flat = rows[:, None] * k + np.arange(k)[None, :]
        z = np.where(keep_at(flat, trunc_mask), 2.0 * feat_rows(rows, k, c["salt"]), 0.0)
        return dict(out=put(rows, z))
    raise KeyError(unit)


def mutants(name):
    """[(label, twin keyword arguments)] of every mutant the case must refuse"""
    c = build(name)
    gather_side = c["side"] in ("in", "A") and c["unit"] not in ("spmm_backward", "aggregate_backward", "spmm_heads_backward")
    if c["unit"] in ("gatv2_backward", "gat_softmax"):                      # its big operand is read and its gradient, as big, is stored
        return [(f"{side}:{t}", {side: t}) for side in ("gather", "store") for t in MUTANTS[c["thr"]]]
    out = [(f"{'gather' if gather_side else 'store'}:{t}", {("gather" if gather_side else "store"): t}) for t in MUTANTS[c["thr"]]]
    if c.get("epilogue") or c["unit"] == "dropout_rows":
        if c["thr"] == "E32":
            out.append(("mask:u32", dict(trunc_mask=True)))
    return out


def differs(a, b):
    """two twins differ somewhere (NaN equals NaN: the fill)"""
    return any(not np.array_equal(a[key], b[key], equal_nan=True) for key in a)
