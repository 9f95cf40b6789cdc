"""numpy twins of gcn_amd.edge_aggregate (gcn_amd/csrc/edge_message.hip) and its gradients.

The message is formed in np.float32 with ONE operation, so it has the kernel's bits: t = x[col[e]] + w[e] or x[col[e]] * w[e],
then relu(t) = t < 0 ? +0 : t (NaN and -0.0 pass).  Sums are taken in fp64 over those messages (any order: callers compare
bit for bit only where every sum is exact in fp32, and against a bound elsewhere).  max / min follow numpy's argmax / argmin
with the NaN rule: the first entry in CSR order among equals, -0.0 equals +0.0, a NaN beats every number and the first NaN
wins.  The derivative of relu is D = t <= 0 ? 0 : 1 (a NaN t passes the gradient) and selects: a zero D gives a zero.
The gradients' products (g * w, g * x) are np.float32 products too, rounded once like the kernels'."""
import numpy as np

F32 = np.float32


def entry_rows(rowptr):
    rowptr = np.asarray(rowptr, np.int64)
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def pre_act(x_rows, w, op):
    """t of the message for gathered node rows x_rows and entry rows w, both float32: one float32 operation"""
    x_rows, w = np.asarray(x_rows, F32), np.asarray(w, F32)
    with np.errstate(all="ignore"):
        return (x_rows * w if op == "mul" else x_rows + w).astype(F32)


def activate(t, act):
    return np.where(t < 0, F32(0), t).astype(F32) if act == "relu" else t


def passes(t, act):
    """D as a mask"""
    return ~(t <= 0) if act == "relu" else np.ones(t.shape, bool)


def messages(col, x, w, op, act):
    return activate(pre_act(np.asarray(x, F32)[np.asarray(col, np.int64)], w, op), act)


def segment_sum(rowptr, terms):
    """fp64 [m, k]: the sums of terms [nnz, k] over the entries of every row (an empty row: 0)"""
    rowptr = np.asarray(rowptr, np.int64)
    m = len(rowptr) - 1
    out = np.zeros((m, terms.shape[1]), np.float64)
    live = np.flatnonzero(np.diff(rowptr) > 0)
    if len(live):
        with np.errstate(all="ignore"):
            out[live] = np.add.reduceat(terms.astype(np.float64), rowptr[live], axis=0)
    return out


def select(rowptr, msg, reduce):
    """(out float32 [m, k] with the winner's bits, arg int64 [m, k]): an empty row gives 0 / -1"""
    rowptr = np.asarray(rowptr, np.int64)
    m, k = len(rowptr) - 1, msg.shape[1]
    out, arg = np.zeros((m, k), F32), np.full((m, k), -1, np.int64)
    live = np.flatnonzero(np.diff(rowptr) > 0)
    if not len(live):
        return out, arg
    big = np.finfo(np.float64).max                        # real infinities rank below a NaN, above every fp32 number
    sign = 1.0 if reduce == "max" else -1.0
    score = sign * msg.astype(np.float64)
    score = np.where(np.isnan(msg), np.inf, np.where(np.isinf(score), np.sign(score) * big, score))
    best = np.maximum.reduceat(score, rowptr[live], axis=0)
    row_of = np.repeat(np.arange(len(live)), np.diff(rowptr)[live])
    ent = np.arange(len(msg), dtype=np.int64)[:, None]
    first = np.minimum.reduceat(np.where(score == best[row_of], ent, np.iinfo(np.int64).max), rowptr[live], axis=0)
    arg[live] = first
    out[live] = msg[first, np.arange(k)[None, :]]
    return out, arg


def forward(rowptr, col, x, w, op="add", act=None, reduce="sum"):
    """sum / mean: (fp64 [m, k], sum of |messages| fp64 [m, k]); max / min: (float32 [m, k], arg int64 [m, k])"""
    msg = messages(col, x, w, op, act)
    if reduce in ("max", "min"):
        return select(rowptr, msg, reduce)
    s, mag = segment_sum(rowptr, msg), segment_sum(rowptr, np.abs(msg))
    if reduce == "mean":
        cnt = np.maximum(np.diff(np.asarray(rowptr, np.int64)), 1)[:, None].astype(np.float64)
        return s / cnt, mag / cnt
    return s, mag


def transpose_pattern(rowptr, col, n):
    """(trowptr [n + 1], trow [nnz], tperm [nnz]): a stable bucketing of the entries by column"""
    col = np.asarray(col, np.int64)
    tperm = np.argsort(col, kind="stable")
    trowptr = np.zeros(n + 1, np.int64)
    trowptr[1:] = np.cumsum(np.bincount(col, minlength=n))
    return trowptr, entry_rows(rowptr)[tperm], tperm


def backward_sum(rowptr, col, n, x, w, g, op, act):
    """(gx fp64 [n, k], |gx| terms fp64 [n, k], ge float32 [nnz, k]) of out = sum of messages, for the gradient g [m, k]"""
    col = np.asarray(col, np.int64)
    x, w, g = np.asarray(x, F32), np.asarray(w, F32), np.asarray(g, F32)
    rows = entry_rows(rowptr)
    xs, gs = x[col], g[rows]
    d = passes(pre_act(xs, w, op), act)
    with np.errstate(all="ignore"):
        tx = np.where(d, (gs * w).astype(F32) if op == "mul" else gs, F32(0))
        ge = np.where(d, (gs * xs).astype(F32) if op == "mul" else gs, F32(0)).astype(F32)
    trowptr, _trow, tperm = transpose_pattern(rowptr, col, n)
    return segment_sum(trowptr, tx[tperm]), segment_sum(trowptr, np.abs(tx[tperm])), ge


def backward_select(rowptr, col, n, x, w, g, arg, op, act):
    """(gx fp64 [n, k], |gx| terms, ge float32 [nnz, k]): the gradient goes to the entry arg[r, j] alone"""
    col = np.asarray(col, np.int64)
    x, w, g = np.asarray(x, F32), np.asarray(w, F32), np.asarray(g, F32)
    k = x.shape[1]
    r, j = np.nonzero(arg >= 0)
    e = arg[r, j]
    c = col[e]
    xa, wa, gg = x[c, j], w[e, j], g[r, j]
    d = passes(pre_act(xa, wa, op), act)
    with np.errstate(all="ignore"):
        tx = np.where(d, (gg * wa).astype(F32) if op == "mul" else gg, F32(0))
        te = np.where(d, (gg * xa).astype(F32) if op == "mul" else gg, F32(0)).astype(F32)
    gx, mag = np.zeros((n, k), np.float64), np.zeros((n, k), np.float64)
    with np.errstate(all="ignore"):
        np.add.at(gx, (c, j), tx.astype(np.float64))
        np.add.at(mag, (c, j), np.abs(tx).astype(np.float64))
    ge = np.zeros((len(col), k), F32)
    ge[e, j] = te
    return gx, mag, ge
