"""The one large problem of tests/test_edge_aggregate_large_gpu.py and its twin on the rows, columns and entries that are
compared: a graph of about 4.2 M entries (nnz > 2^22) at k = 512, so that edge_feat [nnz, k] and its gradient pass 2^31
elements (entry 2^22) and 4 GiB (entry 2^21).  Everything is a formula of small integers, evaluated here in numpy at the
places that are compared and on the device (torch) everywhere; the values are on the exact grid of
tests/test_edge_aggregate_gpu.py, so every comparison is bit for bit.

``trunc`` models a kernel that computes an offset into edge_feat or its gradient in 32 bits: "byte32" (the byte offset
modulo 2^32) or "elem31" (the element index modulo 2^31); tests/test_edge_aggregate_cpu.py proves that either changes what
the large test compares."""
import numpy as np

import edge_aggregate_ref as ref

K = 512
N = 4099                                                 # columns (a prime): x stays small
ROWS = 525_000                                           # rows of 6 .. 10 entries: 4.2 M entries, past 2^22
LAST = 10_000                                            # ... and one long row at the end (chunk partials; a long store loop)
E32 = 1 << 21                                            # the entry whose row of edge_feat starts at byte 2^32
E31 = 1 << 22                                            # ... at element 2^31
BAND = 24                                                # rows on either side of a threshold that are compared


def rowptr():
    lens = 6 + np.arange(ROWS, dtype=np.int64) % 5
    rp = np.zeros(ROWS + 2, np.int64)
    rp[1:ROWS + 1] = np.cumsum(lens)
    rp[ROWS + 1] = rp[ROWS] + LAST
    return rp


def col_of(e):
    """the column of entry e (numpy int64 or a torch int64 tensor)"""
    return ((e * 2654435761) % (1 << 32) >> 8) % N


def x_of(c, j):
    return ((c * 5 + j * 11) % 7 - 3)


def w_of(e, j):
    return ((e * 7 + j * 3 + (e >> 9)) % 17 - 8) / 8.0


def g_of(r, j):
    return ((r * 3 + j * 5) % 7 - 3)


def trunc_entry_col(e, j, trunc):
    """where a kernel that truncates the offset of element (e, j) of an [nnz, K] array lands: (entry, column)"""
    o = np.asarray(e, np.int64) * K + j
    if trunc == "byte32":
        o = (o * 4 % (1 << 32)) // 4
    elif trunc == "elem31":
        o = o % (1 << 31)
    elif trunc is not None:
        raise KeyError(trunc)
    return o // K, o % K


def w_rows(entries, trunc=None):
    """float32 [len(entries), K]: the rows of edge_feat a kernel reads for these entries"""
    e, j = trunc_entry_col(np.asarray(entries, np.int64)[:, None], np.arange(K, dtype=np.int64)[None, :], trunc)
    return w_of(e, j).astype(np.float32)


def x_table():
    return x_of(np.arange(N, dtype=np.int64)[:, None], np.arange(K, dtype=np.int64)[None, :]).astype(np.float32)


def compared_rows(rp, seed=0):
    """sorted row numbers: bands around the rows that hold entries 2^21 and 2^22, the first and last 64 rows, 256 random"""
    m = len(rp) - 1
    rows = set(range(64)) | set(range(m - 64, m))
    for e in (E32, E31):
        r = int(np.searchsorted(rp, e, side="right")) - 1
        rows |= set(range(r - BAND, r + BAND + 1))
    rows |= set(np.random.default_rng(seed).integers(0, m, 256).tolist())
    return np.array(sorted(rows), np.int64)


def compared_entries(rp):
    """sorted entry numbers whose rows of the gradient in edge_feat are compared"""
    nnz = int(rp[-1])
    ent = set(range(64)) | set(range(nnz - 64, nnz))
    for e in (E32, E31):
        ent |= set(range(e - 64, e + 64))
    ent |= set(np.random.default_rng(1).integers(0, nnz, 256).tolist())
    return np.array(sorted(ent), np.int64)


def compared_cols(rp):
    """sorted columns whose rows of the gradient in x are compared: those of a few entries around both thresholds, of the
    last entries and of some entries past 2^22, and the first and last column (every column has about a thousand entries)"""
    ent = np.concatenate([np.arange(E32 - 2, E32 + 2), np.arange(E31 - 2, E31 + 2), np.arange(int(rp[-1]) - 2, int(rp[-1])),
                          E31 + 1000 * np.arange(1, 9)])
    return np.unique(np.concatenate([col_of(ent), np.array([0, N - 1])]))


def sub_csr(rp, rows):
    """(local rowptr, the global entry numbers) of the rows `rows`"""
    lens = rp[rows + 1] - rp[rows]
    lrp = np.zeros(len(rows) + 1, np.int64)
    lrp[1:] = np.cumsum(lens)
    ent = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in rows]) if len(rows) else np.zeros(0, np.int64)
    return lrp, ent


def forward_rows(rp, rows, op, act, reduce, trunc=None):
    """the twin's forward on the rows `rows`: sum -> fp64 [len(rows), K]; max / min -> (float32 values, global arg int64)"""
    lrp, ent = sub_csr(rp, rows)
    res = ref.forward(lrp, col_of(ent), x_table(), w_rows(ent, trunc), op, act, reduce)
    if reduce in ("max", "min"):
        out, arg = res
        return out, np.where(arg >= 0, ent[np.maximum(arg, 0)], -1)
    return res[0]


def grad_x_cols(rp, cols, op, act, trunc=None):
    """fp64 [len(cols), K]: the rows `cols` of the gradient in x of the sum, for g = g_of"""
    nnz = int(rp[-1])
    col = col_of(np.arange(nnz, dtype=np.int64))
    out = np.zeros((len(cols), K), np.float64)
    x, j = x_table(), np.arange(K, dtype=np.int64)[None, :]
    for i, c in enumerate(cols):
        ent = np.flatnonzero(col == c)
        rows = np.searchsorted(rp, ent, side="right") - 1
        w = w_rows(ent, trunc)
        g = g_of(rows[:, None], j).astype(np.float32)
        d = ref.passes(ref.pre_act(x[c][None, :], w, op), act)
        term = np.where(d, (g * w).astype(np.float32) if op == "mul" else g, np.float32(0))
        out[i] = term.astype(np.float64).sum(0)
    return out


def grad_e_rows(rp, entries, op, act):
    """float32 [len(entries), K]: the rows `entries` of the gradient in edge_feat of the sum, for g = g_of"""
    entries = np.asarray(entries, np.int64)
    rows = np.searchsorted(rp, entries, side="right") - 1
    j = np.arange(K, dtype=np.int64)[None, :]
    xs = x_table()[col_of(entries)]
    g = g_of(rows[:, None], j).astype(np.float32)
    d = ref.passes(ref.pre_act(xs, w_rows(entries), op), act)
    return np.where(d, (g * xs).astype(np.float32) if op == "mul" else g, np.float32(0)).astype(np.float32)
