"""numpy twin of the link-prediction contracts: the lookup and the rejection sampler of include/gcn_spmm.h
(gcn_csr_find_entries, gcn_negative_sample_csr), the assignment rule of gcn_amd.split_edges, gcn_amd.edge_subgraph and one
batch of gcn_amd.LinkNeighborLoader — what the device results are compared with, integer for integer.  The Philox words come
from subgraph_ref.walk_keys (the random walk's word and counter convention) and util.dropout_keep (the dropout mask's)."""
import numpy as np

from sampling_ref import sample_blocks_ref
from subgraph_ref import walk_keys
from util import dropout_keep, random_rows_csr

TRAIN, VAL, TEST = 0, 1, 2


def _usable(rowptr, nnz, r):
    if r < 0 or r >= len(rowptr) - 1:
        return None
    b, e = int(rowptr[r]), int(rowptr[r + 1])
    return (b, e) if 0 <= b <= e <= nnz else None


def row_find(col, b, e, q):
    """the contract's row search: the lower bound of q over col[b:e], probe for probe → lowest entry index holding q, or -1"""
    lo, hi = b, e
    while lo < hi:
        mid = lo + ((hi - lo) >> 1)
        if col[mid] < q:
            lo = mid + 1
        else:
            hi = mid
    return lo if lo < e and col[lo] == q else -1


def find_entries_ref(rowptr, col, q_rows, q_cols):
    """→ int32 [len(q_rows)] of gcn_csr_find_entries"""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    out = np.full(len(q_rows), -1, np.int64)
    for i, (r, c) in enumerate(zip(np.asarray(q_rows, np.int64), np.asarray(q_cols, np.int64))):
        be = _usable(rowptr, len(col), int(r))
        if be is not None:
            out[i] = row_find(col, be[0], be[1], int(c))
    return out.astype(np.int32)


def find_entries_brute(rowptr, col, q_rows, q_cols):
    """the same answers from a dictionary of the stored pairs (first occurrence = lowest entry index): no search"""
    rowptr = np.asarray(rowptr, np.int64)
    first = {}
    for r in range(len(rowptr) - 1):
        for e in range(int(rowptr[r]), int(rowptr[r + 1])):
            first.setdefault((r, int(col[e])), e)
    return np.array([first.get((int(r), int(c)), -1) for r, c in zip(q_rows, q_cols)], np.int32)


def negative_sample_ref(rowptr, col, n, q_rows, num_neg=1, seed=0, offset=0, max_tries=32, exclude_self=True):
    """→ int32 [len(q_rows), num_neg] of gcn_negative_sample_csr: slot p = i * num_neg + s is walk index p of
    walk_keys(slots, max_tries): key[p, t] = word (j & 3) of Philox4x32-10(counter (j >> 2, offset), key seed), j = p * T4 + t"""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    q_rows = np.asarray(q_rows, np.int64)
    slots = len(q_rows) * num_neg
    cand = ((walk_keys(slots, max_tries, seed, offset) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)   # [slot, try]
    out = np.full(slots, -1, np.int64)
    stored = {}
    for p in range(slots):
        r = int(q_rows[p // num_neg])
        if r not in stored:
            be = _usable(rowptr, len(col), r)
            stored[r] = None if be is None else set(col[be[0]:be[1]].tolist())
        if stored[r] is None:
            continue
        for c in cand[p].tolist():
            if (exclude_self and c == r) or c in stored[r]:
                continue
            out[p] = c
            break
    return out.reshape(len(q_rows), num_neg).astype(np.int32)


def edge_subgraph_ref(rowptr, col, val, keep):
    """→ (rowptr, col, val, eid) of the kept entries in entry order"""
    keep = np.asarray(keep, bool)
    prefix = np.concatenate([[0], np.cumsum(keep)])
    eid = np.nonzero(keep)[0]
    return prefix[np.asarray(rowptr, np.int64)].astype(np.int32), np.asarray(col)[eid], np.asarray(val)[eid], eid.astype(np.int32)


def split_parts_ref(rowptr, col, val_frac, test_frac, seed=0, undirected=True):
    """→ uint8 [nnz], TRAIN / VAL / TEST per entry: the dropout mask's word of element e (seed, offset 0) below
    float32(val_frac) * 2^32 is VAL, else below float32(val_frac + test_frac) * 2^32 is TEST, else TRAIN; undirected: the
    diagonal is TRAIN and an entry (r, c) with r > c takes the part of the lowest entry (c, r)"""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    nnz = len(col)
    below = lambda p: ~dropout_keep(nnz, p, seed, 0) if p > 0 else np.zeros(nnz, bool)
    part = np.where(below(val_frac), VAL, np.where(below(val_frac + test_frac), TEST, TRAIN)).astype(np.uint8)
    if undirected:
        rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
        part[rows == col] = TRAIN
        rev = find_entries_brute(rowptr, col, col, rows)
        assert (rev[rows != col] >= 0).all(), "an entry without a reverse"
        lower = rows > col
        part[lower] = part[rev[lower]]
    return part


def link_batch_ref(rowptr, col, val, eids, fanouts, num_neg, seed, offset, max_tries=32):
    """one batch of LinkNeighborLoader over the entries ``eids`` at Philox offset ``offset`` → (blocks, input_ids, pair_rows,
    pair_cols, labels, nodes, negatives): blocks as sampling_ref.sample_blocks_ref gives them, the pairs as positions in
    nodes, negatives the raw [len(eids), num_neg] draw (-1 slots included)"""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    eids = np.asarray(eids, np.int64)
    rows = np.searchsorted(rowptr, eids, side="right") - 1
    neg = negative_sample_ref(rowptr, col, len(rowptr) - 1, rows, num_neg, seed, offset, max_tries, True)
    flat = neg.reshape(-1).astype(np.int64)
    drawn = flat >= 0
    u = np.concatenate([rows, np.repeat(rows, num_neg)[drawn]])
    v = np.concatenate([col[eids], flat[drawn]])
    nodes = np.unique(np.concatenate([u, v]))
    labels = np.zeros(len(u), np.float32)
    labels[:len(eids)] = 1.0
    blocks, input_ids = sample_blocks_ref(rowptr, col, val, nodes, fanouts, seed, offset + 1)
    return blocks, input_ids, np.searchsorted(nodes, u), np.searchsorted(nodes, v), labels, nodes, neg


# ---- the fixture of the device tests (and of the twin's own check against brute force) -----------------------------------------
LENS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 5000]


def lookup_fixture(m=6000, n=6000, seed=5):
    """→ (rowptr, col, full_row, almost_row, missing): column-sorted rows of the lengths LENS (capped at n) with columns
    drawn with replacement — so some repeat — whose first and last column are stored twice from length 4 on, then a full
    row (all n columns), a row storing every column but ``missing``, and empty rows up to m"""
    lens = [min(d, n) for d in LENS]
    rp, ci = random_rows_csr(len(lens), n, lens, seed)
    rows = []
    for r, d in enumerate(lens):
        c = ci[rp[r]:rp[r + 1]].astype(np.int64)
        if d >= 4:                                         # repeats at the first and at the last position
            c[1], c[-2] = c[0], c[-1]
        rows.append(np.sort(c))
    full_row, almost_row, missing = len(lens), len(lens) + 1, n // 3
    rows.append(np.arange(n))
    rows.append(np.delete(np.arange(n), missing))
    rows += [np.zeros(0, np.int64)] * (m - len(rows))
    rowptr = np.zeros(m + 1, np.int64)
    rowptr[1:] = np.cumsum([len(c) for c in rows])
    return rowptr.astype(np.int32), np.concatenate(rows).astype(np.int32), full_row, almost_row, missing


def lookup_queries(rowptr, col, n):
    """the queries of the lookup test: every stored entry; for every row the column just below its first and just above its
    last (for an empty row: 0 and n - 1); columns -1 and n; rows -1 and m → (q_rows, q_cols) int64"""
    rowptr = np.asarray(rowptr, np.int64)
    m = len(rowptr) - 1
    rows = np.repeat(np.arange(m), np.diff(rowptr))
    nonempty = np.nonzero(np.diff(rowptr) > 0)[0]
    empty = np.nonzero(np.diff(rowptr) == 0)[0]
    q_rows = [rows, nonempty, nonempty, empty, empty, np.arange(m), np.arange(m), [-1, -1, m, m]]
    q_cols = [col, col[rowptr[nonempty]].astype(np.int64) - 1, col[rowptr[nonempty + 1] - 1].astype(np.int64) + 1,
              np.zeros(len(empty)), np.full(len(empty), n - 1), np.full(m, -1), np.full(m, n), [0, n - 1, 0, n - 1]]
    return np.concatenate(q_rows).astype(np.int64), np.concatenate(q_cols).astype(np.int64)
