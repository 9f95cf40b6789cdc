"""numpy twin of the sampling contract of include/gcn_spmm.h (gcn_sample_neighbors_csr) and of gcn_amd.sample_blocks'
relabelling: what the device results are compared with, integer for integer.  Keys come from util.philox4x32_10."""
import numpy as np

from util import philox4x32_10

TIE_SEARCH = 1 << 22                                   # entry indices searched for equal keys (seed 1, offset 0)


def entry_keys(entries, seed, offset):
    """key(e) = word e & 3 of Philox4x32-10(counter = (lo32(e >> 2), hi32(e >> 2), lo32(offset), hi32(offset)),
    key = (lo32(seed), hi32(seed))) for an array of entry indices → uint64 array of 32-bit keys"""
    e = np.asarray(entries, dtype=np.uint64)
    seed, offset = int(seed), int(offset)
    j = e >> np.uint64(2)
    groups, inverse = np.unique(j, return_inverse=True)
    words = philox4x32_10((groups & np.uint64(0xFFFFFFFF), groups >> np.uint64(32), offset & 0xFFFFFFFF, offset >> 32),
                          (seed & 0xFFFFFFFF, seed >> 32))
    table = np.stack(words, axis=1)                    # [group, word]
    return table[inverse.reshape(-1), (e & np.uint64(3)).astype(np.int64).reshape(-1)].reshape(e.shape)


def sample_row(b, e, fanout, seed, offset):
    """the selected entry indices of the row [b, e), ascending"""
    d = e - b
    idx = np.arange(b, e, dtype=np.int64)
    if fanout < 0 or d <= fanout:
        return idx
    keys = entry_keys(idx, seed, offset)
    order = np.lexsort((idx, keys))                    # by (key, entry index)
    return np.sort(idx[order[:fanout]])


def sample_neighbors_ref(rowptr, col, seeds, fanout, seed=0, offset=0):
    """→ (rowptr [len(seeds) + 1], col, eid), int32, of the contract"""
    rowptr = np.asarray(rowptr, np.int64)
    picks = [sample_row(int(rowptr[v]), int(rowptr[v + 1]), fanout, seed, offset) for v in np.asarray(seeds, np.int64)]
    out_rowptr = np.zeros(len(picks) + 1, np.int64)
    out_rowptr[1:] = np.cumsum([len(p) for p in picks])
    eid = np.concatenate(picks) if picks else np.zeros(0, np.int64)
    eid = eid.astype(np.int64)
    return out_rowptr.astype(np.int32), np.asarray(col)[eid].astype(np.int32), eid.astype(np.int32)


def relabel_ref(dst, cols):
    """src = dst ++ (the distinct values of cols that are not in dst, ascending); → (src, positions of cols in src)"""
    dst = np.asarray(dst, np.int64)
    cols = np.asarray(cols, np.int64)
    new = np.setdiff1d(cols, dst)                      # sorted and distinct
    src = np.concatenate([dst, new])
    where = {int(v): i for i, v in enumerate(src)}
    return src, np.array([where[int(c)] for c in cols], np.int64)


def sample_blocks_ref(rowptr, col, val, seeds, fanouts, seed=0, offset=0):
    """→ (blocks, input_ids): blocks outermost hop first, each a dict with rowptr / col (positions in src_ids) / val /
    eid / src_ids / num_dst; hop l (0 next to the seeds) uses the offset ``offset + l``"""
    dst = np.asarray(seeds, np.int64)
    blocks = []
    for hop, fanout in enumerate(fanouts):
        rp, c, eid = sample_neighbors_ref(rowptr, col, dst, fanout, seed, offset + hop)
        src, local = relabel_ref(dst, c)
        blocks.append(dict(rowptr=rp, col=local.astype(np.int32), val=np.asarray(val)[eid], eid=eid, src_ids=src, num_dst=len(dst)))
        dst = src
    return blocks[::-1], dst


_TIES = {}


def tied_pairs(seed=1, offset=0, count=TIE_SEARCH):
    """every pair (e1 < e2, key) of entry indices below ``count`` whose keys are equal and adjacent in (key, index) order,
    sorted by e2 - e1; computed once per (seed, offset, count)"""
    memo = (seed, offset, count)
    if memo not in _TIES:
        keys = entry_keys(np.arange(count, dtype=np.uint64), seed, offset)
        order = np.argsort(keys, kind="stable")        # equal keys stay in index order
        ks = keys[order]
        at = np.nonzero(ks[1:] == ks[:-1])[0]
        pairs = sorted(((int(order[i]), int(order[i + 1]), int(ks[i])) for i in at), key=lambda p: (p[1] - p[0], p[0]))
        _TIES[memo] = pairs
    return _TIES[memo]


def tie_row(e1, e2, key, seed=1, offset=0):
    """the row [e1 - 3, e2 + 4) and the fanout that puts the threshold between the tied entries: 1 + the number of its keys
    below the tied key → (b, e, fanout)"""
    b, e = e1 - 3, e2 + 4
    keys = entry_keys(np.arange(b, e, dtype=np.uint64), seed, offset)
    return b, e, 1 + int((keys < np.uint64(key)).sum())
