"""numpy twin of the subgraph contracts of include/gcn_spmm.h (gcn_induced_subgraph_count_csr / _fill_csr and
gcn_random_walk_csr): what the device results are compared with, integer for integer.  Keys come from util.philox4x32_10."""
import numpy as np

from util import philox4x32_10, random_rows_csr


def induced_subgraph_ref(rowptr, col, nodes, n=None):
    """→ (rowptr [len(nodes) + 1], col, eid), int32: row i holds the entries e of row nodes[i] whose column is in nodes, in
    ascending e, as the column's position in nodes and as e"""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    nodes = np.asarray(nodes, np.int64)
    n = int(n if n is not None else max(len(rowptr) - 1, int(col.max()) + 1 if len(col) else 0))
    vmap = np.full(n, -1, np.int64)
    vmap[nodes] = np.arange(len(nodes))
    out_rowptr, cols, eids = np.zeros(len(nodes) + 1, np.int64), [], []
    for i, v in enumerate(nodes):
        e = np.arange(rowptr[v], rowptr[v + 1], dtype=np.int64)
        e = e[vmap[col[e]] >= 0]
        out_rowptr[i + 1] = out_rowptr[i] + len(e)
        cols.append(vmap[col[e]])
        eids.append(e)
    cat = lambda parts: (np.concatenate(parts) if parts else np.zeros(0, np.int64)).astype(np.int32)
    return out_rowptr.astype(np.int32), cat(cols), cat(eids)


def walk_keys(n_walks, length, seed, offset):
    """key[i, t] of the contract: word (j & 3) of Philox4x32-10(counter = (lo32(j >> 2), hi32(j >> 2), lo32(offset),
    hi32(offset)), key = (lo32(seed), hi32(seed))), j = i * L4 + t, L4 = 4 * ceil(length / 4) → uint64 [n_walks, length]"""
    seed, offset = int(seed), int(offset)
    groups = (length + 3) // 4
    g = (np.arange(n_walks, dtype=np.uint64)[:, None] * np.uint64(groups) + np.arange(groups, dtype=np.uint64)[None, :]).reshape(-1)
    words = philox4x32_10((g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), offset & 0xFFFFFFFF, offset >> 32),
                          (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(words, axis=1).reshape(n_walks, 4 * groups)[:, :length]       # [walk, 4 * group + word]


def random_walk_ref(rowptr, col, starts, length, seed=0, offset=0):
    """→ int32 [len(starts), length + 1]: walk i in row i (the layout gcn_amd.random_walk returns)"""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    m = len(rowptr) - 1
    v = np.asarray(starts, np.int64).copy()
    out = np.empty((len(v), length + 1), np.int64)
    bad = (v < 0) | (v >= m)
    out[:, 0] = v
    keys = walk_keys(len(v), length, seed, offset)
    for t in range(length):
        vc = np.where(bad, 0, v)
        b, d = rowptr[vc], rowptr[vc + 1] - rowptr[vc]
        pick = ((keys[:, t] * d.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)     # (32 x 32 bits: no overflow in uint64)
        move = (d > 0) & ~bad
        c = np.where(move, col[np.where(move, b + pick, 0)] if len(col) else 0, v)
        v = np.where(move & (c >= 0) & (c < m), c, v)
        out[:, t + 1] = v
    out[bad] = -1
    return out.astype(np.int32)


def walk_graph():
    """the graph of the walk tests: 300 vertices with 0 .. 5 entries each, so about a sixth of them are dead ends (and the
    start of a walk that never moves) → (rowptr, col)"""
    lens = np.random.default_rng(21).integers(0, 6, 300)
    return random_rows_csr(300, 300, lens, seed=22)
