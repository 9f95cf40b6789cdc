"""numpy twin of gcn_knn_f32 and of knn_hypergraph (the contract of include/gcn_spmm.h, re-implemented): distances by the
stated fp32 chain, keys, selection, row sums in fp64, and the hypergraph rule in fp64."""
import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
NAN_BITS = np.uint64(0x7FC00000)


def _fma_f32(diff, acc):
    """fl32(diff * diff + acc) with ONE rounding, for fp32 arrays with acc >= 0: the product of two fp32 is exact in fp64;
    the fp64 sum is made exact by TwoSum and rounded to odd, after which the rounding to fp32 is the correct one (53 >= 24 + 2
    bits)"""
    with np.errstate(over="ignore", invalid="ignore"):
        p = diff.astype(np.float64) * diff.astype(np.float64)
        a = acc.astype(np.float64)
        s = p + a
        bb = s - p
        e = (p - (s - bb)) + (a - bb)
        bits = s.view(np.int64).copy()
        fix = np.isfinite(s) & (e != 0) & ((bits & 1) == 0)
        bits[fix] += np.where(e[fix] > 0, 1, -1)           # (s > 0 here: the other neighbour of the true sum is the odd one)
        return bits.view(np.float64).astype(np.float32)


def dist2_ref(x, y):
    """fp32 [q, n]: acc = 0; for c ascending: diff = fl32(x_c - y_c); acc = fmaf(diff, diff, acc)"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    acc = np.zeros((x.shape[0], y.shape[0]), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(x.shape[1]):
            diff = (x[:, c, None] - y[None, :, c]).astype(np.float32)
            acc = _fma_f32(diff, acc)
    return acc


def keys_ref(d2):
    """uint64 [q, n]: (fp32 bits of d2, NaN of either sign as 0x7fc00000) << 32 | j"""
    d2 = np.ascontiguousarray(d2, np.float32)
    bits = d2.view(np.uint32).astype(np.uint64)
    bits[np.isnan(d2)] = NAN_BITS
    return (bits << np.uint64(32)) | np.arange(d2.shape[1], dtype=np.uint64)[None, :]


def select_ref(keys, k, self_offset=-1):
    """(idx int32 [q, k], dist2 fp32 [q, k]): the k smallest admissible keys of every row, ascending; tail -1 / +inf"""
    q, n = keys.shape
    idx = np.full((q, k), -1, np.int32)
    d2 = np.full((q, k), np.inf, np.float32)
    for i in range(q):
        row = keys[i]
        if self_offset >= 0 and 0 <= self_offset + i < n:
            row = np.delete(row, self_offset + i)
        row = np.sort(row)[:k]
        idx[i, :len(row)] = (row & np.uint64(0xFFFFFFFF)).astype(np.int64)
        d2[i, :len(row)] = (row >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return idx, d2


def knn_ref(x, y, k, self_offset=-1):
    """(idx, dist2, sum fp64 [q]) of gcn_knn_f32; the sum runs over all n candidates, the excluded one included"""
    d2 = dist2_ref(x, y)
    idx, out = select_ref(keys_ref(d2), k, self_offset)
    with np.errstate(invalid="ignore"):
        return idx, out, np.sqrt(d2.astype(np.float64)).sum(axis=1)


def dist2_f64(x):
    x = np.asarray(x, np.float64)
    diff = x[:, None, :] - x[None, :, :]
    return (diff * diff).sum(axis=2)


def knn_hypergraph_ref(x, k, prob=True, m_prob=1.0, d2=None):
    """dense fp64 H [n, len(k) n]: hyperedge c = {c} and the k - 1 nearest other vertices of c by (distance, index); the value
    exp(-d2 / (m_prob * avg_c)^2), avg_c the mean over ALL vertices of sqrt(d2[c, :]) (the centre's 0 included); 1 where
    d2 == 0.  d2: the squared distances to use (default: fp64 from the rows of x)."""
    ks = list(k) if isinstance(k, (list, tuple)) else [k]
    d2 = dist2_f64(x) if d2 is None else np.asarray(d2, np.float64)
    n = d2.shape[0]
    H = np.zeros((n, len(ks) * n))
    for g, kg in enumerate(ks):
        for c in range(n):
            others = np.delete(np.arange(n), c)
            order = others[np.lexsort((others, d2[c, others]))][:kg - 1]
            avg = np.sqrt(d2[c]).mean()
            H[c, g * n + c] = 1.0
            for v in order:
                H[v, g * n + c] = 1.0 if (not prob or d2[c, v] == 0) else np.exp(-d2[c, v] / (m_prob * avg) ** 2)
    return H


def laplacian_dense_ref(H):
    """fp64 G = Dv^-1/2 H De^-1 H^T Dv^-1/2 (unit hyperedge weights)"""
    H = np.asarray(H, np.float64)
    dv, de = H.sum(axis=1), H.sum(axis=0)
    L = H / np.sqrt(dv)[:, None]
    return (L / de[None, :]) @ L.T
