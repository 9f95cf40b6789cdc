"""The numpy twins of the sparse x sparse product (include/gcn_spmm.h: gcn_spgemm_count_csr / _fill_csr) and of
gcn_amd.hypergraph_laplacian: plain loops in the order the contract states, np.float32 arithmetic, one rounding per
operation.  The GPU tests compare with these bit for bit; tests/test_spgemm_cpu.py checks them against scipy and against
the dense formula."""
import numpy as np

ONE = np.float32(1)


def _usable(rp, i, nnz):
    return 0 <= rp[i] <= rp[i + 1] <= nnz


def spgemm_ref(a_rp, a_ci, a_va, b_rp, b_ci, b_va, p, n):
    """C = A · B -> (rowptr int32 [m + 1], col int32, val float32 or None, products int64 [m]).  a_va / b_va None: a
    pattern (ones); both None: no values.  products[i] is U_i of the contract: the lengths of the B rows the usable entries
    of A's row i point at, added up (what decides how the device takes the row)."""
    m = len(a_rp) - 1
    values = a_va is not None or b_va is not None
    rowptr = np.zeros(m + 1, np.int64)
    cols, vals = [], []
    products = np.zeros(m, np.int64)
    with np.errstate(all="ignore"):
        for i in range(m):
            acc = {}
            if _usable(a_rp, i, len(a_ci)):
                for x in range(a_rp[i], a_rp[i + 1]):                  # A's entries of the row, in entry order
                    j = a_ci[x]
                    if not (0 <= j < p and _usable(b_rp, j, len(b_ci))):
                        continue
                    products[i] += b_rp[j + 1] - b_rp[j]
                    av = a_va[x] if a_va is not None else ONE
                    for y in range(b_rp[j], b_rp[j + 1]):              # B's entries of row j, in entry order
                        c = int(b_ci[y])
                        if not 0 <= c < n:
                            continue
                        prod = np.float32(av * (b_va[y] if b_va is not None else ONE))
                        acc[c] = prod if c not in acc else np.float32(acc[c] + prod)     # the first product, not 0 + it
            order = sorted(acc)
            rowptr[i + 1] = rowptr[i] + len(order)
            cols.extend(order)
            vals.extend(acc[c] for c in order)
    return (rowptr.astype(np.int32), np.array(cols, np.int32), np.array(vals, np.float32) if values else None, products)


def transpose_ref(rp, ci, va, n):
    """the transpose [n x m] with the entries of a row by ascending source row (a stable bucketing by column)"""
    order = np.argsort(ci, kind="stable")
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    trp = np.zeros(n + 1, np.int64)
    trp[1:] = np.cumsum(np.bincount(ci, minlength=n))
    return trp.astype(np.int32), rows[order].astype(np.int32), va[order]


def sorted_merged_ref(rp, ci, va):
    """rows column-sorted (stably) with repeated columns added in fp32, left to right: coalesce_csr(adj, "sum")"""
    out_rp, out_ci, out_va = [0], [], []
    for i in range(len(rp) - 1):
        seg = np.arange(rp[i], rp[i + 1])
        seg = seg[np.argsort(ci[seg], kind="stable")]
        for x in seg:
            if len(out_ci) > out_rp[-1] and out_ci[-1] == ci[x]:
                out_va[-1] = np.float32(out_va[-1] + va[x])
            else:
                out_ci.append(ci[x])
                out_va.append(np.float32(va[x]))
        out_rp.append(len(out_ci))
    return np.array(out_rp, np.int32), np.array(out_ci, np.int32), np.array(out_va, np.float32)


def hypergraph_laplacian_ref(rp, ci, va, n_edges, w=None):
    """gcn_amd.hypergraph_laplacian -> (rowptr, col, val float32) of G [n x n]: H merged, Dv = H · w and De = Hᵀ · 1 in
    fp64 (added entry by entry: the order of an fp64 sum is not part of the contract, and the tests use values whose sums
    are exact), L = (h / sqrt(Dv_i)) * sqrt(w_e / De_e) in fp64 rounded to fp32 once, G = L · Lᵀ by spgemm_ref"""
    rp, ci, va = sorted_merged_ref(rp, ci, va)
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    w = np.ones(n_edges, np.float64) if w is None else np.asarray(w, np.float32).astype(np.float64)
    dv, de = np.zeros(n, np.float64), np.zeros(n_edges, np.float64)
    for x in range(len(ci)):
        dv[rows[x]] += np.float64(va[x]) * w[ci[x]]
        de[ci[x]] += np.float64(va[x])
    with np.errstate(all="ignore"):
        inv_dv = np.where(dv == 0, 0.0, 1.0 / np.sqrt(dv))
        edge = np.where(de == 0, 0.0, np.sqrt(w / de))
    lval = ((va.astype(np.float64) * inv_dv[rows]) * edge[ci]).astype(np.float32)
    trp, tci, tva = transpose_ref(rp, ci, lval, n_edges)
    return spgemm_ref(rp, ci, lval, trp, tci, tva, n_edges, n)[:3]
