"""The numpy twin of the sampled sparse product (include/gcn_spmm.h: gcn_csr_sampled_dot_f32): plain loops in the order the
contract states, np.float32 arithmetic with one rounding per operation, np.searchsorted for the lookup in Y's row.  The GPU
tests compare with it bit for bit; tests/test_sampled_dot_cpu.py checks it against the dense formula and against
spgemm_ref."""
import numpy as np

ONE = np.float32(1)
ZERO = np.float32(0)


def _row(rp, r, nnz):
    """the entries [b, e) of row r — none when its row pointer pair is not usable"""
    b, e = int(rp[r]), int(rp[r + 1])
    return (b, e) if 0 <= b <= e <= nnz else (0, 0)


def sampled_dot_ref(p_rp, p_ci, np_cols, x_rp, x_ci, x_va, y_rp, y_ci, y_va, w, x_by_col=False, out=None):
    """out float32 [nnz_p]: for the entry e = (i, j) of P the products of X's row i (x_by_col: j) with Y's row j (x_by_col: i),
    added in X's entry order.  x_va / y_va None: ones.  Entries of a P row with an unusable row pointer keep what `out` held
    (NaN-free zeros when no `out` is given: pass one to see that nothing was written)."""
    mp = len(p_rp) - 1
    out = np.zeros(len(p_ci), np.float32) if out is None else out
    with np.errstate(all="ignore"):
        for i in range(mp):
            b, e = int(p_rp[i]), int(p_rp[i + 1])
            if not 0 <= b <= e <= len(p_ci):
                continue                                               # nothing is written for this row
            for pe in range(b, e):
                j = int(p_ci[pe])
                out[pe] = ZERO
                if not 0 <= j < np_cols:
                    continue
                xr, yr = (j, i) if x_by_col else (i, j)
                xb, xe = _row(x_rp, xr, len(x_ci))
                yb, ye = _row(y_rp, yr, len(y_ci))
                ycols = y_ci[yb:ye]
                acc = None
                for t in range(xb, xe):                                # X's entries, in entry order
                    c = int(x_ci[t])
                    if not 0 <= c < w:
                        continue
                    k = int(np.searchsorted(ycols, c))                 # the first entry of Y's row with a column >= c
                    if k == len(ycols) or ycols[k] != c:
                        continue
                    prod = np.float32((x_va[t] if x_va is not None else ONE) * (y_va[yb + k] if y_va is not None else ONE))
                    acc = prod if acc is None else np.float32(acc + prod)                 # the first product, not 0 + it
                if acc is not None:
                    out[pe] = acc
    return out
