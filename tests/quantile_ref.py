"""The plain reference of gcn_amd.aggregate_quantile: per row and column, the element of rank floor(q (d - 1)) in the
(value, entry) order, by a stable argsort of the gathered slab."""
import math

import numpy as np


def quantile_ref(rp, col, x, qs):
    """(out fp32, arg int32), both [m, len(qs) k]: plane i is quantile qs[i]; an empty row 0 / -1; a column that holds a NaN
    the first NaN entry in every plane"""
    m, k = len(rp) - 1, x.shape[1]
    out = np.zeros((m, len(qs) * k), np.float32)
    arg = np.full((m, len(qs) * k), -1, np.int32)
    jj = np.arange(k)
    for r in range(m):
        b, d = int(rp[r]), int(rp[r + 1]) - int(rp[r])
        if d == 0:
            continue
        slab = x[col[b:b + d]]
        order = np.argsort(slab + np.float32(0.0), axis=0, kind="stable")        # (-0.0 + 0.0 is +0.0: the two tie)
        isnan = np.isnan(slab)
        for i, q in enumerate(qs):
            a = np.where(isnan.any(0), isnan.argmax(0), order[int(math.floor(q * (d - 1)))])
            out[r, i * k:(i + 1) * k], arg[r, i * k:(i + 1) * k] = slab[a, jj], b + a
    return out, arg
