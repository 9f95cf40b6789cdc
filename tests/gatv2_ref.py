"""fp64 numpy twin of the GATv2 score and its backward (gcn_amd/csrc/multihead.hip, include/gcn_spmm.h), written a second
time on the host with no regard for speed or summation order: per-entry [., H*F] arrays and incidence matrices, a block
of entries at a time.

    s[e, h] = sum_j att[h, j] * leaky_relu(h_dst[row(e), hF+j] + h_src[col[e], hF+j], slope)

Layouts as in the header: node arrays [rows, H*F] with head h in columns hF .. hF+F-1, per-entry arrays [nnz, H], att
[H, F].  The derivative of leaky_relu at 0 is the slope."""
import numpy as np
import scipy.sparse as sp

from heads_ref import entry_rows

BLOCK = 1 << 14                                           # entries at a time: the per-entry arrays are [BLOCK, H*F]


def _blocks(rowptr, col, h_dst, h_src):
    """(entries e, their rows, their columns, t [len(e), k] in fp64) block by block; of fp32 inputs the sign of t is the
    sign of the fp32 sum"""
    row, col = entry_rows(rowptr), np.asarray(col, np.int64)
    h_dst, h_src = np.asarray(h_dst, np.float64), np.asarray(h_src, np.float64)
    for b in range(0, len(col), BLOCK):
        e = slice(b, min(b + BLOCK, len(col)))
        yield e, row[e], col[e], h_dst[row[e]] + h_src[col[e]]


def _incidence(index, rows):
    """[rows, len(index)] 0/1 matrix: row index[i] holds i"""
    return sp.csr_matrix((np.ones(len(index)), (index, np.arange(len(index)))), shape=(rows, len(index)))


def scores(rowptr, col, h_dst, h_src, att, slope):
    att = np.asarray(att, np.float64)
    H, F = att.shape
    out = np.zeros((len(col), H))
    for e, _r, _c, t in _blocks(rowptr, col, h_dst, h_src):
        out[e] = (np.where(t > 0, t, float(slope) * t).reshape(-1, H, F) * att).sum(-1)
    return out


def scores_magnitude(rowptr, col, h_dst, h_src, att, slope):
    """sum_j |att| max(1, |slope|) (|h_dst| + |h_src|) per (entry, head)"""
    att = np.abs(np.asarray(att, np.float64))
    H, F = att.shape
    out = np.zeros((len(col), H))
    for e, _r, _c, t in _blocks(rowptr, col, np.abs(h_dst), np.abs(h_src)):
        out[e] = (t.reshape(-1, H, F) * att).sum(-1) * max(1.0, abs(float(slope)))
    return out


def backward(rowptr, col, n, h_dst, h_src, att, slope, g):
    """(grad_h_dst [m, k], grad_h_src [n, k], act_sums [m, k], grad_att [H, F]) for the upstream gradient g [nnz, H]"""
    att, g = np.asarray(att, np.float64), np.asarray(g, np.float64)
    H, F = att.shape
    m = len(rowptr) - 1
    mask_dst, mask_src, act_sums = np.zeros((m, H * F)), np.zeros((n, H * F)), np.zeros((m, H * F))
    for e, r, c, t in _blocks(rowptr, col, h_dst, h_src):
        D = np.where(t > 0, 1.0, float(slope))
        gk = np.repeat(g[e], F, axis=1)                                   # [., k]: column hF+j carries g[., h]
        R = _incidence(r, m)
        mask_dst += R @ (gk * D)
        mask_src += _incidence(c, n) @ (gk * D)
        act_sums += R @ (gk * (t * D))
    flat = att.reshape(1, -1)
    return flat * mask_dst, flat * mask_src, act_sums, act_sums.sum(0).reshape(H, F)


def backward_magnitudes(rowptr, col, n, h_dst, h_src, att, slope, g):
    """sum |terms| of the three kernel outputs: |att| sum_e |g| max(1, |slope|) on either side, and
    sum_e |g| max(1, |slope|) (|h_dst| + |h_src|) for act_sums"""
    att, g = np.abs(np.asarray(att, np.float64)), np.abs(np.asarray(g, np.float64)) * max(1.0, abs(float(slope)))
    H, F = att.shape
    m = len(rowptr) - 1
    mag_dst, mag_src, mag_act = np.zeros((m, H * F)), np.zeros((n, H * F)), np.zeros((m, H * F))
    for e, r, c, t in _blocks(rowptr, col, np.abs(h_dst), np.abs(h_src)):
        gk = np.repeat(g[e], F, axis=1)
        R = _incidence(r, m)
        mag_dst += R @ gk
        mag_src += _incidence(c, n) @ gk
        mag_act += R @ (gk * t)
    flat = att.reshape(1, -1)
    return flat * mag_dst, flat * mag_src, mag_act
