"""Brute-force k nearest neighbours on the device, and the graphs built from them.

    idx, dist2 = gcn_amd.knn(x, 16)                        # the 16 nearest rows of x for every row of x (itself included)
    adj = gcn_amd.knn_graph(x, 16)                         # CsrAdjacency [n x n]: row i holds its 16 nearest other rows
    H = gcn_amd.knn_hypergraph(x, 10)                      # incidence matrix [n x n] of the HGNN construction
    G = gcn_amd.hypergraph_laplacian(H)

The primitive is an exact contract written out in include/gcn_spmm.h (``gcn_knn_f32``) and runs on gcn_amd/csrc/knn.hip;
tests/knn_ref.py is its numpy twin.  The q x n distance matrix is never formed.  There is no CPU path: CPU operands raise.
"""
import ctypes

import torch

from . import _lib
from .construct import transpose_csr
from ._lib import call
from .spmm import CsrAdjacency

KNN_K_MAX = _lib.KNN_K_MAX


def _rows(t, d):
    """(tensor, row stride) as the kernel takes it: unit column stride and a row stride >= d pass as they are"""
    if (d > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < d):
        t = t.contiguous()
    return t, (max(int(t.stride(0)), d) if t.shape[0] > 1 else d)


def _knn(x, y, k, self_offset, splits, want_dist2=True, want_sum=False):
    """(idx int32 [q, k], dist2 fp32 [q, k] or None, sum fp64 [q] or None) of one gcn_knn_f32 call on checked operands"""
    dev = x.device
    q, d, n = int(x.shape[0]), int(x.shape[1]), int(y.shape[0])
    idx = torch.empty((q, k), dtype=torch.int32, device=dev)
    dist2 = torch.empty((q, k), dtype=torch.float32, device=dev) if want_dist2 else None
    rsum = torch.empty(q, dtype=torch.float64, device=dev) if want_sum else None
    if q == 0:
        return idx, dist2, rsum
    x, ldx = _rows(x.detach(), d)
    y, ldy = _rows(y.detach(), d)
    nbytes = ctypes.c_size_t(0)
    with torch.cuda.device(dev):                           # (the rule counts the CUs of the current device)
        call("gcn_knn_ws_bytes", q, n, k, splits, ctypes.byref(nbytes))
    ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
    call("gcn_knn_f32", x, ldx, y, ldy, q, n, d, k, self_offset, splits, idx, dist2, rsum, ws, ws.numel(), device=dev)
    return idx, dist2, rsum


def _check_points(what, x, y=None):
    for t in (x,) if y is None else (x, y):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError(f"{what}: x and y must be fp32 tensors")
    for t in (x,) if y is None else (x, y):
        if not t.is_cuda:
            raise _lib.GcnAmdError(f"{what}: x and y must be CUDA/HIP tensors (no CPU path in gcn_amd)")
    if y is not None and x.device != y.device:
        raise _lib.GcnAmdError(f"{what}: x and y must live on one device, not {x.device} and {y.device}")
    for t in (x,) if y is None else (x, y):
        if t.dim() != 2 or t.shape[1] < 1:
            raise ValueError(f"{what}: x and y must be 2-D [rows, d] with d >= 1, not {tuple(t.shape)}")
    if y is not None and x.shape[1] != y.shape[1]:
        raise ValueError(f"{what}: x has {x.shape[1]} columns and y has {y.shape[1]}: they must agree")
    if max(x.shape[0], 0 if y is None else y.shape[0]) >= 2 ** 31:
        raise ValueError(f"{what}: fewer than 2^31 rows")


def _check_k(what, k, top=KNN_K_MAX):
    if isinstance(k, bool) or not isinstance(k, int) or k < 1 or k > top:
        raise ValueError(f"{what}: k must be an int in [1, {top}], not {k!r}")


def knn(x, k, y=None, exclude_self=False, splits=0, self_offset=None):
    """The k nearest rows of ``y`` for every row of ``x`` by squared Euclidean distance, brute force on the device: returns
    ``(idx int32 [q, k], dist2 fp32 [q, k])``.

    x: fp32 [q, d]; y: fp32 [n, d], None = search x in x.  The distance of a pair is the fp32 chain ``acc = fmaf(x_c - y_c,
    x_c - y_c, acc)`` over ascending columns: exactly 0 for a row and its duplicate, the same bits in both directions, the
    same at every call.  A row lists its neighbours ascending by (distance, index): on equal distances the smaller index
    comes first; a NaN distance ranks behind every number.  With fewer than k admissible candidates the tail is index -1 and
    distance +inf.
    exclude_self=True: candidate i is not admissible for query i; allowed only with y=None or an explicit ``self_offset``
    (the queries are rows [self_offset, self_offset + q) of y).
    splits: parts the candidate range is cut into so that few queries still fill the chip; 0 lets the library choose, and
    ``idx`` / ``dist2`` do not depend on it.
    Rows with unit column stride are passed by their row stride; anything else is made contiguous.  Not differentiable.
    No host synchronisation.
    The checks, in this order: TypeError for a non-tensor or a dtype other than fp32; GcnAmdError for CPU tensors or two
    devices; ValueError for shapes (2-D, equal d >= 1), for k outside [1, KNN_K_MAX], and for exclude_self / self_offset /
    splits that make no sense."""
    what = "knn"
    _check_points(what, x, y)
    _check_k(what, k)
    if self_offset is not None and (isinstance(self_offset, bool) or not isinstance(self_offset, int) or self_offset < 0):
        raise ValueError(f"{what}: self_offset must be None or an int >= 0, not {self_offset!r}")
    if exclude_self and y is not None and self_offset is None:
        raise ValueError(f"{what}: exclude_self=True needs y=None or an explicit self_offset")
    if self_offset is not None and not exclude_self:
        raise ValueError(f"{what}: self_offset is only meaningful with exclude_self=True")
    if isinstance(splits, bool) or not isinstance(splits, int) or splits < 0:
        raise ValueError(f"{what}: splits must be an int >= 0, not {splits!r}")
    off = -1 if not exclude_self else (0 if self_offset is None else self_offset)
    idx, dist2, _ = _knn(x, x if y is None else y, k, off, splits)
    return idx, dist2


def knn_graph(x, k, loop=False, values=None):
    """The k-nearest-neighbour graph of the rows of ``x`` (fp32 [n, d]) on the device: returns a CsrAdjacency [n x n] whose
    row i holds the k nearest rows of i, columns ascending, flagged ``symmetric=False``.

    loop=False: the vertex itself is excluded and a row has ``min(k, n - 1)`` entries.  True: it takes part as a candidate
    (at distance 0 it comes first, unless duplicates with a smaller index fill the row) and a row has ``min(k, n)`` entries.
    Every row has the same length, so the row pointer is arithmetic and nothing is read back: no host synchronisation.
    values: None = ones; "distance" = the fp32 square roots of the squared distances ``knn`` returns.
    The way on to a normalised Â is the existing merge: ``normalize_csr(symmetrize(knn_graph(x, k)), "sym")`` — the
    neighbour relation is not symmetric, ``symmetrize`` adds the missing directions.
    The checks are those of ``knn``, then ValueError for unknown ``values``."""
    what = "knn_graph"
    _check_points(what, x)
    _check_k(what, k)
    if values is not None and values != "distance":
        raise ValueError(f"{what}: values must be None or \"distance\", not {values!r}")
    dev, n = x.device, int(x.shape[0])
    kk = min(k, n if loop else n - 1)
    if n * max(kk, 0) >= 2 ** 31:
        raise ValueError(f"{what}: n * k must stay below 2^31")
    if kk <= 0:
        return CsrAdjacency(torch.zeros(n + 1, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                            torch.zeros(0, dtype=torch.float32, device=dev), (n, n), symmetric=False)
    idx, dist2, _ = _knn(x, x, kk, -1 if loop else 0, 0, want_dist2=values is not None)
    col, order = idx.sort(dim=1)
    val = torch.ones(n * kk, dtype=torch.float32, device=dev) if values is None else dist2.gather(1, order).sqrt().reshape(-1)
    rowptr = (torch.arange(n + 1, dtype=torch.int64, device=dev) * kk).to(torch.int32)
    return CsrAdjacency(rowptr, col.reshape(-1), val, (n, n), symmetric=False)


def knn_hypergraph(x, k, prob=True, m_prob=1.0):
    """The incidence matrix H of the k-nearest-neighbour hypergraph of the rows of ``x`` (fp32 [n, d]), on the device:
    returns a CsrAdjacency [n vertices x n hyperedges], columns ascending, flagged ``symmetric=False``.

    Hyperedge c is ``{c}`` and the ``k - 1`` nearest other vertices of c (by ``knn``'s order: ties go to the smaller index).
    prob=False: every value is 1.  True: vertex v of hyperedge c gets ``exp(-d2(c, v) / (m_prob * avg_c)^2)`` with ``avg_c``
    the mean distance from c to every vertex, itself included; the expression is evaluated in fp64 from the fp32 squared
    distance and rounded to fp32 once.  The centre, and any member at distance 0, gets exactly 1.
    k: an int in [1, KNN_K_MAX], or a list of them: the hyperedge groups are then concatenated column-wise, n x (len(k) n).
    ``hypergraph_laplacian(knn_hypergraph(x, k))`` is the matrix an HGNN layer multiplies with.
    No host synchronisation (one ``knn`` call per k, index arithmetic, one ``transpose_csr``).
    The checks are those of ``knn``, then ValueError for an m_prob that is not a positive number."""
    what = "knn_hypergraph"
    _check_points(what, x)
    ks = list(k) if isinstance(k, (list, tuple)) else [k]
    if not ks:
        raise ValueError(f"{what}: k must not be an empty list")
    for kg in ks:
        _check_k(what, kg)
    if isinstance(m_prob, bool) or not isinstance(m_prob, (int, float)) or not m_prob > 0:
        raise ValueError(f"{what}: m_prob must be a positive number, not {m_prob!r}")
    dev, n = x.device, int(x.shape[0])
    if n * sum(min(kg, max(n, 1)) for kg in ks) >= 2 ** 31:
        raise ValueError(f"{what}: n * sum(k) must stay below 2^31")
    centre = torch.arange(n, dtype=torch.int32, device=dev).unsqueeze(1)
    members, weights, lens = [], [], []
    for kg in ks:
        kk = min(kg - 1, n - 1)                            # the others of a hyperedge
        if kk > 0:
            idx, dist2, rsum = _knn(x, x, kk, 0, 0, want_dist2=prob, want_sum=prob)
            members.append(torch.cat([centre, idx], dim=1).reshape(-1))
        else:
            members.append(centre.reshape(-1))
        if prob and kk > 0:
            d2 = dist2.double()
            scale = (float(m_prob) * (rsum / n)).square().unsqueeze(1)
            w = torch.where(d2 == 0, torch.ones_like(d2), torch.exp(-d2 / scale)).float()
            weights.append(torch.cat([torch.ones((n, 1), dtype=torch.float32, device=dev), w], dim=1).reshape(-1))
        else:
            weights.append(torch.ones(n * (max(kk, 0) + 1), dtype=torch.float32, device=dev))
        lens.append(max(kk, 0) + 1)
    # rows by hyperedge (every group's row pointer is arithmetic), then the transpose: rows by vertex, ascending by hyperedge
    starts, base = [], 0
    for ln in lens:
        starts.append(base + torch.arange(n, dtype=torch.int64, device=dev) * ln)
        base += n * ln
    rowptr = torch.cat(starts + [torch.full((1,), base, dtype=torch.int64, device=dev)]).to(torch.int32)
    by_edge = CsrAdjacency(rowptr, torch.cat(members), torch.cat(weights), (len(ks) * n, n), symmetric=False)
    H, _ = transpose_csr(by_edge)
    return H
