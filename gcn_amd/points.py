"""Batches of point clouds stored back to back: farthest point sampling, radius search and the radius graph.

    idx, out_ptr = gcn_amd.fps(x, ptr, ratio=0.25)                          # every cloud's picks, global rows, in pick order
    nbr, d2 = gcn_amd.radius(x[idx.long()], 0.2, 32, y=x, ptr_x=out_ptr, ptr_y=ptr)    # ball query around the picks
    adj = gcn_amd.radius_graph(x, 0.2, 32, ptr=ptr)                         # CsrAdjacency, neighbours within a cloud only

``ptr`` is the batch as B + 1 ascending row numbers; ``gcn_amd.knn`` / ``knn_graph`` take the same pointers.  The contracts
are written out in include/gcn_spmm.h (``gcn_fps_f32``, ``gcn_knn_segmented_f32``) and run on gcn_amd/csrc/fps.hip and
knn.hip.  Everything is exact and deterministic: distances are the fp32 chain of ``knn``, ties go to the smaller index.
There is no CPU path: CPU operands raise.  Nothing here is differentiable.
"""
import ctypes
import math

import torch

from ._lib import call
from .knn import (_check_k, _check_points, _check_ptr, _csr_of_neighbours, _device_ptrs, _knn_segmented, _pair_ptrs, _rows,
                  _upload)


def fps(x, ptr=None, ratio=None, count=None, start=None, return_dist2=False):
    """Farthest point sampling of every cloud of a batch, on the device: returns ``(idx int32 [M], out_ptr)``, and with
    return_dist2=True ``(idx, out_ptr, dist2 fp32 [M])``.

    x: fp32 [n, d], the clouds back to back.  ptr: a HOST sequence of B + 1 ascending ints from 0 to n, None = one cloud.  It
    stays on the host because the size of the output depends on it: nothing is read back from the device.
    Exactly one of ``ratio`` in (0, 1] (``m_b = ceil(ratio * n_b)``) and ``count`` >= 1 (``m_b = min(count, n_b)``).
    start: None = every cloud starts from its first row; else B global row numbers (a host sequence, or an int32 device
    tensor), each clamped into its cloud.
    idx: the picks of cloud b are ``idx[out_ptr[b]:out_ptr[b + 1]]``, global rows of x in pick order.  Pick 0 is the start
    row; each later pick is the unpicked row farthest from the picks so far (the distance of a pair is ``knn``'s fp32 chain,
    a NaN distance counts as 0, the smaller index wins a tie), so a cloud's picks are distinct.  dist2: that distance at the
    moment of the pick, +inf for pick 0.  out_ptr: the host list of the picks' segment pointers, ready to be the next ``ptr``.
    One workgroup runs one cloud; clouds of up to ``gcn_fps_resident_points(d)`` rows never leave the chip between picks.
    The two pointer arrays (and a host ``start``) go up in one small copy.  No host synchronisation.
    The checks, in this order: TypeError for a non-tensor or a dtype other than fp32; GcnAmdError for a CPU tensor;
    ValueError for the shape, for ratio / count (both, neither, out of range), for ptr and for start."""
    what = "fps"
    _check_points(what, x)
    if (ratio is None) == (count is None):
        raise ValueError(f"{what}: give exactly one of ratio and count")
    if ratio is not None and (isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not 0 < ratio <= 1):
        raise ValueError(f"{what}: ratio must be a number in (0, 1], not {ratio!r}")
    if count is not None and (isinstance(count, bool) or not isinstance(count, int) or count < 1):
        raise ValueError(f"{what}: count must be an int >= 1, not {count!r}")
    dev, n, d = x.device, int(x.shape[0]), int(x.shape[1])
    if isinstance(ptr, torch.Tensor):
        raise ValueError(f"{what}: ptr must be a host sequence (the output size depends on it), not a tensor")
    ptr = [0, n] if ptr is None else _check_ptr(what, "ptr", ptr, n)
    if ptr[0] != 0:
        raise ValueError(f"{what}: ptr must start at 0")
    segments = len(ptr) - 1
    sizes = [b - a for a, b in zip(ptr, ptr[1:])]
    picks = [min(count, nb) if ratio is None else min(nb, math.ceil(ratio * nb)) for nb in sizes]
    out_ptr = [0]
    for m in picks:
        out_ptr.append(out_ptr[-1] + m)
    lists = [ptr, out_ptr]
    if start is not None and not isinstance(start, torch.Tensor):
        try:
            start = [int(v) for v in start]
        except (TypeError, ValueError):
            raise ValueError(f"{what}: start must be a sequence of ints or an int32 device tensor, not {start!r}") from None
        lists.append(start)
    if start is not None and len(start) != segments:
        raise ValueError(f"{what}: start must name one row per cloud ({segments}), not {len(start)}")
    if isinstance(start, torch.Tensor):
        (start,) = _device_ptrs(what, dev, [("start", start, None)])
    total = out_ptr[-1]
    idx = torch.empty(total, dtype=torch.int32, device=dev)
    dist2 = torch.empty(total, dtype=torch.float32, device=dev) if return_dist2 else None
    if total > 0:
        up = _upload(dev, lists)
        xr, ldx = _rows(x.detach(), d)
        nbytes = ctypes.c_size_t(0)
        call("gcn_fps_ws_bytes", n, d, segments, ctypes.byref(nbytes))
        ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
        call("gcn_fps_f32", xr, ldx, n, d, up[0], up[1], up[2] if len(up) > 2 else start, segments, idx, dist2, ws, ws.numel(),
             device=dev)
    return (idx, out_ptr, dist2) if return_dist2 else (idx, out_ptr)


def _radius2(what, r):
    if isinstance(r, bool) or not isinstance(r, (int, float)) or not (0 <= r < math.inf):
        raise ValueError(f"{what}: r must be a finite number >= 0, not {r!r}")
    r32 = torch.tensor(float(r), dtype=torch.float32)
    return float(r32 * r32)


def radius(x, r, k, y=None, ptr_x=None, ptr_y=None, exclude_self=False):
    """At most k rows of ``y`` within distance r of every row of ``x`` (a ball query), on the device: returns ``(idx int32
    [q, k], dist2 fp32 [q, k])`` as ``knn`` does: ascending by (distance, index), the tail index -1 and distance +inf.

    r: a finite number >= 0.  The test is ``dist2 <= radius2`` on ``knn``'s fp32 squared distance, inclusive, where radius2 is
    r ROUNDED TO fp32 AND THEN SQUARED IN fp32 (one more rounding) — not the square of r in double precision.  A NaN distance
    is never inside.  With more than k rows inside, the k NEAREST are kept (ties to the smaller index), not the first k met.
    y=None searches x in x.  ptr_x, ptr_y: as in ``knn``: neighbours come from the query's own segment only; None = one
    segment.  exclude_self: row i is no neighbour of query i (y=None only).
    No host synchronisation.  The checks are those of ``knn``, then ValueError for r."""
    what = "radius"
    _check_points(what, x, y)
    _check_k(what, k)
    if exclude_self and y is not None:
        raise ValueError(f"{what}: exclude_self=True needs y=None")
    r2 = _radius2(what, r)
    if ptr_x is None and ptr_y is None:
        ptr_x, ptr_y = [0, int(x.shape[0])], [0, int((x if y is None else y).shape[0])]
    else:
        ptr_x, ptr_y = _pair_ptrs(what, y, ptr_x, ptr_y)
    return _knn_segmented(what, x, x if y is None else y, k, 0 if exclude_self else -1, r2, ptr_x, ptr_y)


def radius_graph(x, r, max_num_neighbors, ptr=None, loop=False):
    """The graph that joins every row of ``x`` (fp32 [n, d]) to the rows of its own cloud within distance r: returns a
    CsrAdjacency [n x n] with unit values, columns ascending within a row, flagged ``symmetric=False``.

    r: as in ``radius`` (inclusive, fp32).  max_num_neighbors: at most this many entries per row (an int in [1, KNN_K_MAX]);
    a row with more rows inside the ball keeps the nearest ones, so the relation need not be symmetric.  ptr: the clouds'
    segment pointers, None = one cloud.  loop=False leaves the row itself out.
    Row lengths vary: the row pointer is a device cumsum of the per-row counts and the entry count is read back — ONE host
    synchronisation.  The checks are those of ``radius``."""
    what = "radius_graph"
    _check_points(what, x)
    _check_k(what, max_num_neighbors)
    r2 = _radius2(what, r)
    n = int(x.shape[0])
    if n * max_num_neighbors >= 2 ** 31:
        raise ValueError(f"{what}: n * max_num_neighbors must stay below 2^31")
    ptr = [0, n] if ptr is None else ptr
    idx, _ = _knn_segmented(what, x, x, max_num_neighbors, -1 if loop else 0, r2, ptr, ptr, want_dist2=False)
    return _csr_of_neighbours(idx, None, n, None)
