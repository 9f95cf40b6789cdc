"""Point-cloud batches without a GPU: the new symbols and their argument counts, the sizes the host-only entry points refuse,
the route limit's shape, and the Python checks that run before any native call."""
import ctypes

import pytest
import torch

import gcn_amd
from gcn_amd import _lib

INVALID = 1                                            # GCN_ERR_INVALID_ARG


@pytest.mark.parametrize("name, nargs", [("gcn_fps_resident_points", 1), ("gcn_fps_ws_bytes", 4), ("gcn_fps_f32", 13),
                                         ("gcn_knn_segmented_ws_bytes", 4), ("gcn_knn_segmented_f32", 18)])
def test_new_symbols_resolve_with_the_stated_argument_counts(name, nargs):
    fn = getattr(gcn_amd.load_library(), name)
    assert name in _lib.SIGNATURES and fn.restype is ctypes.c_int and len(fn.argtypes) == nargs
    assert all(callable(f) for f in (gcn_amd.fps, gcn_amd.radius, gcn_amd.radius_graph))


def test_workspace_sizes_refuse_negative_sizes_and_a_null_result():
    lib, out = gcn_amd.load_library(), ctypes.c_size_t(0)
    for bad in ((-1, 3, 1), (5, 0, 1), (5, -1, 1), (5, 3, -1)):
        assert lib.gcn_fps_ws_bytes(*bad, ctypes.byref(out)) == INVALID, bad
    for bad in ((-1, 5, 3), (5, -1, 3), (5, 5, 0), (5, 5, _lib.KNN_K_MAX + 1)):
        assert lib.gcn_knn_segmented_ws_bytes(*bad, ctypes.byref(out)) == INVALID, bad
    assert lib.gcn_fps_ws_bytes(5, 3, 1, None) == INVALID and lib.gcn_knn_segmented_ws_bytes(5, 5, 3, None) == INVALID
    assert lib.gcn_knn_segmented_ws_bytes(5, 5, 3, ctypes.byref(out)) == 0 and out.value == 16
    limit = lib.gcn_fps_resident_points(3)             # dmin moves to the workspace once a cloud can pass the limit
    assert lib.gcn_fps_ws_bytes(limit, 3, 1, ctypes.byref(out)) == 0 and out.value == 16
    assert lib.gcn_fps_ws_bytes(limit + 1, 3, 1, ctypes.byref(out)) == 0 and out.value == 16 + (4 * (limit + 1) + 15) // 16 * 16


def test_the_resident_limit_serves_pointnet_clouds_and_never_grows_with_d():
    f = gcn_amd.load_library().gcn_fps_resident_points
    limits = [f(d) for d in range(1, 200)] + [f(1 << 20)]
    assert limits[2] >= 1024 and all(a >= b >= 0 for a, b in zip(limits, limits[1:]))
    assert f(0) == 0 and f(-3) == 0


def test_python_checks_run_before_any_native_call():
    cpu = torch.zeros((6, 3))
    for fn in (lambda t: gcn_amd.fps(t, count=2), lambda t: gcn_amd.radius(t, 1.0, 2), lambda t: gcn_amd.radius_graph(t, 1.0, 2),
               lambda t: gcn_amd.knn(t, 2, ptr_x=[0, 6]), lambda t: gcn_amd.knn_graph(t, 2, ptr=[0, 6])):
        with pytest.raises(TypeError):
            fn(cpu.double())
        with pytest.raises(gcn_amd.GcnAmdError, match="CPU"):
            fn(cpu)

    class _Dev(torch.Tensor):
        """a CPU tensor that claims to live on a device: enough to reach the checks behind the device check"""
        is_cuda = True

    x = cpu.as_subclass(_Dev)
    for kwargs in ({}, {"ratio": 0.5, "count": 2}, {"ratio": 0.0}, {"ratio": 1.5}, {"count": 0}, {"count": 2.0}):
        with pytest.raises(ValueError, match="ratio|count"):
            gcn_amd.fps(x, **kwargs)
    for ptr, match in (([0, 4, 2, 6], "ascend"), ([0, 5], "ends at 5"), ([1, 6], "start at 0"), ([], "ascend")):
        with pytest.raises(ValueError, match=match):
            gcn_amd.fps(x, ptr, count=2)
    with pytest.raises(ValueError, match="one row per cloud"):
        gcn_amd.fps(x, [0, 3, 6], count=2, start=[0])
    for ptr, match in (([0, 4, 2, 6], "ascend"), ([0, 5], "ends at 5")):
        with pytest.raises(ValueError, match=match):
            gcn_amd.knn(x, 2, ptr_x=ptr)
        with pytest.raises(ValueError, match=match):
            gcn_amd.radius_graph(x, 1.0, 2, ptr=ptr)
    with pytest.raises(ValueError, match="splits"):
        gcn_amd.knn(x, 2, splits=2, ptr_x=[0, 6])
    with pytest.raises(ValueError, match="ptr_y"):
        gcn_amd.knn(x, 2, y=x, ptr_x=[0, 6])
    with pytest.raises(ValueError, match="segments"):
        gcn_amd.radius(x, 1.0, 2, y=x, ptr_x=[0, 6], ptr_y=[0, 3, 6])
    for bad in (-1.0, float("inf"), float("nan"), "1", True):
        with pytest.raises(ValueError, match="r must be"):
            gcn_amd.radius(x, bad, 2)
    assert "ROUNDED TO fp32 AND THEN SQUARED" in gcn_amd.radius.__doc__ and "ONE host" in gcn_amd.radius_graph.__doc__
