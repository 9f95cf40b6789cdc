"""gcn_aggregate_multi_csr_f32 / _backward_csr_f32 refuse bad arguments before any device pointer is read: no GPU needed."""
import ctypes

import pytest
import torch

import gcn_amd

P = ctypes.c_void_p(64)                                # a non-null "device pointer" that must never be read
GOOD = dict(m=4, n=4, nnz=8, k=4, codes=(3, 0, 1, 5), eps=1e-5, out=P, argmax=P, argmin=P, ws=P, ws_bytes=16 + 64 * 4)


def forward(**kw):
    a = {**GOOD, **kw}
    codes = (ctypes.c_int32 * max(len(a["codes"]), 1))(*a["codes"]) if a["codes"] is not None else None
    nred = a.get("nred", len(a["codes"]) if a["codes"] is not None else 1)
    return gcn_amd.load_library().gcn_aggregate_multi_csr_f32(P, P, a["m"], a["n"], a["nnz"], P, a["k"], nred, codes, a["eps"], a["out"],
                                                              a["argmax"], a["argmin"], None, a["ws"], a["ws_bytes"], None)


@pytest.mark.parametrize("bad", [dict(m=-1), dict(nnz=-1), dict(k=0), dict(codes=()), dict(codes=None), dict(codes=(0, 1, 2, 3, 4, 5), nred=7),
                                 dict(codes=(3, 3)), dict(codes=(6,)), dict(codes=(-1,)), dict(eps=-1e-5), dict(eps=float("inf")),
                                 dict(eps=float("nan")), dict(eps=0.0), dict(out=None), dict(argmax=None), dict(argmin=None),
                                 dict(ws=None), dict(ws_bytes=16 + 64 * 4 - 1)])
def test_forward_argument_errors(bad):
    assert forward(**bad) == 1                          # GCN_ERR_INVALID_ARG


def test_backward_argument_errors_and_what_is_not_an_error():
    assert forward(m=0) == 0 and forward(m=0, codes=(4,), eps=0.0, argmax=None, argmin=None) == 0       # nothing launched
    codes = (ctypes.c_int32 * 2)(4, 0)                  # var and max: needs ab, rowptr, argmax and the saved mean
    f = gcn_amd.load_library().gcn_aggregate_multi_backward_csr_f32
    call = lambda argmax=P, mean=P, ab=P, gx=P, n=4: f(P, P, P, P, n, 4, 8, P, P, 4, 2, codes, P, argmax, None, mean, ab, gx, P, 16 + 64 * 4, None)
    assert call(n=0) == 0
    for bad in (dict(argmax=None), dict(mean=None), dict(ab=None), dict(gx=None), dict(n=-1)):
        assert call(**bad) == 1, bad


def test_python_front_end_errors():
    with pytest.raises(TypeError):
        gcn_amd.aggregate_multi(None, torch.ones(4, 4))
    for bad in (dict(aggregators=("mean", "median")), dict(scalers=("identity", "identity"))):
        with pytest.raises(ValueError):
            gcn_amd.PNAConv(4, 4, avg_log_degree=1.0, **bad)
    assert gcn_amd.PNAConv(4, 2, avg_log_degree=1.0).weight.shape == (52, 2)
