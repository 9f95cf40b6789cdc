"""bf16 operands without a GPU: the new C entry points validate their arguments, the Python surface refuses what it
cannot run, and install() keeps routing fp32 only."""
import ctypes
import importlib

import torch

import gcn_amd
from gcn_amd import _lib
spmm_mod = importlib.import_module("gcn_amd.spmm")     # (the package attribute `spmm` is the function)

INVALID = 1                                     # GCN_ERR_INVALID_ARG


def test_bf16_entries_reject_a_null_plan_and_an_unknown_result_dtype():
    lib = _lib.load()
    null = ctypes.c_void_p()
    for c_dtype in (_lib.DTYPE_F32, _lib.DTYPE_BF16, 7):
        assert lib.gcn_spmm_csr_bf16_epilogue(None, null, null, null, null, null, c_dtype, null, 0, 0.0, 0, 0, 64, null) == INVALID
        assert lib.gcn_spmm_csr_bf16(None, null, null, null, null, null, c_dtype, 64, null) == INVALID
    buf = ctypes.create_string_buffer(64)
    assert lib.gcn_spmm_plan_main_kernel_bf16(None, 64, 0, buf, 64) == INVALID


def test_bf16_dropout_validates():
    lib = _lib.load()
    null = ctypes.c_void_p()
    assert lib.gcn_dropout_bf16(null, null, -1, 0.5, 0, 0, null) == INVALID
    assert lib.gcn_dropout_bf16(null, null, 4, 1.0, 0, 0, null) == INVALID
    assert lib.gcn_dropout_bf16(null, null, 4, 0.5, 0, 0, null) == INVALID       # (null buffers)
    assert lib.gcn_dropout_bf16(null, null, 0, 0.5, 0, 0, null) == 0


def test_matmul_raw_refuses_cpu_bf16_and_fp16():
    adj = gcn_amd.CsrAdjacency.__new__(gcn_amd.CsrAdjacency)      # (no device: the operand checks come first)
    adj.m = adj.n = 4
    for dt in (torch.bfloat16, torch.float16):
        try:
            adj.matmul_raw(torch.zeros((4, 8), dtype=dt))
        except gcn_amd.GcnAmdError:
            continue
        raise AssertionError(f"{dt} on the CPU was accepted")
    try:
        gcn_amd.dropout_rows(torch.zeros(4, dtype=torch.bfloat16), 0.5, 1, 1)
    except gcn_amd.GcnAmdError:
        pass
    else:
        raise AssertionError("dropout_rows accepted a CPU tensor")


def test_routing_still_requires_fp32():
    a = torch.eye(4).to_sparse()
    assert not spmm_mod._routable(a, torch.ones((4, 2), dtype=torch.bfloat16))
    assert not spmm_mod._routable(a.to(torch.bfloat16), torch.ones((4, 2), dtype=torch.bfloat16))


def test_gcn_compute_dtype_is_validated():
    gcn_amd.GCN(8, 4, 2, device="cpu", compute_dtype=torch.bfloat16)
    try:
        gcn_amd.GCN(8, 4, 2, device="cpu", compute_dtype=torch.float16)
    except ValueError:
        return
    raise AssertionError("fp16 compute_dtype was accepted")
