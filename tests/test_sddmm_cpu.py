"""Learnable edge weights without a GPU: the SDDMM / mutable-value entry points are exported and bound, CPU tensors are
refused (no CPU path), a wrong values length is a ValueError, and default routing still refuses grad-requiring sparse
operands."""
import ctypes
import importlib

import pytest
import torch

import gcn_amd
from gcn_amd import _lib

spmm_mod = importlib.import_module("gcn_amd.spmm")     # (the package's `spmm` attribute is the function)

NEW = ["gcn_sddmm_csr_f32", "gcn_spmm_plan_set_values_mutable", "gcn_spmm_plan_update_values",
       "gcn_spmm_plan_values_mutable", "gcn_spmm_plan_sddmm_kernel"]


@pytest.mark.parametrize("name", NEW)
def test_new_symbols_exported_and_bound(name):
    lib = ctypes.CDLL(gcn_amd.LIB_PATH)
    assert hasattr(lib, name)
    assert name in _lib.SIGNATURES
    fn = getattr(gcn_amd.load_library(), name)
    assert fn.argtypes == _lib.SIGNATURES[name][1]


def test_null_plan_is_rejected():
    lib = gcn_amd.load_library()
    assert lib.gcn_sddmm_csr_f32(None, None, None, None, None, None, 8, None) == 1
    assert lib.gcn_spmm_plan_update_values(None, None, None) == 1
    assert lib.gcn_spmm_plan_set_values_mutable(None, None, None, None, None) == 1
    assert lib.gcn_spmm_plan_values_mutable(None) == -1
    assert lib.gcn_spmm_plan_sddmm_kernel(None, 8, ctypes.create_string_buffer(64), 64) == 1


class _FakeAdj(gcn_amd.CsrAdjacency):
    """a CsrAdjacency shell with host arrays (the constructor refuses CPU tensors): enough to reach the checks that run
    before any native call"""

    def __init__(self):
        self.m = self.n = 3
        self.nnz = 4
        self.rowptr = torch.tensor([0, 2, 3, 4], dtype=torch.int32)
        self.col = torch.tensor([0, 1, 2, 0], dtype=torch.int32)
        self.val = torch.ones(4)
        self.device = torch.device("cpu")
        self.mutable_values = True
        self._plan = None
        self._transpose = None


def test_cpu_tensors_raise():
    rp = torch.tensor([0, 1], dtype=torch.int32)
    with pytest.raises(gcn_amd.GcnAmdError):
        gcn_amd.CsrAdjacency(rp, torch.zeros(1, dtype=torch.int32), torch.ones(1), (1, 1), mutable_values=True)
    adj = _FakeAdj()
    with pytest.raises(gcn_amd.GcnAmdError):
        adj.update_values(torch.ones(4))
    with pytest.raises(gcn_amd.GcnAmdError):
        adj.sddmm(torch.ones(3, 8), torch.ones(3, 8))
    with pytest.raises(gcn_amd.GcnAmdError):
        gcn_amd.spmm(adj, torch.ones(3, 8), values=torch.ones(4, requires_grad=True))


def test_wrong_values_length_is_a_value_error():
    adj = _FakeAdj()
    for bad in (torch.ones(5), torch.ones(3), torch.ones(2, 2)):
        with pytest.raises(ValueError):
            gcn_amd.spmm(adj, torch.ones(3, 8), values=bad)
        with pytest.raises(ValueError):
            adj.update_values(bad)


def test_default_routing_refuses_grad_requiring_sparse_operands():
    a = torch.sparse_coo_tensor(torch.tensor([[0, 1], [1, 0]]), torch.ones(2), (2, 2)).coalesce().requires_grad_(True)
    b = torch.ones(2, 3)
    assert not spmm_mod._routable(a, b)
    assert not spmm_mod._routable_grad(a, b)          # (host tensors: never routed)
    if torch.cuda.is_available():
        ad, bd = a.detach().cuda().requires_grad_(True), b.cuda()
        assert not spmm_mod._routable(ad, bd)
        assert spmm_mod._routable_grad(ad, bd)


def test_install_sparse_grad_flag():
    try:
        gcn_amd.install()
        assert not spmm_mod._route_sparse_grad
        gcn_amd.install(sparse_grad=True)
        assert spmm_mod._route_sparse_grad
    finally:
        gcn_amd.uninstall()
    assert not spmm_mod._route_sparse_grad
