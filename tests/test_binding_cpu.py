"""The binding layer without a GPU: `_lib.call`, the one way a module makes a C-ABI call — status checked
under the function's own name, None as a null pointer, unknown names and wrong argument counts refused before the library
is entered — and a static check that no module has gone back to spelling the call sequence out."""
import ctypes
import glob
import os
import re

import pytest

import gcn_amd
from gcn_amd import _lib

INVALID = 1                                            # GCN_ERR_INVALID_ARG
PKG = os.path.dirname(os.path.abspath(gcn_amd.__file__))


def test_a_refused_call_raises_under_the_functions_own_name_with_its_status():
    need = ctypes.c_size_t(0)
    assert _lib.call("gcn_heads_ws_bytes", 0, 8, 2, 8, ctypes.byref(need)) is None and need.value > 0
    with pytest.raises(gcn_amd.GcnAmdError) as e:
        _lib.call("gcn_heads_ws_bytes", 0, 8, 0, 8, ctypes.byref(need))                # heads = 0
    assert str(e.value).startswith("gcn_heads_ws_bytes: ") and e.value.status == INVALID
    with pytest.raises(gcn_amd.GcnAmdError) as e:
        _lib.call("gcn_gatv2_ws_bytes", 4, 8, 2, 7, ctypes.byref(need))                # k no multiple of heads
    assert str(e.value).startswith("gcn_gatv2_ws_bytes: ") and e.value.status == INVALID


def test_none_arrives_as_a_null_pointer():
    need = ctypes.c_size_t(0)
    _lib.call("gcn_gatv2_ws_bytes", 4, 8, 2, 8, ctypes.byref(need))                    # fine with somewhere to write
    with pytest.raises(gcn_amd.GcnAmdError) as e:
        _lib.call("gcn_gatv2_ws_bytes", 4, 8, 2, 8, None)                              # refused for the null result pointer alone
    assert e.value.status == INVALID
    # an empty problem is legal with every pointer null, the stream included: None must not arrive as anything else
    assert _lib.call("gcn_segment_sum_csr_f32", None, 4, 0, None, None, None, None, 0, None) is None


def test_an_unknown_name_raises():
    with pytest.raises(gcn_amd.GcnAmdError, match="gcn_no_such_function"):
        _lib.call("gcn_no_such_function", 1, 2)
    with pytest.raises(gcn_amd.GcnAmdError):
        _lib.call("printf", b"not ours\n")             # (the process has it, include/gcn_spmm.h does not)


@pytest.mark.parametrize("args", [(0, 8, 2, 8), (0, 8, 2, 8, None, None)])
def test_a_wrong_argument_count_raises_and_does_not_enter_the_library(args, monkeypatch):
    _lib.call("gcn_heads_ws_bytes", 0, 8, 2, 8, ctypes.byref(ctypes.c_size_t(0)))      # (resolved: the table has its entry)
    entered = []
    _fn, nargs = _lib._calls["gcn_heads_ws_bytes"]
    monkeypatch.setitem(_lib._calls, "gcn_heads_ws_bytes", (lambda *a: entered.append(a) or 0, nargs))
    with pytest.raises((ctypes.ArgumentError, TypeError)):
        _lib.call("gcn_heads_ws_bytes", *args)
    assert not entered
    _lib.call("gcn_heads_ws_bytes", 0, 8, 2, 8, None)                                  # (the stand-in is what call enters)
    assert len(entered) == 1


# the direct calls that stay: getters whose return value is a figure, not a status, and the host-array entry points of
# reorder.py (numpy arrays, no device, no stream)
DIRECT = {
    "spmm.py": {"gcn_spmm_plan_num_chunks", "gcn_spmm_plan_chunk_nnz", "gcn_spmm_plan_panel_rows", "gcn_spmm_plan_dense_panels",
                "gcn_spmm_plan_panel_coverage", "gcn_spmm_plan_has_value_factors", "gcn_spmm_plan_num_slices",
                "gcn_spmm_plan_narrow_slices", "gcn_spmm_plan_num_passes", "gcn_spmm_plan_values_mutable"},
    "reorder.py": {"gcn_order_deg", "gcn_order_rcm", "gcn_order_gorder", "gcn_csr_apply_rank", "gcn_order_rabbit"},
}


def test_no_module_spells_the_call_sequence_out():
    """every other C-ABI call of the package goes through _lib.call (dist.py apart: its exchange calls pass raw peer
    addresses).  A new feature that writes `lib.gcn_x(...)` again fails here"""
    pattern = re.compile(r"(?:lib|load\(\))\.(gcn_\w+)\(")
    found = {}
    for path in sorted(glob.glob(os.path.join(PKG, "*.py"))):
        name = os.path.basename(path)
        if name in ("dist.py", "_lib.py"):
            continue
        with open(path) as f:
            hits = set(pattern.findall(f.read()))
        if hits:
            found[name] = hits
    assert found == DIRECT
    for names in DIRECT.values():
        assert names <= set(_lib.SIGNATURES)
