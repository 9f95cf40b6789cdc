"""The autograd contract (tests/autograd_forms.py, DESIGN "The autograd contract") on the two autograd Functions of
gcn_amd/edgefeat.py: the canonical call against fp64 autograd of the plain formulation, bit for bit on the integer grid, and
every form of tests/autograd_forms.py — subsets of operands that ask for a gradient, strided operands and gradients, repeated
and later calls, an operand changed in place between forward and backward, no_grad / inference_mode, a refused second
differentiation.  The specs are built with the Spec class, the "rect" pattern (a chunked row of the transposed pattern) and
the two test bodies of tests/test_autograd_forms_gpu.py, which stays as it is.

tests/test_autograd_forms_cpu.py checks that every autograd Function of the package is under the contract by reading that
module's SPECS; the specs of this file are entered there when this file is imported, as it is whenever the suite is collected.
(Run on its own, tests/test_autograd_forms_cpu.py does not see them.)"""
import importlib

import pytest
import torch

import gcn_amd
import test_autograd_forms_gpu as forms

_edgefeat = importlib.import_module("gcn_amd.edgefeat")
CASES = [("add", "relu", "sum", 5), ("mul", None, "sum", 64), ("mul", "relu", "max", 5), ("add", None, "min", 64)]


def ref_pick(P, E, reduce):
    """row-wise max / min of the messages E [nnz, k] with the kernel's tie rule — the lowest entry index — so that the
    gradient goes to that entry (test_autograd_forms_gpu.ref_select, on messages)"""
    row, _col = P.index(E.device)
    k = E.shape[1]
    key = -E.detach() if reduce == "min" else E.detach()
    ridx = row[:, None].expand(-1, k).contiguous()
    best = torch.full((P.m, k), float("-inf"), dtype=E.dtype, device=E.device).scatter_reduce(0, ridx, key, "amax")
    eidx = torch.arange(P.nnz, device=E.device)[:, None].expand(-1, k).contiguous()
    cand = torch.where(key == best[row], eidx, P.nnz)
    arg = torch.full((P.m, k), P.nnz, dtype=torch.int64, device=E.device).scatter_reduce(0, ridx, cand, "amin")
    picked = E[arg.clamp(max=P.nnz - 1), torch.arange(k, device=E.device)[None, :]]
    return torch.where(arg < P.nnz, picked, torch.zeros_like(picked))


def edge_specs():
    P = forms.pattern("rect")
    specs = []
    for op, act, reduce, k in CASES:
        name = f"edge_aggregate {op} {act or 'none'} {reduce} k={k}"

        # integers up to 8: a message is at most 64, a row or a column has fewer than 2^24 / 64 entries, so every sum is exact
        def make(seed, device, k=k):
            return ([forms.ints((P.n, k), 70 * seed + k, 8, device), forms.ints((P.nnz, k), 70 * seed + k + 1, 8, device)],
                    forms.ints((P.m, k), 70 * seed + k + 2, 8, device))

        def reference(x, w, op=op, act=act, reduce=reduce):
            row, col = P.index(x.device)
            msg = x[col] * w if op == "mul" else x[col] + w
            if act == "relu":
                msg = msg.relu()
            if reduce == "sum":
                return torch.zeros(P.m, x.shape[1], dtype=x.dtype, device=x.device).index_add(0, row, msg)
            return ref_pick(P, msg, reduce)

        def build(name=name, op=op, act=act, reduce=reduce):
            adj = P.adj(name)
            return (lambda x, w: gcn_amd.edge_aggregate(adj, x, w, op, act, reduce)), None
        fn = _edgefeat._SumFunction if reduce == "sum" else _edgefeat._SelectFunction
        specs.append(forms.Spec(name, [fn], make, reference, build))
    return specs


EDGE_SPECS = edge_specs()
EDGE_IDS = [s.name.replace(" ", "_") for s in EDGE_SPECS]
if not any(s.name == EDGE_SPECS[0].name for s in forms.SPECS):
    forms.SPECS = forms.SPECS + EDGE_SPECS                 # (a new list: that module's own parametrisation keeps its own)


@pytest.mark.gpu
@pytest.mark.parametrize("spec", EDGE_SPECS, ids=EDGE_IDS)
def test_the_canonical_call_matches_fp64_autograd_of_the_plain_formulation(spec):
    forms.test_the_canonical_call_matches_fp64_autograd_of_the_plain_formulation(spec)


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(forms.af.FORMS), ids=[f.replace(" ", "_") for f in forms.af.FORMS])
@pytest.mark.parametrize("spec", EDGE_SPECS, ids=EDGE_IDS)
def test_every_form_gives_the_canonical_bits_or_a_clear_error(spec, form):
    forms.test_every_form_gives_the_canonical_bits_or_a_clear_error(spec, form)


def test_both_functions_are_entered_where_the_coverage_check_reads():
    covered = {f"{f.__module__}.{f.__name__}" for s in forms.SPECS for f in s.functions}
    assert {"gcn_amd.edgefeat._SumFunction", "gcn_amd.edgefeat._SelectFunction"} <= covered
