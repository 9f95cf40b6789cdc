"""The autograd contract (tests/autograd_forms.py) on gcn_amd.aggregate._QuantileFunction, with the Spec class, the "rect"
pattern and the two test bodies of tests/test_autograd_forms_gpu.py: one spec on the integer grid, three quantiles side by
side.  The plain formulation picks x[col[arg]] with arg from tests/quantile_ref.py, so its gradient goes to the same entry.
The spec is entered into that module's SPECS on import, where tests/test_autograd_forms_cpu.py reads it (as
tests/test_aggregate_multi_forms_gpu.py does)."""
import importlib

import pytest
import torch

import gcn_amd
import test_autograd_forms_gpu as forms
from quantile_ref import quantile_ref

_aggregate = importlib.import_module("gcn_amd.aggregate")
Q, K = (0.25, 0.5, 0.75), 5
P = forms.pattern("rect")


def reference(x):
    _out, arg = quantile_ref(P.rowptr, P.col, x.detach().cpu().float().numpy(), Q)
    arg = torch.from_numpy(arg).long().to(x.device)
    picked = x[P.index(x.device)[1][arg.clamp(min=0)], torch.arange(K, device=x.device).repeat(len(Q))]
    return torch.where(arg >= 0, picked, torch.zeros_like(picked))


NAME = f"aggregate_quantile quartiles k={K}"
SPEC = forms.Spec(NAME, [_aggregate._QuantileFunction],
                  lambda seed, device: ([forms.ints((P.n, K), 70 * seed + K, 8, device)], forms.ints((P.m, len(Q) * K), 70 * seed + K + 1, 8, device)),
                  reference, lambda: ((lambda x, adj=P.adj(NAME): gcn_amd.aggregate_quantile(adj, x, Q)), None))
if not any(s.name == NAME for s in forms.SPECS):
    forms.SPECS = forms.SPECS + [SPEC]                     # (a new list: that module's own parametrisation keeps its own)


@pytest.mark.gpu
def test_the_canonical_call_matches_fp64_autograd_of_the_plain_formulation():
    forms.test_the_canonical_call_matches_fp64_autograd_of_the_plain_formulation(SPEC)


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(forms.af.FORMS), ids=[f.replace(" ", "_") for f in forms.af.FORMS])
def test_every_form_gives_the_canonical_bits_or_a_clear_error(form):
    forms.test_every_form_gives_the_canonical_bits_or_a_clear_error(SPEC, form)
