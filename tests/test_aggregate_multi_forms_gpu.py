"""The autograd contract (tests/autograd_forms.py) on gcn_amd.aggregate._MultiFunction, with the Spec class, the "rect" pattern
and the two test bodies of tests/test_autograd_forms_gpu.py: two specs on the integer grid (max | sum | min: exact in fp64) and
one on all six planes, held to the bounds of tests/test_aggregate_multi_gpu.py.  The specs are entered into that module's
SPECS on import, where tests/test_autograd_forms_cpu.py reads them (as tests/test_edge_aggregate_forms_gpu.py does)."""
import importlib

import pytest
import torch

import gcn_amd
import test_aggregate_multi_gpu as multi
import test_autograd_forms_gpu as forms

_aggregate = importlib.import_module("gcn_amd.aggregate")


def anchor_all_planes(spec):
    P = forms.pattern("rect")
    (x,), g, out, grads = forms.af.canonical(spec.op())
    _out, argmax, argmin = gcn_amd.aggregate_multi(P.adj(spec.name), x, multi.ALL, multi.EPS, return_arg=True)
    multi.check_planes(out.cpu().numpy(), argmax, argmin, P.rowptr, multi.ref_rows(P.rowptr, P.col, x.cpu().numpy()), spec.name)
    ref, mag = (multi.ref_gradient(P.rowptr, P.col, P.n, x.cpu().double(), g.cpu(), argmax.cpu(), argmin.cpu(), magnitude)
                for magnitude in (False, True))
    excess = (grads[0].cpu().double() - ref).abs() - (1e-5 * mag + 1e-30)
    print(f"[forms] {spec.name} gradient: max |err| - bound = {excess.max():.3e}")
    assert excess.max() <= 0, float(excess.max())


def multi_specs():
    P = forms.pattern("rect")
    specs = []
    for k in (5, 64):                                      # integers up to 8: every sum of a row or a column is exact
        name = f"aggregate_multi max sum min k={k}"
        make = lambda seed, device, k=k: ([forms.ints((P.n, k), 80 * seed + k, 8, device)], forms.ints((P.m, 3 * k), 80 * seed + k + 1, 8, device))
        reference = lambda x: torch.cat([forms.ref_select(P, x, "max"), forms.ref_spmm(P, x, torch.ones(P.nnz, dtype=x.dtype, device=x.device)),
                                         forms.ref_select(P, x, "min")], 1)
        build = lambda name=name: ((lambda x, adj=P.adj(name): gcn_amd.aggregate_multi(adj, x, ("max", "sum", "min"))), None)
        specs.append(forms.Spec(name, [_aggregate._MultiFunction], make, reference, build))
    name = "aggregate_multi all planes k=8"
    make = lambda seed, device: ([forms.normal((P.n, 8), 90 + seed, device)], forms.normal((P.m, 48), 95 + seed, device))
    build = lambda: ((lambda x, adj=P.adj(name): gcn_amd.aggregate_multi(adj, x, multi.ALL, multi.EPS)), None)
    specs.append(forms.Spec(name, [_aggregate._MultiFunction], make, None, build, grid=False, anchor=anchor_all_planes))
    return specs


MULTI_SPECS = multi_specs()
MULTI_IDS = [s.name.replace(" ", "_") for s in MULTI_SPECS]
if not any(s.name == MULTI_SPECS[0].name for s in forms.SPECS):
    forms.SPECS = forms.SPECS + MULTI_SPECS                # (a new list: that module's own parametrisation keeps its own)


@pytest.mark.gpu
@pytest.mark.parametrize("spec", MULTI_SPECS, ids=MULTI_IDS)
def test_the_canonical_call_matches_fp64_autograd_of_the_plain_formulation(spec):
    forms.test_the_canonical_call_matches_fp64_autograd_of_the_plain_formulation(spec)


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(forms.af.FORMS), ids=[f.replace(" ", "_") for f in forms.af.FORMS])
@pytest.mark.parametrize("spec", MULTI_SPECS, ids=MULTI_IDS)
def test_every_form_gives_the_canonical_bits_or_a_clear_error(spec, form):
    forms.test_every_form_gives_the_canonical_bits_or_a_clear_error(spec, form)

