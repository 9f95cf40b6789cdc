"""The harness of tests/autograd_forms.py catches what it is for — no GPU needed.  Two torch-only twin Functions on the CPU,
written the way the gcn_amd wrappers are (detach().contiguous() operands, a contiguous gradient, needs_input_grad branches,
once_differentiable): a two-operand SDDMM-like op on a fixed square pattern and a three-operand op with a bias whose matrix
lives outside it, like the values of a mutable adjacency.  The correct twins pass every form; each planted defect fails its
own form and no other.  Inputs are small integers: every sum is exact, as on the GPU.

Also: the GPU file's ops cover every torch.autograd.Function defined under gcn_amd/ (but the drop-in flexspmm, which keeps the
reference's semantics), and its exact-grid ops have fp64 references that lie on the fp32 grid."""
import importlib
import inspect
import pkgutil

import pytest
import torch

import autograd_forms as af
from autograd_forms import FORMS, Op

once = torch.autograd.function.once_differentiable
M_ROWS, K = 6, 4
_gen = torch.Generator().manual_seed(5)
ROW = torch.randint(0, M_ROWS, (40,), generator=_gen).sort().values
COL = torch.randint(0, M_ROWS, (40,), generator=_gen)
STATE = {}                                                 # the three-operand twin's "adjacency": its matrix and its version


def _as_if_contiguous(t):
    """the defect of a dropped .contiguous(): the storage read with the strides of a contiguous tensor"""
    strides, acc = [], 1
    for s in reversed(t.shape):
        strides.insert(0, acc)
        acc *= s
    return t.as_strided(t.shape, strides, t.storage_offset())


def sddmm_twin(defect=None):
    """out[e] = <a[ROW[e]], b[COL[e]]>"""
    buf = torch.empty(len(ROW))

    class Twin(torch.autograd.Function):
        @staticmethod
        def forward(ctx, a, b):
            ad = _as_if_contiguous(a.detach()) if defect == "operand strides" else a.detach().contiguous()
            bd = b.detach().contiguous()
            if defect == "live operand":                   # (held outside save_for_backward: no version check guards it)
                ctx.save_for_backward(ad.clone(), bd.clone())
                ctx.live = a.detach()
            else:
                ctx.save_for_backward(ad, bd)
            if defect == "mutates saved":
                ctx.scratch = bd.clone()
            out = (ad[ROW] * bd[COL]).sum(1)
            if defect == "one buffer":
                buf.copy_(out)
                return buf.detach()
            return out

        @staticmethod
        @once
        def backward(ctx, g):
            ad, bd = ctx.saved_tensors
            g = _as_if_contiguous(g) if defect == "gradient strides" else g.contiguous()
            need_a, need_b = ctx.needs_input_grad
            frozen = need_a != need_b
            if defect == "none for the needed" and frozen:
                need_a, need_b = need_b, need_a
            if defect == "swapped slots" and frozen:
                need_a = need_b = True
            if defect == "live operand":
                ad = ctx.live.contiguous()
            if defect == "mutates saved":
                bd = ctx.scratch
            ga = torch.zeros_like(ad).index_add_(0, ROW, g[:, None] * bd[COL]) if need_a else None
            gb = torch.zeros_like(bd).index_add_(0, COL, g[:, None] * ad[ROW]) if need_b else None
            if defect == "mutates saved":
                ctx.scratch.mul_(2)
            if defect == "swapped slots" and frozen:
                return gb, ga
            return ga, gb

    def make(seed):
        gen = torch.Generator().manual_seed(100 + seed)
        a, b = (torch.randint(-3, 4, (M_ROWS, K), generator=gen).float() for _ in range(2))
        return [a, b], torch.randint(-3, 4, (len(ROW),), generator=gen).float()

    return Op(f"sddmm twin ({defect})", make, Twin.apply, share=(0, 1))


def bias_twin(defect=None):
    """out = M (x * s) + bias, M the matrix in STATE (changed by mutate(), as update_values changes an adjacency)"""
    class Twin(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, s, bias):
            xd, sd, bd = (t.detach().contiguous() for t in (x, s, bias))
            ctx.M, ctx.version = STATE["M"], STATE["version"]
            ctx.save_for_backward(xd, sd)
            return ctx.M @ (xd * sd) + bd

        @staticmethod
        def _backward(ctx, g):
            xd, sd = ctx.saved_tensors
            if defect == "current values":
                M = STATE["M"]
            else:
                if ctx.version != STATE["version"]:
                    raise RuntimeError("the matrix changed between forward and backward")
                M = ctx.M
            if defect == "unmarked":
                with torch.no_grad():                      # (a raw kernel call: its result carries no graph)
                    t = M.t() @ g.detach().contiguous()
                    gx, gs = t * sd, (t * xd).sum(0)
                return gx, gs, g.sum(0)                    # ... and one torch op that does
            g = g.contiguous()
            t = M.t() @ g
            return (t * sd if ctx.needs_input_grad[0] else None, (t * xd).sum(0) if ctx.needs_input_grad[1] else None,
                    g.sum(0) if ctx.needs_input_grad[2] else None)

        backward = staticmethod(_backward.__func__ if defect == "unmarked" else once(_backward.__func__))

    def make(seed):
        gen = torch.Generator().manual_seed(200 + seed)
        x = torch.randint(-3, 4, (5, K), generator=gen).float()
        s, bias = (torch.randint(-3, 4, (K,), generator=gen).float() for _ in range(2))
        return [x, s, bias], torch.randint(-3, 4, (M_ROWS, K), generator=gen).float()

    def mutate():
        old = STATE["M"]
        STATE["M"], STATE["version"] = -old - 1, STATE["version"] + 1

        def undo():
            STATE["M"], STATE["version"] = old, STATE["version"] + 1
        return undo

    return Op(f"bias twin ({defect})", make, Twin.apply, mutate=mutate)


@pytest.fixture(autouse=True)
def _state():
    STATE["M"] = torch.randint(-3, 4, (M_ROWS, 5), generator=torch.Generator().manual_seed(9)).float()
    STATE["version"] = 0


def failing(op):
    out = []
    for name, form in FORMS.items():
        try:
            form(op)
        except (AssertionError, RuntimeError) as e:
            print(f"{op.name}: form {name}: {type(e).__name__}: {str(e)[:160]}")
            out.append(name)
    return out


@pytest.mark.parametrize("twin", [sddmm_twin, bias_twin])
def test_the_correct_twins_pass_every_form(twin):
    assert failing(twin()) == []


# one planted defect per form fails exactly that form
DEFECTS = [(sddmm_twin, "swapped slots", "1 subsets"), (sddmm_twin, "none for the needed", "1 subsets"),
           (sddmm_twin, "operand strides", "2 strided operands"), (sddmm_twin, "gradient strides", "3 strided gradients"),
           (sddmm_twin, "mutates saved", "4 repeated and shared"), (sddmm_twin, "one buffer", "5 later calls"),
           (sddmm_twin, "live operand", "6 in-place change"), (bias_twin, "current values", "7 mutated adjacency"),
           (bias_twin, "unmarked", "9 second differentiation")]


@pytest.mark.parametrize("twin,defect,form", DEFECTS, ids=[d[1] for d in DEFECTS])
def test_a_planted_defect_fails_its_own_form_and_no_other(twin, defect, form):
    assert failing(twin(defect)) == [form]


def test_the_in_place_form_accepts_the_version_check_and_the_forwards_values():
    """autograd's version check fires for a saved detach().contiguous() of a contiguous operand (a RuntimeError: accepted);
    a twin that saves copies returns the gradients of the forward's values (accepted too)"""
    op = sddmm_twin()
    operands, g = op.make(0)
    leaves = af.leaves_of(op, operands)
    out = op.call(*leaves)
    with torch.no_grad():
        leaves[0].neg_()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.backward(g)

    class Copies(torch.autograd.Function):
        @staticmethod
        def forward(ctx, a, b):
            ctx.save_for_backward(a.detach().clone(), b.detach().clone())
            return (a.detach()[ROW] * b.detach()[COL]).sum(1)

        @staticmethod
        @once
        def backward(ctx, g):
            ad, bd = ctx.saved_tensors
            return (torch.zeros_like(ad).index_add_(0, ROW, g[:, None] * bd[COL]),
                    torch.zeros_like(bd).index_add_(0, COL, g[:, None] * ad[ROW]))

    FORMS["6 in-place change"](Op("copies", op.make, Copies.apply))


def test_second_differentiation_unmarked_is_silent_and_marked_raises():
    for defect, silent in (("unmarked", True), (None, False)):
        op = bias_twin(defect)
        operands, _g = op.make(0)
        leaves = af.leaves_of(op, operands)
        loss = op.call(*leaves).square().sum()
        gx, gs, gb = torch.autograd.grad(loss, leaves, create_graph=True)
        if silent:
            assert not gx.requires_grad and gb.requires_grad       # half of a second derivative, and nothing says so
            (loss + gx.square().sum() + gb.square().sum()).backward()
        else:
            with pytest.raises(RuntimeError, match="differentiate twice"):
                (loss + gx.square().sum()).backward()


# ---- the GPU file covers every autograd Function of the package, and its grid is a grid ---------------------------------------
def _package_functions():
    import gcn_amd
    found = {}
    for info in pkgutil.walk_packages(gcn_amd.__path__, "gcn_amd."):
        mod = importlib.import_module(info.name)
        for name, obj in vars(mod).items():
            if (inspect.isclass(obj) and issubclass(obj, torch.autograd.Function) and obj is not torch.autograd.Function
                    and obj.__module__ == mod.__name__):
                found[f"{mod.__name__}.{name}"] = obj
    return found


def test_the_gpu_ops_cover_every_autograd_function_of_the_package():
    import test_autograd_forms_gpu as gpu
    found = _package_functions()
    print("\n".join(sorted(found)))
    assert "gcn_amd.dropin.flexspmm" in found and len(found) >= 13
    covered = set()
    for spec in gpu.SPECS:
        covered.update(f"{f.__module__}.{f.__name__}" for f in spec.functions)
    assert covered == set(found) - {"gcn_amd.dropin.flexspmm"}, sorted(set(found) ^ covered)
    for name, obj in found.items():
        if name != "gcn_amd.dropin.flexspmm":
            assert hasattr(obj.backward, "__wrapped__") or "once_differentiable" in inspect.getsource(obj), name


def test_the_patterns_hold_what_the_gpu_file_needs_of_them():
    import test_autograd_forms_gpu as gpu
    rect = gpu.pattern("rect")
    lens = rect.lens
    assert (rect.m, rect.n) == (60, 300) and list(lens[:10]) == gpu.RECT_LENS and not lens[-10:].any()
    assert int((rect.col == 3).sum()) > 4096 and rect.nnz < 16000
    square = gpu.pattern("square")
    assert square.m == square.n and square.nnz > 0
    pairs = set(zip(square.row.tolist(), square.col.tolist()))
    assert len(pairs) == square.nnz                        # (no repeated entry: a coalesced COO pattern)


def test_the_exact_grid_references_lie_on_the_fp32_grid():
    """the precondition of bit equality with fp64, checked on the GPU file's own inputs: every fp64 reference of an op that
    claims the grid — output and gradients — survives the cast to fp32 and back"""
    import test_autograd_forms_gpu as gpu
    checked = 0
    for spec in gpu.SPECS:
        if not spec.grid or spec.reference is None:
            continue
        for seed in (0, 1):
            operands, g = spec.make(seed, "cpu")
            out, grads = gpu.fp64_reference(spec, operands, g)
            for what, t in [("output", out)] + [(f"gradient {i}", gr) for i, gr in grads.items()]:
                assert torch.equal(t.float().double(), t), f"{spec.name} seed {seed}: the fp64 {what} is not on the fp32 grid"
                assert bool(t.abs().max() < 2 ** 24)
            checked += 1
    assert checked >= 40
