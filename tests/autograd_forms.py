"""The autograd contract, as a harness: an op's result and gradients are fixed once by a canonical call, and every other legal
way of calling it must give the same bits, every illegal way a clear error ("The autograd contract").

An op is an ``Op``: a name, ``make(seed) -> (operands, g)`` (the operand tensors and the upstream gradient, all on the op's
device), ``call(*operands)``, the indices of the differentiable operands, and optionally ``mutate()`` (changes the values of
the mutable adjacency the op runs on and returns a callable that puts them back) and ``share`` (two operand indices that may
be one leaf).  The canonical call: every operand a fresh contiguous leaf, every differentiable one with requires_grad, one
``torch.autograd.grad(out, operands, g)`` with a contiguous ``g``.  Each form below runs the op another way and compares
with the canonical call by ``torch.equal``; a form is a function ``form(op, seed=0)`` that raises AssertionError.

This module imports no GPU code and runs on any device: tests/test_autograd_forms_cpu.py runs it on torch-only twins with
planted defects, tests/test_autograd_forms_gpu.py on every autograd Function of gcn_amd."""
import itertools

import torch


class Op:
    def __init__(self, name, make, call, diff=None, mutate=None, share=None):
        self.name, self.make, self.call, self.mutate, self.share = name, make, call, mutate, share
        self._diff = diff
        self._canon = {}

    def diff(self, operands):
        return tuple(range(len(operands))) if self._diff is None else tuple(self._diff)

    def __repr__(self):
        return f"Op({self.name})"


# ---- the canonical call ---------------------------------------------------------------------------------------------------------
def leaves_of(op, operands, subset=None):
    """fresh contiguous leaves; those of `subset` (default: every differentiable operand) require grad"""
    want = op.diff(operands) if subset is None else subset
    return [t.detach().clone(memory_format=torch.contiguous_format).requires_grad_(i in want) for i, t in enumerate(operands)]


def run(op, operands, g):
    """(out, {operand index: gradient}) of the canonical call on these operands; the output is a copy"""
    leaves = leaves_of(op, operands)
    out = op.call(*leaves)
    idx = op.diff(operands)
    grads = torch.autograd.grad(out, [leaves[i] for i in idx], g.contiguous())
    return out.detach().clone(), {i: gr.detach().clone() for i, gr in zip(idx, grads)}


def canonical(op, seed=0):
    """(operands, g, out, grads) of the canonical call for make(seed): computed once per op and seed and left alone"""
    if seed not in op._canon:
        operands, g = op.make(seed)
        operands, g = [t.detach() for t in operands], g.detach().contiguous()
        op._canon[seed] = (operands, g) + run(op, operands, g)
    return op._canon[seed]


def same(got, want, what):
    assert got is not None, f"{what}: no gradient arrived"
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {tuple(got.shape)} {got.dtype}, want {tuple(want.shape)} {want.dtype}"
    assert torch.equal(got, want), f"{what}: not the bits of the canonical call"


# ---- 1. every subset of operands requiring grad ---------------------------------------------------------------------------------
def form_subsets(op, seed=0):
    operands, g, out, grads = canonical(op, seed)
    idx = op.diff(operands)
    for r in range(len(idx) + 1):
        for subset in itertools.combinations(idx, r):
            leaves = leaves_of(op, operands, subset)
            got = op.call(*leaves)
            what = f"{op.name}, grad for operands {subset}"
            same(got.detach(), out, what + ": output")
            if not subset:
                assert not got.requires_grad, f"{what}: the output of constants requires grad"
                continue
            got.backward(g)
            for i, leaf in enumerate(leaves):
                if i in subset:
                    same(leaf.grad, grads[i], f"{what}: gradient {i}")
                else:
                    assert leaf.grad is None, f"{what}: operand {i} is a constant and got a gradient"


# ---- 2. strided operands --------------------------------------------------------------------------------------------------------
def _junk(t):
    """values a correct op never reads: they differ from t's (almost) everywhere"""
    return (-t.float() - 1).to(t.dtype)


def _transposed(t):
    if t.dim() != 2:
        return _second(t)
    base = t.t().contiguous().detach().requires_grad_(True)
    return base, base.t(), lambda gr: gr.t()


def _columns(t):
    if t.dim() != 2:
        return _second(t)
    k = t.shape[1]
    base = _junk(t[:, :1]).expand(t.shape[0], k + 3).contiguous()
    base[:, 1:1 + k] = t
    base.requires_grad_(True)

    def scatter(gr):
        z = torch.zeros_like(base)
        z[:, 1:1 + k] = gr
        return z
    return base, base[:, 1:1 + k], scatter


def _second(t):
    """every second row of a [2 rows, k] tensor / every second element of a 2 len tensor"""
    base = torch.stack([t, _junk(t)], 1).reshape((2 * t.shape[0],) + tuple(t.shape[1:])).contiguous()
    base.requires_grad_(True)

    def scatter(gr):
        z = torch.zeros_like(base)
        z[::2] = gr
        return z
    return base, base[::2], scatter


STRIDED = {"transposed": _transposed, "columns": _columns, "every second": _second}


def _check_views(op, operands, g, out, grads, views, what):
    """views: {operand index: (base leaf, view, scatter)}; the other operands are contiguous leaves"""
    leaves = leaves_of(op, operands)
    args = [views[i][1] if i in views else leaf for i, leaf in enumerate(leaves)]
    for i in views:
        assert not args[i].is_contiguous() or args[i].numel() <= 1 or min(args[i].shape) <= 1, f"{what}: operand {i} came out contiguous"
        assert torch.equal(args[i].detach(), operands[i]), f"{what}: the view does not hold the operand"
    got = op.call(*args)
    same(got.detach(), out, what + ": output")
    idx = op.diff(operands)
    got.backward(g)
    for i in idx:
        if i in views:
            same(views[i][0].grad, views[i][2](grads[i]), f"{what}: gradient {i}, through the view")
        else:
            same(leaves[i].grad, grads[i], f"{what}: gradient {i}")


def form_strided_operands(op, seed=0):
    operands, g, out, grads = canonical(op, seed)
    for kind, build in STRIDED.items():
        for chosen in [(i,) for i in range(len(operands))] + [tuple(range(len(operands)))]:
            views = {i: build(operands[i]) for i in chosen}
            _check_views(op, operands, g, out, grads, views, f"{op.name}, operands {chosen} {kind}")
    # an expanded single row, in a case of its own: the reference is the materialised tensor
    for i in range(len(operands)):
        t = operands[i]
        row = t[:1].detach().clone()
        full = row.expand(t.shape).contiguous()
        ops2 = list(operands)
        ops2[i] = full
        out2, grads2 = run(op, ops2, g)
        base = row.clone().requires_grad_(True)
        views = {i: (base, base.expand(t.shape), lambda gr: gr.sum(0, keepdim=True))}
        _check_views(op, ops2, g, out2, grads2, views, f"{op.name}, operand {i} an expanded row")


# ---- 3. strided upstream gradients ----------------------------------------------------------------------------------------------
def form_strided_gradients(op, seed=0):
    operands, g, out, grads = canonical(op, seed)
    idx = op.diff(operands)
    if g.dim() == 2:
        wide = _junk(g[:, :1]).expand(g.shape[0], g.shape[1] + 3).contiguous()
        wide[:, 1:1 + g.shape[1]] = g
        forms = {"transposed storage": g.t().contiguous().t(), "a column slice": wide[:, 1:1 + g.shape[1]]}
    else:
        wide = _junk(g)[:, None].expand(g.shape[0], 3).contiguous()
        wide[:, 1] = g
        forms = {"every second element": torch.stack([g, _junk(g)], 1).reshape(-1)[::2], "a column slice": wide[:, 1]}
    for what, gv in forms.items():
        assert torch.equal(gv, g) and (not gv.is_contiguous() or min(g.shape) <= 1)
        leaves = leaves_of(op, operands)
        got = torch.autograd.grad(op.call(*leaves), [leaves[i] for i in idx], gv)
        for i, gr in zip(idx, got):
            same(gr, grads[i], f"{op.name}, g as {what}: gradient {i}")
    # out.sum().backward(): a stride-0 gradient, against the canonical call given ones
    _, ones_grads = run(op, operands, torch.ones_like(out))
    leaves = leaves_of(op, operands)
    op.call(*leaves).sum().backward()
    for i in idx:
        same(leaves[i].grad, ones_grads[i], f"{op.name}, out.sum().backward(): gradient {i}")


# ---- 4. repeated and shared use -------------------------------------------------------------------------------------------------
def form_repeated_and_shared(op, seed=0):
    operands, g, out, grads = canonical(op, seed)
    idx = op.diff(operands)
    # backward twice on one graph
    leaves = leaves_of(op, operands)
    got = op.call(*leaves)
    got.backward(g, retain_graph=True)
    for i in idx:
        same(leaves[i].grad, grads[i], f"{op.name}, first backward: gradient {i}")
    got.backward(g)
    for i in idx:
        same(leaves[i].grad, grads[i] + grads[i], f"{op.name}, second backward: accumulated gradient {i}")
    # two consumers of the output
    leaves = leaves_of(op, operands)
    got = op.call(*leaves)
    both = torch.autograd.grad([got * 1.0, got * 1.0], [leaves[i] for i in idx], [g, g])
    for i, gr in zip(idx, both):
        same(gr, grads[i] + grads[i], f"{op.name}, two consumers: gradient {i}")
    # one leaf as two operands
    if op.share is not None:
        i, j = op.share
        ops2 = list(operands)
        ops2[j] = operands[i]
        out2, grads2 = run(op, ops2, g)
        leaves = leaves_of(op, ops2)
        leaves[j] = leaves[i]
        got = op.call(*leaves)
        same(got.detach(), out2, f"{op.name}, one leaf as operands {i} and {j}: output")
        got.backward(g)
        same(leaves[i].grad, grads2[i] + grads2[j], f"{op.name}, one leaf as operands {i} and {j}: the sum of the two gradients")
        for o in idx:
            if o not in (i, j):
                same(leaves[o].grad, grads2[o], f"{op.name}, one leaf as operands {i} and {j}: gradient {o}")


# ---- 5. earlier results survive later calls -------------------------------------------------------------------------------------
def form_later_calls(op, seed=0):
    operands, g, out, grads = canonical(op, seed)
    other, g_other = op.make(seed + 1)
    idx = op.diff(operands)
    leaves = leaves_of(op, operands)
    out1 = op.call(*leaves)
    kept = out1.detach().clone()
    leaves2 = leaves_of(op, other)
    op.call(*leaves2).backward(g_other)
    assert torch.equal(out1.detach(), kept), f"{op.name}: a later call changed an earlier result"
    same(kept, out, f"{op.name}: output")
    got = torch.autograd.grad(out1, [leaves[i] for i in idx], g)
    for i, gr in zip(idx, got):
        same(gr, grads[i], f"{op.name}, backward after a later call: gradient {i}")


# ---- 6. an operand changed in place between forward and backward ----------------------------------------------------------------
def form_inplace_change(op, seed=0):
    operands, g, out, grads = canonical(op, seed)
    idx = op.diff(operands)
    for c in range(len(operands)):
        changed = list(operands)
        changed[c] = -operands[c]
        _, grads_changed = run(op, changed, g)
        leaves = leaves_of(op, operands)
        got = op.call(*leaves)
        with torch.no_grad():
            leaves[c].neg_()
        try:
            res = torch.autograd.grad(got, [leaves[i] for i in idx], g)
        except RuntimeError:
            continue                                       # autograd's version check, or the op's own refusal
        for i, gr in zip(idx, res):
            if not torch.equal(gr, grads[i]):
                late = torch.equal(gr, grads_changed[i])
                raise AssertionError(f"{op.name}, operand {c} changed in place after the forward: gradient {i} is "
                                     + ("that of the CHANGED values" if late else "neither that of the forward's nor of the changed values"))


# ---- 7. the values of a mutable adjacency changed between forward and backward --------------------------------------------------
def form_mutated_adjacency(op, seed=0):
    if op.mutate is None:
        return
    operands, g, out, grads = canonical(op, seed)
    idx = op.diff(operands)
    leaves = leaves_of(op, operands)
    got = op.call(*leaves)
    undo = op.mutate()
    try:
        try:
            res = torch.autograd.grad(got, [leaves[i] for i in idx], g)
        except RuntimeError:
            return
    finally:
        if undo is not None:
            undo()
    for i, gr in zip(idx, res):
        same(gr, grads[i], f"{op.name}, adjacency values changed after the forward: gradient {i}")


# ---- 8. no_grad and inference_mode ----------------------------------------------------------------------------------------------
def form_no_graph(op, seed=0):
    operands, g, out, grads = canonical(op, seed)
    for name, ctx in (("no_grad", torch.no_grad), ("inference_mode", torch.inference_mode)):
        leaves = leaves_of(op, operands)
        with ctx():
            got = op.call(*leaves)
        assert not got.requires_grad and got.grad_fn is None, f"{op.name} under {name}: the output carries a graph"
        same(got, out, f"{op.name} under {name}: output")


# ---- 9. second differentiation is refused ---------------------------------------------------------------------------------------
def form_second_differentiation(op, seed=0):
    operands, g, out, grads = canonical(op, seed)
    idx = op.diff(operands)
    leaves = leaves_of(op, operands)
    loss = op.call(*leaves).float().square().sum()         # (quadratic: the upstream gradient itself has a graph)
    try:
        first = torch.autograd.grad(loss, [leaves[i] for i in idx], create_graph=True)
        (loss + sum(gr.float().square().sum() for gr in first)).backward()
    except RuntimeError as e:
        assert "twice" in str(e), f"{op.name}: second differentiation raised, but not the refusal: {e}"
        return
    raise AssertionError(f"{op.name}: a second differentiation went through in silence (its gradients carry no graph, or half of one)")


FORMS = {
    "1 subsets": form_subsets,
    "2 strided operands": form_strided_operands,
    "3 strided gradients": form_strided_gradients,
    "4 repeated and shared": form_repeated_and_shared,
    "5 later calls": form_later_calls,
    "6 in-place change": form_inplace_change,
    "7 mutated adjacency": form_mutated_adjacency,
    "8 no graph": form_no_graph,
    "9 second differentiation": form_second_differentiation,
}
