"""The dropout mask against its contract (include/gcn_spmm.h), not against itself: element i is kept iff word i % 4 of
Philox4x32-10 with counter (i / 4, offset) and key seed is >= p * 2^32.  The reference is util.dropout_keep (numpy,
pinned to the Random123 known-answer vectors by test_philox_ref.py); every carrier of the mask is compared with it: the
standalone pass (gcn_dropout_f32 / gcn_dropout_bf16: vec4 and scalar paths, chosen by pointer alignment and count % 4),
the in-place pass behind an unsliced SpMM, the three slice reductions, and the bf16 hot path with an fp32 and a bf16 C.

Not covered on the device: the high counter word (i / 4 >= 2^32) needs at least 2^34 elements — 64 GiB of fp32 — which
no test of seconds reaches.  The CPU reference covers its arithmetic (test_philox_ref.py)."""
import numpy as np
import pytest
import torch

import gcn_amd
from util import dropout_keep, dropout_threshold, guards_intact, offset_view, philox4x32_10, sym_norm_graph

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

COUNTS = (1, 2, 3, 4, 5, 1023, 1024, 4097, 65536)
P_BELOW_ONE = float(np.nextafter(np.float32(1), np.float32(0)))
PS = (2.0 ** -33, 2.0 ** -32, 0.3, 0.5, 0.999, P_BELOW_ONE)
STREAMS = ((0, 0), (42, 7), (0x9E3779B97F4A7C15, 2 ** 40 + 3), (2 ** 32, 2 ** 32), (2 ** 64 - 1, 2 ** 64 - 1))
CARRIER = (0.3, 0x9E3779B97F4A7C15, 2 ** 40 + 3)


def _scale(p):
    return 1.0 / (1.0 - float(np.float32(p)))           # fp64, from the float32 the ABI receives


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _input(count, dtype):
    g = torch.Generator(device="cpu")
    g.manual_seed(count)
    x = torch.randn(count, generator=g)
    x[::5] = -x[::5].abs()                               # negatives for certain
    if count >= 3:
        x[2::7] = 0.0                                    # exact zeros (kept or dropped: 0 either way)
    return x.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("count", COUNTS)
def test_standalone_pass_matches_the_philox_contract(count, dtype):
    x_cpu = _input(count, dtype)
    rel = 2.0 ** -23 if dtype == torch.float32 else 2.0 ** -8
    srcs = {o: offset_view(x_cpu, o, dtype, DEV) for o in (0, 1)}
    src_bits = _bits(srcs[0][0]).clone()
    xd = srcs[0][0].double()
    for p in PS:
        s = _scale(p)
        want = xd * s
        tol = want.abs() * rel
        for seed, offset in STREAMS:
            keep = torch.from_numpy(dropout_keep(count, p, seed, offset)).to(DEV)
            first = None
            for so in (0, 1):
                src, src_flat = srcs[so]
                for do in (0, 1):
                    dst, dst_flat = offset_view((count,), do, dtype, DEV)
                    gcn_amd.dropout_rows(src, p, seed, offset, out=dst)
                    where = (count, p, hex(seed), hex(offset), so, do)
                    assert bool(torch.all(_bits(dst)[~keep] == 0)), where          # dropped: +0.0, and nothing else is
                    got = dst.double()
                    assert bool(torch.all(((got - want).abs() <= tol)[keep])), where
                    assert bool(torch.all((got != 0)[keep & (xd != 0)])), where
                    assert guards_intact(dst_flat, dst) and guards_intact(src_flat, src), where
                    assert torch.equal(_bits(src), src_bits), where
                    if first is None:
                        first = _bits(dst).clone()
                    else:                                # vec4 and scalar paths: the same bits whatever the pointers
                        assert torch.equal(_bits(dst), first), where
            for o in (0, 1):                             # in place
                buf, buf_flat = offset_view(x_cpu, o, dtype, DEV)
                gcn_amd.dropout_rows(buf, p, seed, offset, out=buf)
                assert torch.equal(_bits(buf), first), (count, p, hex(seed), hex(offset), "in place", o)
                assert guards_intact(buf_flat, buf)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_a_word_equal_to_the_threshold_is_kept(dtype):
    """keep iff word >= threshold: the equality itself.  Any word below 2^24 is a threshold some float32 p gives exactly
    (p = word * 2^-32), and one in 256 words is that small: take the first such element of a stream, make its word the
    threshold, and it must be kept — on the vec4 path (count % 4 == 0, aligned) and on the scalar one."""
    seed, offset = 42, 7
    j = np.arange(1024, dtype=np.uint64)
    words = np.stack(philox4x32_10((j, 0, offset, 0), (seed, 0)), axis=1).reshape(-1)
    i = int(np.flatnonzero((words > 0) & (words < 2 ** 24))[0])
    p = float(words[i]) * 2.0 ** -32
    assert float(np.float32(p)) == p and dropout_threshold(p) == int(words[i])
    for count, off in ((4096, 0), (4096, 1), (4095, 0)):
        keep = dropout_keep(count, p, seed, offset)
        assert keep[i] and not keep.all()                # (smaller words exist among 4095 others)
        x, _ = offset_view(torch.ones(count), off, dtype, DEV)
        got = gcn_amd.dropout_rows(x, p, seed, offset)
        assert np.array_equal((got != 0).cpu().numpy(), keep), (count, off)


# ---- the mask through every carrier ----
_CACHE = {}


def _sym3000():
    if "sym" not in _CACHE:
        _CACHE["sym"] = sym_norm_graph(3000, 90000, seed=3)
    return _CACHE["sym"]


def _adj(rp, ci, va, n, **kw):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return gcn_amd.CsrAdjacency(t(rp), t(ci), t(va), (n, n), symmetric=True, **kw)


def _plan3000(slices):
    """one plan per slice count for the whole module"""
    if ("plan", slices) not in _CACHE:
        _CACHE["plan", slices] = _adj(*_sym3000(), 3000, slices=slices)
    return _CACHE["plan", slices]


def _check_carrier(adj, B, k, out_off=0, out_dtype=torch.float32):
    """Cd == 0 exactly where ~keep | (C0 == 0); kept values within 1e-6 * max|want| of C0 * s (fp32 C)"""
    m = adj.m
    p, seed, offset = CARRIER
    g = torch.Generator(device="cpu")
    g.manual_seed(k)
    bias = (torch.randn(k, generator=g) * 0.1).to(DEV)
    C0 = adj.matmul_raw(B, out=torch.empty((m, k), dtype=torch.float32, device=DEV), bias=bias, relu=True)
    assert 0.05 < float((C0 == 0).float().mean()) < 0.95                # ReLU leaves zeros of its own
    out, flat = offset_view((m, k), out_off, torch.float32, DEV)
    Cd = adj.matmul_raw(B, out=out, bias=bias, relu=True, dropout=(p, seed, offset))
    assert Cd.data_ptr() == out.data_ptr() and guards_intact(flat, out)
    keep = torch.from_numpy(dropout_keep(m * k, p, seed, offset).reshape(m, k)).to(DEV)
    assert torch.equal(Cd == 0, ~keep | (C0 == 0)), "dropped set differs from the Philox contract"
    want = C0.double() * _scale(p)
    err = float(((Cd.double() - want).abs() * keep).max())
    assert err <= 1e-6 * float(want.abs().max()), err
    if out_dtype == torch.bfloat16:                      # a bf16 C is that fp32 result rounded once: the same set
        out16, flat16 = offset_view((m, k), out_off, torch.bfloat16, DEV)
        C16 = adj.matmul_raw(B, out=out16, bias=bias, relu=True, dropout=(p, seed, offset))
        assert guards_intact(flat16, out16)
        assert torch.equal(_bits(C16), _bits(Cd.to(torch.bfloat16)))
        assert torch.equal(C16 == 0, ~keep | (C0 == 0))


def _features(n, k, dtype=torch.float32):
    g = torch.Generator(device="cpu")
    g.manual_seed(1000 + k)
    return torch.randn((n, k), generator=g).to(device=DEV, dtype=dtype)


@pytest.mark.parametrize("k", [64, 41])
def test_mask_behind_an_unsliced_spmm(k):
    """no epilogue pass to carry it: launch_dropout in place on C (k = 41: count % 4 != 0 -> the scalar path)"""
    adj = _plan3000(0)
    assert adj.num_slices == 0
    _check_carrier(adj, _features(3000, k), k)


@pytest.mark.parametrize("k,out_off", [(64, 0), (128, 0), (512, 0), (64, 1)],
                         ids=["wide-64", "wide-128", "reduce4-512", "reduce1-64-out+1"])
def test_mask_in_the_slice_reductions(k, out_off):
    """k <= 256: slice_reduce_wide_kernel; k = 512: slice_reduce_kernel<4>; C at a 1-float offset: <1>"""
    adj = _plan3000(8)
    assert adj.num_slices == 8
    _check_carrier(adj, _features(3000, k), k, out_off=out_off)


def test_mask_on_the_bf16_hot_path():
    """the bf16 group walk: slice_reduce (fp32 C) and slice_reduce_bf16_kernel (bf16 C) carry the mask"""
    rp, ci, va = sym_norm_graph(4000, 120000, seed=3)    # the plan of test_bf16_gpu.test_epilogue_bias_relu_dropout
    adj = _adj(rp, ci, va, 4000, slices=4)
    assert adj.main_kernel(128, dtype=torch.bfloat16).startswith("gcn::spmm_group_bf16")
    _check_carrier(adj, _features(4000, 128, torch.bfloat16), 128, out_dtype=torch.bfloat16)
