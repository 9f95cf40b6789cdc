"""Seeded sweep of the drop-in pair on the GPU: the cases of tests/stress_dropin.py (their coverage, their power to discriminate
and csr2tile's packing of every one of them are proven without a GPU in tests/test_stress_dropin_cpu.py).  A seed packs once
and then runs, ON THE SAME DEVICE BUFFERS, three flexspmm steps at widths narrow, wide, narrow, one cuspmm on the unpacked
CSR and one permutate; B and C sit 0 .. 3 floats past a 16-byte boundary between guard elements, C is the zero matrix the
reference hands over.  Values and features are chosen so that every sum is exact in fp32 in any order: every result must
EQUAL the fp64 oracle.  When seed s is through, the first flexspmm step of seed s - 1 runs again on that seed's still-live
buffers and must give the same bits: the process-wide scratch plan has been regrown and reused in between, often by the
other format.  The symmetric seeds take one more step through dropin.flexspmm.apply with a gradient.  Everything runs on the
legacy default stream, as the symbols do; stderr holds a `libgcnspmm:` line only where a seed expects one (csr2tile refusing
seed 3, and flexspmm saying that nothing was packed).  No malformed buffer is offered to flexspmm."""
import ctypes

import numpy as np
import pytest
import torch

import stress_dropin as sd
from gcn_amd import _lib, dropin
from util import assert_exact, elementwise_bound, guards_intact, int_features, offset_view, oracle_spmm, spmm_references

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_LIVE = {}                                             # seed -> the packed buffers on the device and step 0's operands and bits


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().copy()


def _upload(c):
    """csr2tile on the host (inside guards), the buffers shrunk as gcn6.py:353-354 shrinks them and copied to the device"""
    out = sd.pack(c["rp"], c["ci"], c["va"], c["m"], c["n"])
    ns = out["n_segs"]
    assert out["guards"] and ns == c["n_segs"], (sd.describe(c, 0), ns)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return dict(n_segs=ns, seg_rowPtr=dev(out["seg_rowPtr"][:max(9 * ns, 1)]), segNzCV=dev(out["segNzCV"]),
                segVoMap=dev(out["segVoMap"][:max(8 * ns, 1)]), tail=dev(out["tail"]), next=dev(out["next"]))


def _flexspmm(c, live, B, C):
    nxt = live["next"].clone()                           # (a fresh copy per call: gcn6.py:38)
    _lib.load().flexspmm(_vp(live["seg_rowPtr"]), _vp(live["segNzCV"]), _vp(live["segVoMap"]), _vp(live["tail"]), _vp(nxt),
                         c["m"], c["n"], B.shape[1], live["n_segs"], _vp(B), _vp(C))
    torch.cuda.synchronize()


def _operands(c, i, rows):
    """(B at its offset, a zero C at its offset, their guarded buffers)"""
    s = c["steps"][i]
    X = sd.features(c, i)
    B, b_flat = offset_view(X, s["off_b"], torch.float32, DEV)
    C, c_flat = offset_view((rows, s["k"]), s["off_c"], torch.float32, DEV)
    C.zero_()
    return X, B, b_flat, C, c_flat


def _first_step(c, live):
    """step 0 of a seed on its buffers -> (C as numpy, its bits)"""
    X, B, b_flat, C, c_flat = _operands(c, 0, c["m"])
    _flexspmm(c, live, B, C)
    what = sd.describe(c, 0)
    assert guards_intact(b_flat, B) and guards_intact(c_flat, C), what + ": a guard was written"
    assert np.array_equal(B.cpu().numpy(), X), what + ": B was written"
    return C.cpu().numpy(), _bits(C)


def _prepare(seed):
    """the seed's buffers on the device and its first step's bits (kept until the next seed has run)"""
    if seed not in _LIVE:
        c = sd.case(seed)
        live = _upload(c)
        live["C0"], live["bits0"] = _first_step(c, live)
        _LIVE[seed] = live
    return _LIVE[seed]


@pytest.mark.parametrize("seed", range(sd.SEEDS))
def test_dropin_sweep(seed, capfd):
    prev = seed - 1 if seed > 0 else None
    if prev is not None:
        _prepare(prev)                                   # (live already when the sweep runs in order)
    capfd.readouterr()
    c = sd.case(seed)
    m, n, nnz = c["m"], c["n"], c["nnz"]
    want = sd.twin(c)
    live = _prepare(seed)
    refused = c["n_segs"] == 0
    assert_exact(live["C0"], want[0], sd.describe(c, 0))
    for i in (1, 2):
        what = sd.describe(c, i)
        X, B, b_flat, C, c_flat = _operands(c, i, m)
        _flexspmm(c, live, B, C)
        assert guards_intact(b_flat, B) and guards_intact(c_flat, C), what + ": a guard was written"
        assert np.array_equal(B.cpu().numpy(), X), what + ": B was written"
        got = C.cpu().numpy()
        assert_exact(got, want[i], what)
        assert np.all(got[c["lens"] == 0] == 0.0), what
    # cuspmm on the unpacked CSR
    what = sd.describe(c, 3)
    rp, ci, va = (torch.from_numpy(a).to(DEV) for a in (c["rp"], c["ci"], c["va"]))
    X, B, b_flat, C, c_flat = _operands(c, 3, m)
    dropin.cuspmm(rp, ci, va, B, C, m, n, nnz, c["steps"][3]["k"])
    torch.cuda.synchronize()
    assert guards_intact(b_flat, B) and guards_intact(c_flat, C), what + ": a guard was written"
    assert_exact(C.cpu().numpy(), want[3], what)
    # permutate, in place
    what, s = sd.describe(c, 4), c["steps"][4]
    X, B, b_flat, _, _ = _operands(c, 4, 1)
    vo = torch.from_numpy(s["perm"]).to(DEV)
    labels = torch.arange(n, dtype=torch.int32, device=DEV)
    dropin.permutate(B, vo, labels, m, n, s["k"])
    torch.cuda.synchronize()
    assert guards_intact(b_flat, B), what + ": a guard was written"
    assert_exact(B.cpu().numpy(), want[4], what)
    assert torch.equal(labels, torch.arange(n, dtype=torch.int32, device=DEV)), what
    if c["symmetric"]:                                   # backward = the same op on the gradient: valid because A = A^T
        what, s = sd.describe(c, 5), c["steps"][5]
        x = int_features(n, s["k"], seed=s["feat"] + 500)
        inp = torch.from_numpy(x).to(DEV).requires_grad_(True)
        out = dropin.flexspmm.apply(live["seg_rowPtr"], live["segNzCV"], live["segVoMap"], m, n, live["n_segs"], live["tail"], live["next"], inp)
        assert_exact(out.detach().cpu().numpy(), oracle_spmm(c["rp"], c["ci"], c["va"], x), what + " forward")
        out.backward(torch.from_numpy(sd.features(c, 5)).to(DEV))
        torch.cuda.synchronize()
        assert_exact(inp.grad.cpu().numpy(), want[5], what + " grad == oracle(A^T, g)")
    # the previous seed's first step again, on its own buffers: the same bits as before this seed regrew the scratch
    lines = 4 if refused else 0
    if prev is not None:
        p = sd.case(prev)
        _, again = _first_step(p, _LIVE[prev])
        assert np.array_equal(again, _LIVE[prev]["bits0"]), f"{sd.describe(p, 0)}: other bits after {sd.describe(c, 0)}"
        lines += 1 if p["n_segs"] == 0 else 0
        del _LIVE[prev]
        sd.forget(prev)
    err = capfd.readouterr().err
    assert err.count("libgcnspmm:") == lines, err
    if refused:
        assert err.count("libgcnspmm: csr2tile:") == 1 and err.count("libgcnspmm: flexspmm: n_segs=0") == lines - 1, err
    if seed == sd.SEEDS - 1:
        _LIVE.clear()
        sd.forget(seed)


def test_the_four_ulp_rule_on_the_device(capfd):
    """(e) one entry of a factoring group-format graph 2 ulp off u[r] * u[c]: csr2tile's rule (values_factor: 4.8e-7 * |v| per
    entry) still calls the values factors, the kernels multiply u[r] * u[c] in its place, and the result is held to the
    project's rounding bound plus the rule's own constant summed over the row, 4.8e-7 * (|A| . |B|).  16 ulp off, the values
    travel beside the stream and the result is exact again."""
    figures = []
    for ulps in (2, 16):
        c = sd.ulp_case(ulps)
        n = c["n"]
        live = _upload(c)
        assert (live["n_segs"] & 1) == (1 if ulps == 2 else 0) and c["layout"] is not None
        for k in (5, 64):
            X = int_features(n, k, seed=9000 + k)
            B, b_flat = offset_view(X, 1, torch.float32, DEV)
            C, c_flat = offset_view((n, k), 3, torch.float32, DEV)
            C.zero_()
            _flexspmm(c, live, B, C)
            assert guards_intact(b_flat, B) and guards_intact(c_flat, C)
            got = C.cpu().numpy()
            ref, mag = spmm_references(c["rp"], c["ci"], c["va"], X)
            err = np.abs(got.astype(np.float64) - ref)
            r = c["moved"][0]
            figures.append(f"ulps {ulps} k {k}: max |C - C*| {err.max():.3e} (row {int(err.max(1).argmax())}), in the moved row {err[r].max():.3e}")
            print(figures[-1])
            if ulps == 2:
                bound = elementwise_bound(c["rp"], mag) + 4.8e-7 * mag
                assert np.all(err <= bound), f"ulps 2 k {k}: exceeded by {(err - bound).max():.3e}"
                assert np.array_equal(np.delete(got, r, 0), np.delete(ref, r, 0).astype(np.float32))     # every other row: exact
            else:
                assert_exact(got, ref.astype(np.float32), f"ulps 16 k {k}")
    assert "libgcnspmm:" not in capfd.readouterr().err
    print("\n".join(figures))
    sd.forget(18)
