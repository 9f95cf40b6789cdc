"""The class twin of tests/nonfinite_ref.py without a GPU: its classes equal those of a plain fp64 loop in several summation
orders and groupings; three wrong results built in numpy — a padding entry that multiplies a real row of B with 0, a ReLU that
answers 0 to a NaN (fmaxf), a bf16 rounding that carries a low-payload NaN into Inf — are each refused by the assertions
tests/test_nonfinite_gpu.py makes (nonfinite_ref.assert_contained); and the inputs of every case of that module meet the
twin's preconditions and can tell (assert_nonfinite_inputs)."""
import numpy as np
import pytest

import nonfinite_ref as nr
from nonfinite_ref import FINITE, NAN, NINF, PINF, ZERO
from util import EPILOGUES, exact_operands


def _loop(ops, B, order, split=False):
    """C = A.B row by row in fp64, the entries of a row added one at a time in the order `order` gives them (split: the two
    halves of a row summed apart, then added)"""
    m, k = ops["m"], B.shape[1]
    C = np.zeros((m, k))
    with np.errstate(invalid="ignore"):                  # (a signalling NaN raises the flag when it is widened, too)
        B64, va = B.astype(np.float64), ops["va"].astype(np.float64)
        for r in range(m):
            e = order(np.arange(ops["rp"][r], ops["rp"][r + 1]))
            parts = [e[:len(e) // 2], e[len(e) // 2:]] if split else [e]
            sums = []
            for part in parts:
                acc = np.zeros(k)
                for q in part:
                    acc = acc + va[q] * B64[ops["ci"][q]]
                sums.append(acc)
            C[r] = sums[0] if len(sums) == 1 else sums[0] + sums[1]
    return C


@pytest.mark.parametrize("kind", ["int", "pow2"])
def test_twin_equals_a_plain_fp64_loop_in_any_order(kind):
    d = nr.nonfinite_inputs("unsliced", kind, 4)
    ops, Bp = d["ops"], d["Bp"]
    rng = np.random.default_rng(1)
    orders = [("stored", lambda e: e, False), ("reversed", lambda e: e[::-1], False), ("shuffled", rng.permutation, False),
              ("shuffled halves", rng.permutation, True)]
    for name, order, split in orders:
        C = _loop(ops, Bp, order, split)
        got = nr.class_of(C)
        got[got == ZERO] = FINITE
        assert np.array_equal(got, d["cls"]), (kind, name)
        assert np.array_equal(~np.isfinite(C), d["touched"]), (kind, name)
    print(kind, d["report"])


def _refused(Cp, Cc, cls, touched, what, **kw):
    with pytest.raises(AssertionError) as info:
        nr.assert_contained(Cp, Cc, cls, touched, what, **kw)
    print(f"mutant refused: {info.value}")
    return str(info.value)


def _results(d):
    """a correct fp32 result pair for a case, from the fp64 product"""
    ops = d["ops"]
    import scipy.sparse as sp
    A = sp.csr_matrix((ops["va"].astype(np.float64), ops["ci"], ops["rp"]), shape=(ops["m"], ops["n"]))
    Cc = (A @ d["B"].astype(np.float64)).astype(np.float32)
    Cp = Cc.copy()
    t, cls = d["touched"], d["cls"]
    Cp[t & (cls == NAN)], Cp[t & (cls == PINF)], Cp[t & (cls == NINF)] = np.nan, np.inf, -np.inf
    return Cp, Cc


def test_three_mutants_are_each_refused():
    d = nr.nonfinite_inputs("group_dup", "pow2", 64, 3)
    ops, cls, touched = d["ops"], d["cls"], d["touched"]
    Cp, Cc = _results(d)
    nr.assert_contained(Cp, Cc, cls, touched, "the correct result")
    # 1. a padding entry (value 0) behind the rows whose length is no multiple of 16 gathers row 0 of B, not the zero row
    ragged = (np.diff(ops["rp"]) % 16 != 0)[:, None]
    with np.errstate(invalid="ignore"):
        leak = np.where(ragged, Cp + np.float32(0) * d["Bp"][0][None, :], Cp).astype(np.float32)
    assert not np.isfinite(d["Bp"][0]).all()
    assert "untouched elements changed" in _refused(leak, Cc, cls, touched, "0 * Inf through a padding entry")
    # 2. the ReLU as fmaxf(x, 0): NaN -> 0
    relu_cls = nr.apply_epilogue(cls, relu=True)
    good = np.where(np.isnan(Cp), Cp, np.maximum(Cp, np.float32(0)))
    nr.assert_contained(good, np.maximum(Cc, np.float32(0)), relu_cls, touched, "ReLU that keeps NaN")
    assert "wrong class" in _refused(np.fmax(Cp, np.float32(0)), np.maximum(Cc, np.float32(0)), relu_cls, touched, "fmaxf ReLU")
    # 3. bf16 by adding 0x7FFF + lsb to the bits, a NaN not set apart: payload 1 carries into the exponent's neighbour, +Inf
    def bf16_bits(x, nan_safe):
        u = x.view(np.uint32).astype(np.uint64)
        r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
        return np.where(np.isnan(x), np.uint16(0x7FC0), r) if nan_safe else r
    low = Cp.copy()
    low.view(np.int32)[np.isnan(Cp)] = nr.SNAN_BITS
    assert np.isnan(low).sum() == np.isnan(Cp).sum() > 0
    widen = lambda h: (h.astype(np.uint32) << 16).view(np.float32)
    for nan_safe in (True, False):
        hp, hc = bf16_bits(low, nan_safe), bf16_bits(Cc, True)
        args = (widen(hp), widen(hc), cls, touched, f"bf16 store, NaN set apart: {nan_safe}")
        if nan_safe:
            nr.assert_contained(*args, bits=(hp, hc), sentinel=0x7FC1)
        else:
            assert "wrong class" in _refused(*args, bits=(hp, hc))


def test_epilogue_rules_and_the_sentinel():
    d = nr.nonfinite_inputs("group_dup", "int", 16, 3)
    cls, touched, m = d["cls"], d["touched"], d["ops"]["m"]
    keep = nr.keep_mask(m, 16)
    for e in EPILOGUES:
        got = nr.apply_epilogue(cls, d["bias"] if e.get("bias") else None, bool(e.get("relu")), keep if e.get("dropout") else None)
        assert np.all(got[touched & (cls == NAN) & (keep | (not e.get("dropout")))] == NAN), e      # ReLU keeps NaN
        assert np.all(got[touched & (cls == PINF) & (keep | (not e.get("dropout")))] == PINF), e
        want = ZERO if e.get("relu") else NINF
        assert np.all(got[touched & (cls == NINF) & (keep | (not e.get("dropout")))] == want), e
        if e.get("dropout"):
            assert np.all(got[~keep] == ZERO) and (touched & ~keep).any() and (touched & keep).any(), e
    Cp, Cc = _results(d)
    Cp.view(np.int32)[5, 5] = 0x7FC12345
    assert "not written" in _refused(Cp, Cc, cls, touched, "sentinel left", sentinel=0x7FC12345)
    Cc[7, 7] = np.nan
    assert "not finite" in _refused(Cp, Cc, cls, touched, "clean result not written")


def test_merged_entries_of_a_dense_tile():
    """the counts over a dense panel's tile: repeated entries summed, a zero sum skipped; outside the tile entry by entry"""
    rp, ci = np.array([0, 2, 4, 6, 6], np.int32), np.array([0, 0, 1, 1, 2, 2], np.int32)
    va = np.array([3, -1, 2, -2, 1, -1], np.float32)
    B = np.array([[np.inf], [np.inf], [np.inf]], np.float32)
    cls, touched = nr.spmm_class(rp, ci, va, B)
    assert cls[:, 0].tolist() == [NAN, NAN, NAN, FINITE] and touched[:, 0].tolist() == [True, True, True, False]
    merged = np.array([True, True, True, True, False, False])
    cls, touched = nr.spmm_class(rp, ci, va, B, merged=merged)
    assert cls[:, 0].tolist() == [PINF, FINITE, NAN, FINITE] and touched[:, 0].tolist() == [True, False, True, False]


_CASES = [(p, kd, k, S) for p, kd, widths, S in nr.NONFINITE_CASES for k in widths]


@pytest.mark.parametrize("pattern,kind,k,slices", _CASES, ids=[f"{p}-{kd}-k{k}-S{S}" for p, kd, k, S in _CASES])
def test_inputs_of_every_gpu_case_meet_the_preconditions(pattern, kind, k, slices):
    d = nr.nonfinite_inputs(pattern, kind, k, slices)          # (asserts them)
    print(pattern, kind, k, slices, d["report"], [(b, j, v, r) for b, j, v, r in d["placed"]])
    assert len(d["placed"]) >= 8 and d["touched"].any()
    if pattern == "mfma":
        assert d["dense"] >= 10 and d["merged"].any()
    if kind == "pow2":
        assert np.all(d["ops"]["u_row"] > 0) and np.all(d["ops"]["u_col"] > 0)


def test_every_epilogue_case_of_the_gpu_module_is_among_the_checked_inputs():
    from exact_plans import EPI_CASES, epilogue_slices, smallest_epilogue_cases
    picked = smallest_epilogue_cases()
    covered = {(p, kd, k, S) for p, kd, k, S in _CASES}
    for cid, carrier, pattern, kind, k, opt in picked:
        assert (pattern, kind, k, epilogue_slices(pattern, opt)) in covered, cid
    families = {(c[1], c[2], c[3], tuple(sorted(c[5].items()))) for c in EPI_CASES}
    assert families == {(c[1], c[2], c[3], tuple(sorted(c[5].items()))) for c in picked}        # no family left out
    assert {c[0] for c in EPI_CASES if c[4] > 256} <= {c[0] for c in picked}


def test_inputs_of_the_transposed_dropin_and_heads_cases():
    for pattern, kind, k, S in nr.TRANSPOSED_CASES:
        d = nr.nonfinite_inputs(pattern, kind, k, S, transpose=True)
        ops, src = d["ops"], exact_operands(pattern, kind)
        assert (ops["m"], ops["n"]) == (src["n"], src["m"]) and len(ops["ci"]) == len(src["ci"])      # repeated entries kept
        assert np.all(np.diff(ops["ci"])[np.diff(np.repeat(np.arange(ops["m"]), np.diff(ops["rp"]))) == 0] >= 0)
    d = nr.dropin_inputs()
    print("dropin", d["report"])
    h = nr.heads_inputs()
    assert h["touched"].sum() >= 2
