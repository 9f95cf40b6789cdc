"""The two checks of tests/test_exact_gpu.py, without a GPU: every input generator that file uses meets the exactness
precondition (leg 1) and a plain fp32 reference (oracle/spmm_oracle.c, spmm_oracle_f32: sequential fp32 sums) passes the
element-wise bound on the wide-range operands (leg 2); and the reason both exist: a result with one product missing from
a small-scale element passes the suite's 1e-5 matrix-wide metric and fails the element-wise bound, and the exact
comparison refuses an entry that is off by 2^-6.  The fused epilogue's cases (util.EXACT_EPILOGUE_CASES) get the same, with
the bias and the dropout scale in the precondition, and the proof that their inputs discriminate: results with one step of
the epilogue missing or out of order, built in numpy, are each refused by assert_exact on these very inputs."""
import numpy as np
import pytest

from util import (EPILOGUE_NINE_SLICES, EPILOGUES, EXACT_CASES, EXACT_EPILOGUE_CASES, WIDE_CASES, assert_elementwise, assert_exact,
                  assert_exact_inputs, dropout_keep, elementwise_ratio, epilogue_inputs, epilogue_reference, exact_operands,
                  int_features, oracle_spmm, rel_err, spmm_references, sym_norm_graph, wide_features, EPILOGUE_DROPOUT)


@pytest.mark.parametrize("pattern,kind,widths", EXACT_CASES, ids=[f"{c[0]}-{c[1]}" for c in EXACT_CASES])
def test_exact_generators_meet_the_precondition_and_the_fp32_reference_is_exact(pattern, kind, widths):
    ops = exact_operands(pattern, kind)
    k = widths[-1] if len(ops["ci"]) < 10 ** 6 else widths[0]     # (the widest where that is cheap)
    B = int_features(ops["n"], k, seed=k)
    lhs, longest = assert_exact_inputs(ops["rp"], ops["ci"], ops["va"], B)
    print(f"{pattern}/{kind}: max |A|.|B| * 2^g = {lhs:.0f} < 2^24, longest row {longest}")
    lens = np.diff(ops["rp"])
    assert (lens == 0).any() or "diag" in pattern
    if kind == "int":
        assert np.all(ops["va"] != 0) and np.all(np.abs(ops["va"]) <= 4) and np.all(ops["va"] == np.rint(ops["va"]))
    else:
        assert np.all(np.isin(ops["va"], 2.0 ** -np.arange(7)))
    Cref = oracle_spmm(ops["rp"], ops["ci"], ops["va"], B)
    assert_exact(oracle_spmm(ops["rp"], ops["ci"], ops["va"], B, fp64=False), Cref, (pattern, kind))
    assert np.all(Cref[lens == 0] == 0)
    # any order: the entries of every row reversed, the same values
    rows = np.repeat(np.arange(ops["m"]), lens)
    rev = np.lexsort((-np.arange(len(rows)), rows))
    assert_exact(oracle_spmm(ops["rp"], ops["ci"][rev], ops["va"][rev], B, fp64=False), Cref, (pattern, kind, "reversed"))


@pytest.mark.parametrize("pattern,kind,widths", WIDE_CASES, ids=[f"{c[0]}-{c[1]}" for c in WIDE_CASES])
def test_fp32_reference_passes_the_elementwise_bound_on_the_wide_range_generators(pattern, kind, widths):
    ops = exact_operands(pattern, kind)
    k = widths[-1] if len(ops["ci"]) < 10 ** 6 else widths[0]
    B = wide_features(ops["n"], k, seed=k)
    tiny = np.finfo(np.float32).tiny
    assert np.all(np.abs(B[B != 0]) >= tiny * 2.0 ** 40) and np.all(np.abs(ops["va"][ops["va"] != 0]) >= tiny * 2.0 ** 40)
    bias = (np.random.default_rng(k).standard_normal(k) * 2.0 ** np.random.default_rng(k + 1).integers(-12, 13, k)).astype(np.float32)
    Cref, mag = spmm_references(ops["rp"], ops["ci"], ops["va"], B)
    C = oracle_spmm(ops["rp"], ops["ci"], ops["va"], B, fp64=False)
    ratio = assert_elementwise(C, Cref, mag, ops["rp"], (pattern, kind))
    assert ratio <= 0.5                                       # room without tuning
    Ce = np.maximum(C + bias[None, :], np.float32(0))
    Eref, emag = spmm_references(ops["rp"], ops["ci"], ops["va"], B, bias=bias, relu=True)
    assert_elementwise(Ce, Eref, emag, ops["rp"], (pattern, kind, "bias+relu"))
    assert np.all(Ce[np.diff(ops["rp"]) == 0] == np.maximum(bias, 0))


def test_one_dropped_product_passes_the_matrix_wide_metric_and_fails_the_elementwise_bound():
    """the gap: max|C - C*| / max|C*| <= 1e-5 tests an element only against the LARGEST entry of C"""
    n, k = 6000, 41
    rp, ci, va = sym_norm_graph(n, 260000, seed=3)
    B = wide_features(n, k, seed=3)
    Cref, mag = spmm_references(rp, ci, va, B)
    C = oracle_spmm(rp, ci, va, B, fp64=False)
    before = rel_err(C, Cref.astype(np.float32))
    ratio, _ = elementwise_ratio(C, Cref, mag, rp)
    assert before <= 1e-5 and ratio <= 1.0
    # the element with the smallest magnitude among the rows that hold entries; its largest product goes
    lens = np.diff(rp)
    cand = np.where(lens[:, None] > 1, mag, np.inf)
    i, j = np.unravel_index(int(np.argmin(cand)), cand.shape)
    e = np.arange(rp[i], rp[i + 1])
    prod = va[e].astype(np.float64) * B[ci[e], j].astype(np.float64)
    broken = C.copy()
    broken[i, j] = np.float32(broken[i, j] - prod[np.argmax(np.abs(prod))])
    after = rel_err(broken, Cref.astype(np.float32))
    assert after <= 1e-5 and after == before                  # the old metric does not notice
    ratio, at = elementwise_ratio(broken, Cref, mag, rp)
    assert at == (i, j) and ratio > 1.0, (ratio, at)          # the new bound does
    with pytest.raises(AssertionError):
        assert_elementwise(broken, Cref, mag, rp, "one product dropped")


def test_exact_comparison_rejects_one_entry_off_by_one_granule():
    ops = exact_operands("group", "pow2")
    B = int_features(ops["n"], 16, seed=1)
    assert_exact_inputs(ops["rp"], ops["ci"], ops["va"], B)
    Cref = oracle_spmm(ops["rp"], ops["ci"], ops["va"], B)
    assert_exact(Cref.copy(), Cref)
    neg_zero = Cref.copy()
    neg_zero[Cref == 0] = -0.0
    assert_exact(neg_zero, Cref)                              # values, not bit patterns
    i, j = np.unravel_index(int(np.argmax(np.abs(Cref))), Cref.shape)      # the largest entry: 2^-6 is still representable
    off = Cref.copy()
    off[i, j] += np.float32(2.0 ** -6)
    assert off[i, j] != Cref[i, j]
    with pytest.raises(AssertionError):
        assert_exact(off, Cref)


# ---------------------------------------------------------------------------------------------------------------
# the fused epilogue: dropout(act(A.B + bias)), p = 0.5 (scale 2), integer bias
def _rejected(mutant, ref32, what):
    """assert_exact refuses `mutant`; -> how many elements it changes"""
    mutant = np.asarray(mutant, np.float64).astype(np.float32)
    changed = int((mutant != ref32).sum())
    print(f"mutant {what}: {changed} of {ref32.size} elements differ")
    with pytest.raises(AssertionError):
        assert_exact(mutant, ref32, what)
    return changed


def _epilogue_case(ops, k):
    """inputs, precondition (with the bias and the factor 2) and both oracles of one width"""
    B, bias, keep = epilogue_inputs(ops["m"], ops["n"], k)
    lhs, longest = assert_exact_inputs(ops["rp"], ops["ci"], ops["va"], B, extra=bias, scale=2.0)
    C64 = oracle_spmm(ops["rp"], ops["ci"], ops["va"], B).astype(np.float64)
    C32 = oracle_spmm(ops["rp"], ops["ci"], ops["va"], B, fp64=False)
    assert 0.45 < keep.mean() < 0.55 and np.any(bias != 0)
    return B, bias, keep, C64, C32, lhs, longest


@pytest.mark.parametrize("pattern,kind,widths", EXACT_EPILOGUE_CASES, ids=[f"{c[0]}-{c[1]}" for c in EXACT_EPILOGUE_CASES])
def test_epilogue_inputs_meet_the_precondition_and_every_mutant_is_rejected(pattern, kind, widths):
    """The mutants.  ReLU commutes with the mask (relu(2z) = 2 relu(z), relu(0) = 0), so "mask before the ReLU" can only
    show with a bias between them: the mask applied to the sums, then bias and ReLU."""
    ops = exact_operands(pattern, kind)
    m, n, scale = ops["m"], ops["n"], 1.0 / (1.0 - EPILOGUE_DROPOUT[0])
    assert scale == 2.0
    k = widths[-1] if len(ops["ci"]) < 10 ** 6 else widths[0]
    B, bias, keep, C64, C32, lhs, longest = _epilogue_case(ops, k)
    print(f"{pattern}/{kind} k={k}: max (|A|.|B| + |bias|) * 2 * 2^g = {lhs:.0f} < 2^24, longest row {longest}")
    empty = np.diff(ops["rp"]) == 0
    assert empty.sum() >= 2
    f32 = np.float32
    for e in EPILOGUES:
        b, kp = (bias if e.get("bias") else None), (keep if e.get("dropout") else None)
        ref = epilogue_reference(C64, b, bool(e.get("relu")), kp, scale)
        assert np.array_equal(ref.astype(f32).astype(np.float64), ref), e        # an fp32 number: the conversion rounds nothing
        assert_exact(epilogue_reference(C32, b, bool(e.get("relu")), kp, scale).astype(f32), ref.astype(f32), (pattern, kind, e, "fp32 oracle"))
        Z = C32 + (bias[None, :] if e.get("bias") else f32(0))                   # ... and plain fp32 arithmetic gives it
        Z = np.maximum(Z, f32(0)) if e.get("relu") else Z
        Z = np.where(keep, f32(2) * Z, f32(0)) if e.get("dropout") else Z
        assert Z.dtype == f32
        assert_exact(Z, ref.astype(f32), (pattern, kind, e, "fp32 arithmetic"))
        want = np.broadcast_to(epilogue_reference(np.zeros((1, k)), b, bool(e.get("relu")), None, scale), (m, k))
        want = np.where(keep, scale * want, 0.0) if e.get("dropout") else want
        assert np.array_equal(ref[empty], want[empty])                           # empty rows: dropout(act(bias))
    br = epilogue_reference(C64, bias, True, None, scale).astype(f32)
    full = epilogue_reference(C64, bias, True, keep, scale).astype(f32)
    what = f"{pattern}/{kind} k={k}"
    assert _rejected(np.maximum(C64, 0.0) + bias[None, :], br, f"{what}: bias added after the ReLU") > 0
    assert _rejected(np.maximum(np.where(keep, scale * C64, 0.0) + bias[None, :], 0.0), full, f"{what}: mask before bias and ReLU") > 0
    off = epilogue_reference(C64, bias, True, keep, scale)
    off[empty] = np.maximum(bias, 0.0)[None, :]
    assert _rejected(off, full, f"{what}: mask left off the empty rows") > 0
    if ops["u_row"] is not None:                                                 # value-free: (sum + bias) * u_row
        u = ops["u_row"].astype(np.float64)
        sums = C64 / u[:, None]                                                  # (a power of two: exact)
        assert np.array_equal(sums * u[:, None], C64)
        assert_exact(epilogue_reference(sums, bias, True, keep, scale, u_row=u).astype(f32), full, "row factor in the reference")
        tell = (u != 1.0)[:, None] & (bias != 0)[None, :] & keep
        assert tell.sum() > 0
        print(f"{what}: {int(tell.sum())} kept elements with u_row != 1 and bias != 0")
        assert _rejected((sums + bias[None, :]) * u[:, None], epilogue_reference(C64, bias, False, None, scale).astype(f32),
                         f"{what}: row factor after the bias") > 0
        assert _rejected(np.where(keep, scale * np.maximum((sums + bias[None, :]) * u[:, None], 0.0), 0.0), full,
                         f"{what}: row factor after the bias, whole epilogue") > 0
    for ko in [w for w in widths if w % 4 != 0]:                                 # the mask indexed with k_run = ceil(k / 4) * 4
        _B, bo, ko_keep, Co, _C32, _l, _r = _epilogue_case(ops, ko)
        k_run = (ko + 3) // 4 * 4
        p, seed, offset = EPILOGUE_DROPOUT
        wrong = dropout_keep(m * k_run, p, seed, offset).reshape(m, k_run)[:, :ko]
        assert np.array_equal(wrong[0], ko_keep[0]) and not np.array_equal(wrong[1], ko_keep[1])
        assert _rejected(epilogue_reference(Co, bo, True, wrong, scale), epilogue_reference(Co, bo, True, ko_keep, scale).astype(f32),
                         f"{pattern}/{kind} k={ko}: mask with a row stride of {k_run}") > 0
    if pattern in EPILOGUE_NINE_SLICES:                                          # the ninth slice's partial row dropped
        k9 = EPILOGUE_NINE_SLICES[pattern][-1]
        B9, b9, keep9, C9, _C32, _l, _r = _epilogue_case(ops, k9)
        w = (n + 8) // 9
        rows = np.repeat(np.arange(m), np.diff(ops["rp"]))
        part = []
        for sel in (ops["ci"] < 8 * w, ops["ci"] >= 8 * w):                      # slices 0..7, slice 8
            rp = np.zeros(m + 1, np.int64)
            rp[1:] = np.cumsum(np.bincount(rows[sel], minlength=m))
            part.append(oracle_spmm(rp.astype(np.int32), ops["ci"][sel], ops["va"][sel], B9).astype(np.float64))
        assert np.array_equal(part[0] + part[1], C9) and np.any(part[1] != 0)
        assert _rejected(epilogue_reference(part[0], b9, True, keep9, scale), epilogue_reference(C9, b9, True, keep9, scale).astype(f32),
                         f"{pattern}/{kind} k={k9}: the ninth slice's partial row dropped") > 0
