"""The two checks of tests/test_exact_gpu.py, without a GPU: every input generator that file uses meets the exactness
precondition (leg 1) and a plain fp32 reference (oracle/spmm_oracle.c, spmm_oracle_f32: sequential fp32 sums) passes the
element-wise bound on the wide-range operands (leg 2); and the reason both exist: a result with one product missing from
a small-scale element passes the suite's 1e-5 matrix-wide metric and fails the element-wise bound, and the exact
comparison refuses an entry that is off by 2^-6."""
import numpy as np
import pytest

from util import (EXACT_CASES, WIDE_CASES, assert_elementwise, assert_exact, assert_exact_inputs, elementwise_ratio,
                  exact_operands, int_features, oracle_spmm, rel_err, spmm_references, sym_norm_graph, wide_features)


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
