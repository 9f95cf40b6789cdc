"""The cases of tests/large_ref.py, proven without a GPU: the feat twin is the same in numpy and in torch, dropout_keep_at
is dropout_keep at chosen indices, every touched row above a threshold has alias rows with other content, and every
truncation mutant of every case is refused by what tests/test_large_operands_gpu.py compares."""
import numpy as np
import pytest
import torch

import large_ref as lr
from stress_units import BOUNDS
from test_dropout_mask_gpu import STREAMS
from util import dropout_keep, dropout_keep_at

NAMES = sorted(lr.CASES)


def test_feat_is_the_same_in_numpy_and_torch_and_exact_in_bf16():
    rows = np.concatenate([np.arange(0, 70), np.arange(2 ** 22 - 40, 2 ** 22 + 70), np.arange(2 ** 25, 2 ** 25 + 64)]).astype(np.int64)
    for k, salt in ((512, 0), (513, 7), (64, 3)):
        a = lr.feat(rows[:, None], np.arange(k, dtype=np.int64)[None, :], salt)
        b = lr.feat(torch.from_numpy(rows)[:, None], torch.arange(k, dtype=torch.int64)[None, :], salt)
        assert a.dtype == np.int64 and b.dtype == torch.int64 and np.array_equal(a, b.numpy())
        assert a.min() == -8 and a.max() == 8 and len(np.unique(a)) == 17
        assert np.array_equal(torch.from_numpy(a).to(torch.bfloat16).double().numpy(), a.astype(np.float64))
        assert np.array_equal(a, lr.feat_rows(rows, k, salt))
        assert abs(a.mean()) < 0.1                        # (no value is favoured: sums stay small)


@pytest.mark.parametrize("seed,offset", STREAMS)
def test_dropout_keep_at_is_dropout_keep(seed, offset):
    for p in (0.5, 0.3, 0.999):
        want = dropout_keep(4096, p, seed, offset)
        assert np.array_equal(dropout_keep_at(np.arange(4096), p, seed, offset), want)
        pick = np.array([[4095, 0], [17, 4093]])
        assert np.array_equal(dropout_keep_at(pick, p, seed, offset), want[pick])
    hi = np.array([2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 34 + 2], np.uint64)    # counter word 1 is the index's high part
    assert not np.array_equal(dropout_keep_at(np.arange(2 ** 32, 2 ** 32 + 256), 0.5, seed, offset),
                              dropout_keep_at(np.arange(256), 0.5, seed, offset))
    assert dropout_keep_at(hi, 0.5, seed, offset).shape == (4,)


def test_thresholds_and_bands():
    assert lr.rows_for("E32", 512, 4) == 2 ** 23 + 64 < 2 ** 24
    assert lr.rows_for("E31", 512, 4) == 2 ** 22 + 64 and lr.rows_for("B32", 512, 4) == 2 ** 21 + 64
    b = lr.bands(2 ** 23 + 64, 512, (2,))                # bf16 at E32: B32 and E31 fall on one row
    assert [x[1:] for x in b] == [(0, 64), (2 ** 22 - 32, 2 ** 22 + 32), (2 ** 22 - 32, 2 ** 22 + 32), (2 ** 23 - 32, 2 ** 23 + 32),
                                  (2 ** 23, 2 ** 23 + 64)]
    assert lr.truncate(np.array([2 ** 31 + 5]), "elem_i32", 4, 2 ** 32)[0] == 0
    assert lr.truncate(np.array([2 ** 32 + 5]), "elem_u32", 4, 2 ** 33)[0] == 5
    assert lr.truncate(np.array([2 ** 30 + 5]), "byte_u32", 4, 2 ** 33)[0] == 5
    assert lr.truncate(np.array([2 ** 31 + 5]), "byte_u32", 2, 2 ** 33)[0] == 5


@pytest.mark.parametrize("name", NAMES)
def test_case_shape(name):
    """the operand is the smallest that reaches its threshold, every band is there, and the rows have the lengths asked for"""
    c = lr.build(name)
    s = lr.ITEMSIZE[c["dtype"]]
    assert c["R"] == lr.rows_for(c["thr"], c["k"], s) and (c["R"] < 2 ** 24 or c["unit"] == "gat_softmax")
    assert (c["R"] - 1) * c["k"] * (s if c["thr"] == "B32" else 1) >= lr.LIMIT[c["thr"]]
    assert c["R"] * c["k"] * max(lr.itemsizes(c)) <= 17 * 2 ** 30
    bs = lr.bands(c["R"], c["k"], lr.itemsizes(c))
    assert len(bs) >= 3 and bs[-1][1:] == (c["R"] - 64, c["R"])
    if "rp" not in c:
        return
    if c["unit"] == "prelaid":                            # no tiny graph: the value-free pass exists from 48 entries per column
        assert len(c["ci"]) // c["n"] >= 48 and c["R"] == c["slices"] * (c["w"] + 1) and c["R"] * c["k"] * 4 >= 2 ** 32
        t = c["ci"].astype(np.int64) + c["ci"] // c["w"]
        for r in c["check_rows"]:                         # every compared row reads every band of the table
            tr = t[c["rp"][r]:c["rp"][r + 1]]
            assert all(((tr >= lo) & (tr < hi)).sum() >= 8 for _, lo, hi in bs) and (tr * c["k"] * 4 >= 2 ** 32).any()
        assert np.array_equal(c["va"], c["u_row"][np.repeat(np.arange(c["m"]), np.diff(c["rp"]))] * c["u_col"][c["ci"]])
        return
    lens = np.diff(c["rp"])
    assert len(c["ci"]) < 200000 and lens.max() == c["long"]
    # (the plan's chunks for the SpMM; sddmm's and the row-gather engine's largest bounds, stress_units.BOUNDS)
    assert c["long"] > (2 * lr.CHUNK_NNZ if c["unit"] in ("spmm", "spmm_backward") else max(BOUNDS["sddmm"]) if c["unit"] == "sddmm"
                         else 1024 if c["unit"] in ("sddmm_heads", "gatv2") else max(BOUNDS["attention" if c["unit"] == "gat_softmax" else "aggregate"]))
    if c["n"] == c["R"]:                                  # the big side is gathered (or is the gradient): every band is pointed at
        assert c["ci"].max() == c["R"] - 1 and c["ci"].min() == 0
        for _, lo, hi in bs:
            hit = (c["ci"] >= lo) & (c["ci"] < hi)
            rows_of = np.repeat(np.arange(c["m"]), lens)[hit]
            assert len(np.unique(c["ci"][hit])) == hi - lo and lens[rows_of].max() == c["long"] and lens[rows_of].min() <= 5
    else:                                                 # the big side is stored: every band holds every row length
        assert np.all(lens[:c["R"]][np.setdiff1d(np.arange(0, c["R"], 4099), c["touched"])] == 0)
        assert int(lens.sum()) == int(lens[c["touched"]].sum())
        for _, lo, hi in bs:
            got = set(int(x) for x in lens[lo:hi])
            assert {0, 1, 64, c["long"]} <= got, (name, lo)
        assert (lens[c["R"] - 1] > 0 or c["R"] % 32) and lens[0] == 0


@pytest.mark.parametrize("name", NAMES)
def test_alias_rows_differ(name):
    """a touched row above a threshold and the row its truncated offset lands in hold different content (gather side), or
    have different expected results (store side: the alias row holds what the unit defines for it, the true row its own)"""
    c = lr.build(name)
    k, s, rows = c["k"], lr.ITEMSIZE[c["dtype"]], c["touched"]
    checked = 0
    for kind in lr.MUTANTS[c["thr"]]:
        alias = lr.truncate(rows * k, kind, s, c["numel"]) // k
        moved = alias != rows
        assert moved.any(), (name, kind)
        assert np.all(rows[moved] >= min(lr.threshold_rows(c["R"], k, lr.itemsizes(c)).values()))
        if c["side"] in ("in", "A") and (not c["unit"].endswith("backward") or c["unit"] == "gatv2_backward"):   # (gathered)
            content = (lambda rr: lr.table_content(c, rr[:, None] * k + np.arange(k)[None, :])) if c["unit"] == "prelaid" \
                else (lambda rr: lr.feat_rows(rr, k, c["salt"]))
            same = np.all(content(rows[moved]) == content(alias[moved]), axis=1)
            assert not same.any(), (name, kind, rows[moved][same])
        checked += int(moved.sum())
    assert checked >= 32                                  # (at least the upper half of a straddling band)


@pytest.mark.parametrize("name", NAMES)
def test_mutants_are_refused(name):
    truth = lr.twin(name)
    for key, a in truth.items():
        assert np.all(np.isfinite(a)) and np.abs(a).max() > 0, (name, key)     # (no fill left, and something to compare)
    muts = lr.mutants(name)
    assert len(muts) >= len(lr.MUTANTS[lr.CASES[name]["thr"]])
    for label, kw in muts:
        assert lr.differs(truth, lr.twin(name, **kw)), f"{name}: the mutant {label} gives what the truth gives"
    assert not lr.differs(truth, lr.twin(name))
    if lr.CASES[name]["unit"] == "gat_softmax":           # compared within bounds of some 1e-5 relative: a mutant is far outside
        for label, kw in muts:
            other = lr.twin(name, **kw)
            gap = max(float(np.nanmax(np.abs(np.nan_to_num(other[key], nan=1e9) - truth[key]) / (np.abs(truth[key]) + 1e-3))) for key in truth)
            assert gap > 1e-2, (name, label, gap)


@pytest.mark.parametrize("name", [n for n in NAMES if lr.CASES[n]["side"] == "out" and "rp" in lr.build(n)])
def test_store_side_aliases_have_other_results(name):
    """on the output side a non-empty row's result differs from what its alias rows are to hold (an empty row's value
    outside the bands, the alias row's own result inside them)"""
    c = lr.build(name)
    truth = lr.twin(name)
    out = np.concatenate([truth[key] for key in sorted(truth)], axis=1)     # (an aggregation's result is its values and its arg)
    rows, k, s = c["touched"], c["k"], lr.ITEMSIZE[c["dtype"]]
    lens = np.diff(c["rp"])
    big_rows = c["R"]
    for kind in lr.MUTANTS[c["thr"]]:
        alias = lr.truncate(rows * k, kind, s, c["numel"]) // k
        for i in np.flatnonzero((alias != rows) & (lens[rows] > 0 if c["m"] == big_rows else True)):
            at = np.searchsorted(rows, alias[i])
            if at < len(rows) and rows[at] == alias[i]:
                assert not np.array_equal(out[i], out[at]), (name, kind, rows[i])
            elif not c.get("epilogue"):
                assert np.any(out[i] != 0), (name, kind, rows[i])


def test_exact_in_fp32():
    """every sum of a case is a multiple of 1/8 (the pre-laid case: of 1/64, its values are products of two powers of two
    down to 1/8) below 2^24 granules in magnitude, dropout's factor 2 included, so any order of additions is exact"""
    for name in NAMES:
        c = lr.build(name)
        if "rp" in c:
            g = 64 if c["unit"] == "prelaid" else 8
            assert int(np.diff(c["rp"]).max()) * 8 * g * 2 < 2 ** 24 and np.array_equal(c["va"] * g, np.rint(c["va"] * g))
