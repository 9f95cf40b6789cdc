"""The seeded sweep of tests/stress_dropin.py is sound, and csr2tile packs every one of its matrices exactly — checked on the
host, with no GPU.  Coverage is asserted over the whole seed range (SEEDS = 24: 16 small plain-format seeds, 2 across the
chunk-size step, 6 at the group format's smallest shapes); the packer runs on every seed inside guarded buffers of the
capacities gcn6.py:334-339 gives them; the twins depend on what lies past every bound a case claims and on the last feature
column.  The three argument checks of csr2tile (rows bounded by m, columns by n) are here too."""
import numpy as np
import pytest

import stress_dropin as sd
import stress_units as su
from gcn_amd import _lib
from test_abi import _check_group_format

ALL = range(sd.SEEDS)


def _cases():
    return [sd.case(s) for s in ALL]


def test_case_is_a_pure_function_of_the_seed():
    for seed in (1, 4, 7):
        a, b = sd._make(seed), sd._make(seed)
        assert all(np.array_equal(a[key], b[key]) for key in ("rp", "ci", "va"))
        assert sd.describe(a, 1) == sd.describe(b, 1) and f"seed {seed} " in sd.describe(a, 1)
        assert np.array_equal(sd.features(a, 0), sd.features(b, 0))


def test_the_rules_are_the_librarys():
    """the chunk-size step sits where 9 * n_segs reaches 2^20, the group rule at 9 * n_segs // m >= 128 and n * 256 > 4 MiB"""
    assert sd.dropin_T((2 ** 20 - 1) // 9) == 64 and sd.dropin_T((2 ** 20 + 8) // 9) == 128 and sd.dropin_T(2 ** 21 // 9 + 1) == 256
    f = _lib.load().gcn_spmm_auto_slices
    assert f(16385, 16385, 128 * 16385, 1) == 2 and f(16385, 16385, 128 * 16385 - 1, 1) == 0
    assert f(16384, 16384, 140 * 16384, 1) == 0 and f(32769, 32769, 128 * 32769, 1) == 4
    assert sd.QUAD_MIN_ROW == 48 and sd.GROUP_T == 512


def test_matrices_are_well_formed_and_every_sum_is_exact():
    entries = distinct = 0
    for c in _cases():
        m, n, rp, ci, va = c["m"], c["n"], c["rp"], c["ci"], c["va"]
        what = sd.describe(c, 0)
        assert rp[0] == 0 and rp[-1] == c["nnz"] == len(ci) == len(va) and len(rp) == m + 1 and np.all(np.diff(rp) >= 0), what
        assert ci.min() >= 0 and ci.max() < n, what
        if c["cls"] == "a":
            assert m <= 1500 and c["nnz"] <= sd.NNZ_MAX, what
        # exactness: |value| <= 4 (integers) or a multiple of 2^-6 up to 1, |feature| <= 8: with L entries in the longest row
        # (or column: the gradient step sums columns) every partial sum, in units of the granule, stays below 2^24
        longest = max(int(c["lens"].max()), int(np.bincount(ci, minlength=n).max()) if c["symmetric"] else 0)
        if c["factoring"]:
            assert np.array_equal(va * 64, np.rint(va * 64)) and np.all(va > 0) and va.max() <= 1, what
            assert longest * 8 * 64 < 2 ** 24, what             # granule 2^-6, |term| <= 8
            rows = np.repeat(np.arange(m), c["lens"])
            assert np.array_equal(np.unique(rows[rows == ci]), np.arange(m)), what      # a stored diagonal in every row
            assert np.array_equal(va, c["u"][rows] * c["u"][ci]), what
        else:
            assert np.array_equal(va, np.rint(va)) and np.abs(va).max() <= 4 and np.all(va != 0), what
            assert longest * 32 < 2 ** 24, what
        if c["symmetric"]:
            import scipy.sparse as sp
            A = sp.csr_matrix((va.astype(np.float64), ci, rp), shape=(m, n))
            assert m == n and abs(A - A.T).max() == 0, what
        rows = np.repeat(np.arange(m), c["lens"])
        key = rows.astype(np.int64) * n + ci
        srt = bool(np.all(np.diff(key) >= 0))
        assert srt == (not c["shuffled"]), what
        if c["cls"] == "a":                                     # a quarter of the entries is drawn as a repeat; rows of one or two
            entries, distinct = entries + len(key), distinct + len(np.unique(key))     # entries have none, a row longer than n more
            assert c["nnz"] // m < 8 or len(np.unique(key)) <= 0.9 * len(key), what
        for i, s in enumerate(c["steps"]):
            X = sd.features(c, i)
            assert np.array_equal(X, np.rint(X)) and np.abs(X).max() <= 8
    assert 0.2 <= 1.0 - distinct / entries <= 0.5, (distinct, entries)


def test_coverage_over_the_seed_range():
    cases = _cases()
    by = lambda **kw: [c for c in cases if all(c[k] == v for k, v in kw.items())]
    assert len(by(cls="a")) == 16 and len(by(cls="b")) == 2 and len(by(cls="c")) == 6 and len(cases) <= 24
    assert {c["format"] for c in cases} == {"plain", "group", "refused"}
    assert [c["seed"] for c in by(format="group")] == [18, 19, 20, 23] and [c["seed"] for c in by(format="refused")] == [3]
    packed = [c for c in cases if c["n_segs"] > 0]
    # both parities of n_segs and both outcomes of the parity step, crossed with every residue of nnz % 9
    assert {(c["nnz"] % 9, c["n_segs"] & 1) for c in packed} == {(r, p) for r in range(9) for p in (0, 1)}
    assert {(c["nnz"] % 9, c["n_segs"] == c["nnz"] // 9) for c in packed} == {(r, o) for r in range(9) for o in (False, True)}
    assert {(c["n_segs"] & 1, c["n_segs"] == c["nnz"] // 9, c["format"]) for c in packed} >= {(p, o, f) for p in (0, 1) for o in (False, True)
                                                                                           for f in ("plain",)}
    assert all(c["n_segs"] in (c["nnz"] // 9, c["nnz"] // 9 - 1) and (c["n_segs"] & 1) == c["factoring"] for c in packed)
    assert {c["factoring"] for c in by(format="group")} == {False, True} and sum(c["factoring"] for c in by(cls="c")) == 3
    assert {c["layout"]["S"] for c in by(format="group")} == {2, 4}
    assert {c["T"] for c in by(format="plain")} >= {64, 128} and {c["T"] for c in by(format="group")} == {512}
    assert by(cls="b")[0]["T"] == 64 and by(cls="b")[1]["T"] == 128
    assert 9 * by(cls="b")[0]["n_segs"] < 2 ** 20 <= 9 * by(cls="b")[1]["n_segs"] < 2 ** 20 + 64
    assert all(c["lens"][c["hub"]] > 2 * c["T"] and c["nnz"] // c["m"] < 128 for c in by(cls="b"))
    # every width class on every format, every operand offset on B and on C
    for fmt in ("plain", "group"):
        ks = [s["k"] for c in by(format=fmt) for s in c["steps"] if s["op"] == "flexspmm"]
        for name, holds in sd.WIDTH_CLASSES.items():
            assert any(holds(k) for k in ks), (fmt, name)
        assert all(k in sd.K_LIST for k in ks)
        flex = [s for c in by(format=fmt) for s in c["steps"] if s["op"] == "flexspmm"]
        assert {s["off_b"] for s in flex} == {s["off_c"] for s in flex} == {0, 1, 2, 3}, fmt
    for c in cases:
        k = [s["k"] for s in c["steps"][:3]]
        assert k[0] < k[2] < k[1], c["seed"]                     # narrow, wide, narrow
        assert [s["op"] for s in c["steps"]][:5] == ["flexspmm"] * 3 + ["cuspmm", "permutate"]
        assert (len(c["steps"]) == 6) == c["symmetric"] and np.array_equal(np.sort(c["steps"][4]["perm"]), np.arange(c["n"]))
    assert [c["seed"] for c in cases if c["symmetric"]] == [0, 4, 8, 12, 23]
    # sorted and shuffled input on both formats, both rectangular directions, half of class (a) square
    assert {(c["format"], c["shuffled"]) for c in packed} == {(f, s) for f in ("plain", "group") for s in (False, True)}
    assert sorted(c["seed"] for c in cases if c["m"] < c["n"]) == sorted(sd.RECT_WIDE)
    assert sorted(c["seed"] for c in cases if c["m"] > c["n"]) == sorted(sd.RECT_TALL)
    assert sum(c["m"] == c["n"] for c in by(cls="a")) == 8
    assert all(c["format"] == "plain" for c in cases if c["seed"] in sd.RECT_WIDE)              # (refused before the fix)
    # both sides of the quad kernel's mean row length, as launch_spmm estimates it from the upper bound of the chunk count
    est = {c["seed"]: -(-(9 * c["n_segs"] + 17) // c["T"]) * c["T"] // c["m"] for c in by(format="plain")}
    assert all((est[c["seed"]] >= sd.QUAD_MIN_ROW) == (c["seed"] in sd.DENSE) for c in by(cls="a", format="plain"))
    assert {su.style_of(s) for s in sd.DENSE} >= {1, 2, 3} and {su.style_of(s) for s in range(16) if s not in sd.DENSE} >= {0, 1, 3}
    # the degree-128 rule, the L2 rule and the refusal boundary, from both sides
    g128, p127, l2 = sd.case(18), sd.case(22), sd.case(21)
    assert 9 * g128["n_segs"] // g128["n"] == 128 and g128["format"] == "group" and g128["n"] == 16385
    assert 9 * p127["n_segs"] // p127["n"] == 127 and p127["format"] == "plain"
    assert l2["n"] == 16384 and 9 * l2["n_segs"] // l2["n"] >= 128 and l2["format"] == "plain"
    assert sd.case(19)["n"] == 32769 and sd.case(19)["layout"]["S"] == 4
    for seed, over in sd.BOUNDARY.items():
        c = sd.case(seed)
        ns = c["nnz"] // 9 - 1                                    # (the parity step costs a segment on all three)
        assert c["nnz"] == c["m"] + over and c["nnz"] % 9 == 8 and (c["nnz"] // 9) & 1 and not c["factoring"]
        assert 9 * ns == c["m"] + over - 17 and (c["n_segs"] == ns) == (9 * ns >= c["m"] + 1) and c["n_segs"] in (0, ns)
    assert [sd.case(s)["n_segs"] > 0 for s in sd.BOUNDARY] == [False, True, True]


def test_class_a_rows_meet_the_chunk_bounds():
    lens = np.concatenate([sd.case(s)["lens"] for s in range(16)])
    for b in sd.BOUNDS:
        assert (lens == b - 1).any() and (lens == b).any() and (lens == b + 1).any(), b
    assert lens.max() > 3 * sd.T_SMALL
    hit = ends = 0
    for s in range(16):
        L = sd.case(s)["lens"]
        floor = 1 if sd.case(s)["factoring"] else 0              # (a single-entry diagonal row stands for an empty one)
        hit += bool(np.any(np.isin(L[3:], sd.BOUNDS) & (L[2:-1] == floor) & (L[1:-2] == floor) & (L[:-3] == floor)))
        ends += bool(L[0] == floor and L[-1] == floor)
        if su.forced(s) and not sd.case(s)["symmetric"]:
            assert L[0] > max(sd.BOUNDS) and L[-1] > max(sd.BOUNDS), s
    assert hit >= 2 and ends >= 10


def test_group_cases_hold_their_rows():
    for seed in (18, 19, 20, 23):
        c = sd.case(seed)
        n, w, S = c["n"], c["layout"]["w"], c["layout"]["S"]
        rows = np.repeat(np.arange(n), c["lens"])
        virt = np.bincount((c["ci"] // w).astype(np.int64) * n + rows, minlength=S * n).reshape(S, n)
        assert sorted(v[0] for v in c["specials"].values()) == list(sd.GROUP_SPECIALS)
        for r, (L, (lo, hi)) in c["specials"].items():           # the whole row inside one slice, empty in the others
            assert virt[lo // w, r] == L == c["lens"][r] and hi <= min(n, (lo // w + 1) * w), (seed, r)
        assert len({lo // w for _, (lo, hi) in c["specials"].values()}) == S
        assert c["lens"][c["hub"]] == sd.GROUP_HUB and np.all(virt[:, c["hub"]] > 0)
        ends = 1 if c["factoring"] else 0
        assert c["lens"][0] == ends and (c["lens"][-1] == ends or c["hub"] == n - 1), seed
        assert ((virt == 0).any(0) & (virt > 0).any(0)).sum() >= 5
        key = rows.astype(np.int64) * n + c["ci"]
        assert len(np.unique(key)) < len(key)                    # duplicates
    assert {sd.case(s)["hub"] == sd.case(s)["n"] - 1 for s in (18, 19, 20, 23)} == {False, True}


# ---- the packer, on every seed, inside guarded buffers ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ALL)
def test_csr2tile_packs_the_case_exactly(seed, capfd):
    c = sd.case(seed)
    m, n, nnz, rp, ci, va = c["m"], c["n"], c["nnz"], c["rp"], c["ci"], c["va"]
    what = sd.describe(c, 0)
    out = sd.pack(rp, ci, va, m, n)
    err = capfd.readouterr().err
    ns = out["n_segs"]
    assert out["guards"], what
    assert ns == c["n_segs"], (what, ns)
    if c["format"] == "refused":
        assert ns == 0 and all(out["untouched"].values()), what
        assert err.count("libgcnspmm:") == 1 and "libgcnspmm: csr2tile:" in err, err
        return
    assert "libgcnspmm" not in err, err
    assert ns in (nnz // 9, nnz // 9 - 1) and (ns & 1) == c["factoring"], what
    assert np.all(out["tail"] == 0) and np.all(out["next"] == 0), what
    if c["format"] == "plain":
        T = sd.dropin_T(ns)
        assert T == c["T"], what
        assert np.array_equal(out["seg_rowPtr"][:m + 1], rp) and np.all(out["seg_rowPtr"][m + 1: 9 * ns] == nnz), what
        assert np.array_equal(out["segNzCV"][:nnz].view(np.int32), ci) and np.array_equal(out["segNzCV"][nnz:2 * nnz].view(np.int32), va.view(np.int32)), what
        nchunks = -(-nnz // T)
        holder = np.searchsorted(rp[1:], np.arange(nchunks, dtype=np.int64) * T, side="right")     # the row holding entry c * T
        assert holder.max() < m and np.all(rp[holder] <= np.arange(nchunks) * T) and holder[0] == np.flatnonzero(c["lens"])[0]
        holder[0] = 0                                              # (chunk 0 starts at row 0, empty or not)
        assert np.array_equal(out["segVoMap"][:nchunks], holder) and np.all(out["segVoMap"][nchunks: 8 * ns] == 0), what
    else:
        rows = np.repeat(np.arange(n), c["lens"])
        hd, _ = _check_group_format(out["seg_rowPtr"], out["segNzCV"], out["segVoMap"], n, ns, rp, ci, va, S=c["layout"]["S"],
                                    value_free=c["factoring"])
        assert hd["nchunks"] <= c["layout"]["nchunks_ub"] and hd["total"] <= c["layout"]["total_ub"], what
        if c["factoring"]:                                         # powers of two: csr2tile's square root is exact
            assert np.array_equal(out["segVoMap"][:n].view(np.float32), c["u"]), what


# ---- discrimination ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 5, 9, 13, 16, 17, 18, 19, 20, 23])
def test_outputs_depend_on_what_lies_past_every_bound(seed):
    c = sd.case(seed)
    only = None if c["cls"] == "a" else (0,)
    full = sd.twin(c, only=only)
    assert c["bounds"]
    for b in c["bounds"]:
        rows = np.flatnonzero(c["lens"] == b + 1)
        assert len(rows), (seed, b)
        less = sd.twin(c, cut=b, only=only)
        assert any(not np.array_equal(f[rows], g[rows]) for f, g, s in zip(full, less, c["steps"]) if s["op"] != "permutate"), (seed, b)


@pytest.mark.parametrize("seed", [0, 2, 6, 11, 12, 15, 22])
def test_outputs_depend_on_the_last_feature_column(seed):
    c = sd.case(seed)
    only = None if c["cls"] == "a" else (0, 4)                  # (the large graphs: the narrow flexspmm step and permutate)
    steps = [s for i, s in enumerate(c["steps"]) if only is None or i in only]
    for s, f, g in zip(steps, sd.twin(c, only=only), sd.twin(c, narrow=True, only=only)):
        if s["k"] > 1 and not (s["op"] == "flexspmm" and c["n_segs"] == 0):
            assert np.array_equal(f[:, :-1], g) and np.any(f[:, -1] != 0), (seed, s["op"], s["k"])
            assert not np.array_equal(f[:, -1], f[:, -2]), (seed, s["op"], s["k"])


def test_the_ulp_cases_land_on_opposite_parities(capfd):
    """(e): one entry 2 ulp off u[r] * u[c] is inside csr2tile's rule (n_segs stays odd: value-free), 16 ulp is outside it
    (even: the values travel) — on the host"""
    got = {}
    for ulps in (2, 16):
        c = sd.ulp_case(ulps)
        r, cc, e = c["moved"]
        want = c["u"][r] * c["u"][cc]
        assert c["ci"][e] == cc and want == 1.0 and c["va"][e] == np.float32(1.0 + ulps * 2.0 ** -23)
        assert (abs(c["va"][e] - want) <= np.float32(4.8e-7) * c["va"][e]) == (ulps == 2) == c["factoring"]
        out = sd.pack(c["rp"], c["ci"], c["va"], c["n"], c["n"])
        got[ulps] = out["n_segs"]
        assert out["guards"] and out["n_segs"] == c["n_segs"] and c["layout"] is not None
        hd, _ = _check_group_format(out["seg_rowPtr"], out["segNzCV"], out["segVoMap"], c["n"], out["n_segs"], c["rp"], c["ci"], c["va"],
                                    S=2, value_free=ulps == 2)
    assert got[2] & 1 == 1 and got[16] & 1 == 0 and abs(got[2] - got[16]) == 1
    assert "libgcnspmm" not in capfd.readouterr().err


# ---- csr2tile checks its input as an m x n matrix ---------------------------------------------------------------------------------
def _tall_with_a_column_past_n():
    m, n = 40, 10
    rng = np.random.default_rng(0)
    lens = np.full(m, 3)
    rp = np.zeros(m + 1, np.int32)
    rp[1:] = np.cumsum(lens)
    ci = rng.integers(0, n, int(rp[-1])).astype(np.int32)
    ci[57] = 35                                                   # in [n, m): a row of B that does not exist
    return m, n, rp, ci, np.ones(len(ci), np.float32)


def test_csr2tile_refuses_a_column_in_n_to_m(capfd):
    m, n, rp, ci, va = _tall_with_a_column_past_n()
    out = sd.pack(rp, ci, va, m, n)
    err = capfd.readouterr().err
    assert out["n_segs"] == 0 and out["guards"] and all(out["untouched"].values()), out["n_segs"]
    assert err.count("libgcnspmm:") == 1 and "libgcnspmm: csr2tile:" in err, err
    ci[57] = 9                                                    # the same matrix with that column inside: packs
    out = sd.pack(rp, ci, va, m, n)
    assert out["n_segs"] == sd.expected_n_segs(m, len(ci), False) > 0 and "libgcnspmm" not in capfd.readouterr().err


def test_csr2tile_packs_a_wide_matrix_with_columns_past_m(capfd):
    m, n = 30, 500
    rng = np.random.default_rng(1)
    rp = (np.arange(m + 1) * 4).astype(np.int32)
    ci = np.sort(rng.integers(m, n, (m, 4)), axis=1).ravel().astype(np.int32)        # every column >= m
    va = np.ones(len(ci), np.float32)
    out = sd.pack(rp, ci, va, m, n)
    assert "libgcnspmm" not in capfd.readouterr().err
    assert out["n_segs"] == sd.expected_n_segs(m, len(ci), False) > 0 and out["guards"]
    assert np.array_equal(out["seg_rowPtr"][:m + 1], rp) and np.array_equal(out["segNzCV"][:len(ci)].view(np.int32), ci)
    ci[-1] = n                                                    # one past the last column: refused
    assert sd.pack(rp, ci, va, m, n)["n_segs"] == 0 and "csr2tile" in capfd.readouterr().err


def test_csr2tile_refusal_names_both_sizes(capfd):
    m, n, rp, ci, va = _tall_with_a_column_past_n()
    sd.pack(rp, ci, va, m, n)
    err = capfd.readouterr().err
    assert "m=40" in err and "n=10" in err and f"nnz={len(ci)}" in err, err
    rp2 = rp.copy()
    rp2[3], rp2[4] = rp[4], rp[3]                                 # not monotone
    ci[57] = 1
    sd.pack(rp2, ci, va, m, n)
    err = capfd.readouterr().err
    assert err.count("libgcnspmm: csr2tile:") == 1 and "m=40" in err and "n=10" in err, err
