"""The random-shape sweep of tests/stress_units.py is sound — checked on the host, with no GPU: over the committed seed range
every bound of every unit is met from both sides, every forced placement, width, dtype, operand offset and stream occurs;
the drawn rows have outputs that depend on what lies past each bound (the twin on rows cut at the bound gives something
else) and on the last feature column; and the twins themselves agree, on these very cases, with independent formulations
(scipy for the transpose, the CSR of an edge list, the merged sum and the product; a plain fp64 argsort for the kNN
selection; np.maximum.reduceat for max / min).

SEEDS = 48.  Every assertion below holds from 40 seeds on: with 16 the widths of K_LIST have not met every row-length style
(that cycle has 20 seeds), with 20 and 24 the merge has not drawn every reduce x diagonal pair and the sampling group has not
run every step kind in every style, with 32 the latter still misses one.  48 is the next whole number of the 16-seed cycle in
which every style meets a forced placement once, one cycle above what is needed."""
import numpy as np
import pytest
import scipy.sparse as sp

import stress_units as su
from gcn_amd import _lib

SEEDS = 48
PAIRS = [(unit, b) for unit in su.UNITS for b in su.BOUNDS[unit]]


def test_the_bounds_are_the_librarys():
    assert _lib.KNN_TILE_Q == _lib.KNN_TILE_C == _lib.KNN_K_MAX == 64 and su.LONG == 2048
    assert su.SPGEMM_WIDE_N > _lib.SPGEMM_BLOCK_MAX and su.HUB_TOP == 2 * 8192 + 1
    for seed in range(SEEDS):
        for unit in su.UNITS:
            c = su.case(seed, unit)
            if unit == "knn":
                continue
            assert c["m"] <= 4000 and len(c["ci"]) <= su.NNZ_MAX, (seed, unit)
            assert c["n"] <= 4000 or (unit == "spgemm" and c["n"] == su.SPGEMM_WIDE_N), (seed, unit)
            assert c["rp"][-1] == len(c["ci"]) == len(c["va"]) and c["ci"].min(initial=0) >= 0, (seed, unit)
            assert c["ci"].max(initial=0) < (c["p"] if unit == "spgemm" else c["n"]), (seed, unit)
            assert np.array_equal(c["va"] * 8, np.rint(c["va"] * 8))


def test_case_is_a_pure_function_of_the_seed():
    for unit in su.UNITS:
        a, b = su._MAKERS[unit](5), su._MAKERS[unit](5)
        for key in ("rp", "ci", "va"):
            if key in a:
                assert np.array_equal(a[key], b[key])
        assert su.describe(a, 1) == su.describe(b, 1) and "seed 5" in su.describe(a, 1)


@pytest.mark.parametrize("unit, b", PAIRS, ids=str)
def test_every_bound_is_met_from_both_sides(unit, b):
    lens = np.concatenate([su.case(seed, unit)["lens"] for seed in range(SEEDS)])
    assert (lens == b).any() and (lens == b + 1).any() and (lens == b - 1).any()
    if unit in su.LONG_ROW_UNITS:
        assert lens.max() == su.HUB_TOP if unit != "spgemm" else lens.max() > 2 * b


def test_knn_meets_every_axis_bound():
    steps = [s for seed in range(SEEDS) for s in su.case(seed, "knn")["steps"]]
    for axis, b in (("q", 64), ("n", 64), ("d", 32), ("d", 64)):
        got = {s[axis] for s in steps}
        assert {b, b + 1} <= got and (b - 1 in got or (axis, b) == ("d", 64)), (axis, got)   # (K_LIST has no 63)
    assert {s["d"] for s in steps} >= set(su.K_LIST)
    ks = {s["knn_k"] for s in steps}
    assert {1, 63, _lib.KNN_K_MAX} <= ks and max(ks) == _lib.KNN_K_MAX
    assert any(s["knn_k"] > s["n"] for s in steps) and any(s["self_offset"] > 0 for s in steps)
    assert {s["splits"] for s in steps} >= {0, 1, 2, 3, 7} and any(s["ldx"] > s["d"] for s in steps)


@pytest.mark.parametrize("unit", su.LONG_ROW_UNITS)
def test_forced_placements(unit):
    top, seen = max(su.BOUNDS[unit]), set()
    for seed in range(SEEDS):
        c = su.case(seed, unit)
        assert c["forced"] == su.forced(seed)
        if not c["forced"]:
            continue
        seen.add(c["style"])
        lens, at = c["lens"], c["placed"]
        if unit == "aggregate" and c["transposed"]:
            lens = np.bincount(c["ci"], minlength=c["n"])          # (the drawn lengths are the columns' there)
        assert lens[0] > top and lens[-1] > top and lens[at["pair"]] > top and lens[at["pair2"]] > top, (unit, seed)
        if unit not in ("spgemm", "aggregate"):                    # one of the pair holds a single repeated column
            r = at["pair2"]
            assert len(np.unique(c["ci"][c["rp"][r]:c["rp"][r + 1]])) == 1
    assert seen == {0, 1, 2, 3}                                     # combined with every row-length style


def test_a_bound_length_row_follows_an_empty_run():
    for unit in su.LONG_ROW_UNITS:
        hit = False
        for seed in range(1, SEEDS, 4):
            lens = su.case(seed, unit)["lens"]
            r = np.flatnonzero(np.isin(lens[3:], su.BOUNDS[unit]) & (lens[2:-1] == 0) & (lens[1:-2] == 0) & (lens[:-3] == 0))
            hit |= len(r) > 0
        assert hit, unit


@pytest.mark.parametrize("unit", su.UNITS)
def test_widths_dtypes_offsets_and_streams_all_occur(unit):
    steps = [(seed, i, s) for seed in range(SEEDS) for i, s in enumerate(su.case(seed, unit)["steps"])]
    if unit in su.WIDTH_UNITS:
        for style in range(4):                                      # every width, in every row-length style
            assert {s["k"] for seed, _, s in steps if seed & 3 == style} == set(su.K_LIST), (unit, style)
    assert {s["dtype"] for _, _, s in steps} == set(su.TWO_DTYPES.get(unit, ("fp32",)))
    for operand in range(6):
        assert {s["offsets"][operand] for _, _, s in steps} == {0, 1, 2, 3}
    for i in range(3):                                              # both streams at every step, and changes between steps
        assert {s["side_stream"] for _, j, s in steps if j == i} == {False, True}
    ops = {}
    for seed, _, s in steps:
        ops.setdefault(s.get("op"), set()).add(seed & 3)
    assert all(styles == {0, 1, 2, 3} for styles in ops.values()), ops   # every step kind in every row-length style
    if unit == "sampling":
        assert {s["fanout"] for _, _, s in steps if s["op"] == "sample_neighbors"} >= {1, 64, 65, -1}
        assert {s["length"] for _, _, s in steps if s["op"] == "random_walk"} >= {0, 1, 4, 5}
    if unit == "coalesce":
        assert {(s["reduce"], s["diagonal"]) for _, _, s in steps if s["op"] == "coalesce_csr"} >= {(r, d) for r in ("sum", "max", "min", "first")
                                                                                                     for d in ("keep", "drop", "fill", "add")}
    if unit == "sddmm":
        assert len({tuple(sorted(su.case(seed, unit)["plan"].items())) for seed in range(SEEDS)}) == 5
    if unit == "aggregate":
        assert {(su.case(seed, unit)["transposed"], su.case(seed, unit)["mutable"]) for seed in range(SEEDS)} == {(a, b) for a in (False, True)
                                                                                                                 for b in (False, True)}
        assert {s["linear"] for _, _, s in steps} == {None, "sum", "mean"}


def _differs(a, b):
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            if u is None and v is None:
                continue
            u, v = np.asarray(u), np.asarray(v)
            if u.shape != v.shape or not np.array_equal(u, v, equal_nan=u.dtype.kind == "f"):
                return True
    return False


@pytest.mark.parametrize("unit, b", PAIRS, ids=str)
def test_outputs_depend_on_what_lies_past_the_bound(unit, b):
    """the twin on every row cut to its first b entries (kNN: the features cut to b columns) differs from the true twin on
    some seed — and not merely in shape: where only the shapes could differ (the integer outputs of a merge, say), the
    selected values, sums or samples past the bound are what changes"""
    hits = 0
    for seed in range(1, SEEDS, 4):                                 # the clustered-length seeds hold b + 1
        c = su.case(seed, unit)
        if (c["lens"] > b).any():
            hits += _differs(su.twin(c), su.twin(c, cut=b))
        if hits:
            break
    assert hits, (unit, b)


@pytest.mark.parametrize("unit", su.WIDTH_UNITS)
def test_outputs_depend_on_the_last_feature_column(unit):
    for seed in range(0, SEEDS, 5):
        c = su.case(seed, unit)
        full, less = su.twin(c), su.twin(c, narrow=True)
        for s, f, g in zip(c["steps"], full, less):
            if s["k"] == 1:
                continue
            if unit == "aggregate":                                 # the last column's selection is its own
                assert not np.array_equal(f[1][:, -1], f[1][:, -2]) and np.array_equal(f[1][:, :-1], g[1]), (seed, s["k"])
            else:
                assert _differs([f], [g]), (unit, seed, s["k"])


# ---- the twins on these cases against independent formulations -------------------------------------------------------------------
def _scipy(rp, ci, va, shape):
    return sp.csr_matrix((va.astype(np.float64), ci.astype(np.int64), rp.astype(np.int64)), shape=shape)


@pytest.mark.parametrize("seed", [1, 2, 5, 10, 15, 22])
def test_construct_and_coalesce_twins_are_scipys(seed):
    from coalesce_ref import coalesce_ref
    from construct_ref import bucket_ref, csr_from_edges_ref, transpose_ref
    c = su.case(seed, "construct")
    m, n = c["m"], c["n"]
    for i, s in enumerate(c["steps"]):
        e_rows, e_cols, e_vals = su.edge_list(c, i)
        mm = s["rows"][1] - s["rows"][0]
        rrp, rci, rva, eid = csr_from_edges_ref(e_rows, e_cols, (mm, n), e_vals, True)
        S = sp.coo_matrix((e_vals.astype(np.float64), (e_rows, e_cols)), shape=(mm, n)).tocsr()   # (sums repeats: eighths, exact)
        assert np.array_equal(_scipy(rrp, rci, rva, (mm, n)).toarray(), S.toarray()) if mm * n < 4e6 else True
        assert np.array_equal(np.diff(rrp), np.bincount(e_rows, minlength=mm)) and np.array_equal(e_cols[eid], rci)
        off, perm = bucket_ref(e_rows, mm)
        assert np.array_equal(e_rows[perm], np.sort(e_rows)) and np.array_equal(off, rrp)
        rp, ci, va = su.step_matrix(c, i)
        trp, trow, tva, teid = transpose_ref(rp, ci, va, n)
        T = _scipy(rp, ci, va, (mm, n)).T.tocsr()
        assert np.array_equal(trp, T.indptr) and np.array_equal(ci[teid], np.repeat(np.arange(n), np.diff(trp)))
        assert np.array_equal(va[teid], tva)
    c = su.case(seed, "coalesce")
    rp, ci, va = c["rp"], c["ci"], c["va"]
    orp, oci, ova, first, seg = coalesce_ref(rp, ci, va, c["n"], "sum", "keep")
    S = _scipy(rp, ci, va, (c["m"], c["n"]))
    S.sum_duplicates()
    S.sort_indices()
    assert np.array_equal(orp, S.indptr) and np.array_equal(oci, S.indices) and np.array_equal(ova.astype(np.float64), S.data)
    assert len(oci) < len(ci) and np.array_equal(oci[seg], ci)


@pytest.mark.parametrize("seed", [1, 2, 7, 10])
def test_spgemm_twin_is_scipys_product(seed):
    from spgemm_ref import sorted_merged_ref, spgemm_ref
    c = su.case(seed, "spgemm")
    b = sorted_merged_ref(c["d_rp"], c["d_ci"], c["d_va"])
    for B in ((c["b_rp"], c["b_ci"], c["b_va"]), b):
        rp, ci, va, prod = spgemm_ref(c["rp"], c["ci"], c["va"], *B, c["p"], c["n"])
        assert np.array_equal(prod, c["lens"])
        P = _scipy(c["rp"], c["ci"], c["va"], (c["m"], c["p"])) @ _scipy(*B, (c["p"], c["n"]))     # (64ths: every sum is exact)
        P.sort_indices()
        got = _scipy(rp, ci, va, (c["m"], c["n"]))
        assert abs(got - P).max() == 0 and got.nnz >= P.nnz         # (structural: a sum that cancels keeps its entry)


@pytest.mark.parametrize("seed", range(0, 12))
def test_knn_twin_is_an_fp64_argsort_on_integer_points(seed):
    from knn_ref import knn_ref
    for s in su.case(seed, "knn")["steps"]:
        idx, d2, rsum = knn_ref(s["x"], s["y"], s["knn_k"], s["self_offset"])
        D = ((s["x"].astype(np.float64)[:, None, :] - s["y"].astype(np.float64)[None, :, :]) ** 2).sum(2)   # exact: integers
        if s["self_offset"] >= 0:
            D[np.arange(s["q"]), s["self_offset"] + np.arange(s["q"])] = np.inf
        order = np.argsort(D, axis=1, kind="stable")[:, :s["knn_k"]]
        live = np.take_along_axis(D, order, 1) < np.inf
        have = min(s["knn_k"], s["n"])
        assert np.array_equal(idx[:, :have][live], order[live]) and np.all(idx[:, :have][~live] == -1) and np.all(idx[:, have:] == -1)
        assert np.array_equal(d2[:, :have][live].astype(np.float64), np.take_along_axis(D, order, 1)[live])


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 6])
def test_select_twin_is_reduceat_and_the_softmax_sums_to_one(seed):
    c = su.case(seed, "aggregate")
    rp, ci = c["rp"], c["ci"]
    ne = np.diff(rp) > 0
    for s in c["steps"]:
        out, arg = su.select_host(rp, ci, s["x"], s["op"])
        red = (np.maximum if s["op"] == "max" else np.minimum).reduceat(s["x"][ci], rp[:-1][ne].astype(np.int64), axis=0)
        assert np.array_equal(out[ne], red) and np.all(out[~ne] == 0) and np.all(arg[~ne] == -1)
        jj = np.arange(s["k"])[None, :]
        assert np.array_equal(s["x"][ci[arg[ne]], jj], out[ne])
        assert np.all(arg[ne] >= rp[:-1][ne, None]) and np.all(arg[ne] < rp[1:][ne, None])
    c = su.case(seed, "attention")
    for i, s in enumerate(c["steps"]):
        rp, _, _ = su.step_matrix(c, i)
        assert s["scores"].min() >= -8 and s["scores"].max() < 8
    p, sums = su.twin(c)[0]
    rp = su.step_matrix(c, 0)[0]
    assert np.allclose(np.add.reduceat(p, rp[:-1][np.diff(rp) > 0].astype(np.int64)), 1.0, rtol=1e-12)


def test_sddmm_host_is_the_dense_product_on_the_pattern():
    c = su.case(3, "sddmm")
    s = c["steps"][0]
    ref, mag = su.sddmm_host(c["rp"], c["ci"], s["A"], s["B"])
    rows = np.repeat(np.arange(c["m"]), c["lens"])
    dense = s["A"].astype(np.float64) @ s["B"].astype(np.float64).T
    assert np.array_equal(ref, dense[rows, c["ci"]]) and np.all(mag >= np.abs(ref)) and mag.max() < 2 ** 24
