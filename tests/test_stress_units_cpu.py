"""The random-shape sweep of tests/stress_units.py is sound — checked on the host, with no GPU: over the committed seed range
every bound of every unit is met from both sides, every forced placement, width, dtype, operand offset and stream occurs;
the drawn rows have outputs that depend on what lies past each bound (the twin on rows cut at the bound gives something
else) and on the last feature column; and the twins themselves agree, on these very cases, with independent formulations
(scipy for the transpose, the CSR of an edge list, the merged sum and the product; a plain fp64 argsort for the kNN
selection; np.maximum.reduceat for max / min).

The same holds for the units added later (heads, gatv2, edge_aggregate, sampled_dot, linkpred, mixed), with what is theirs:
the softmax bounds are met for EVERY head packing hp on its own, in entries whose len * hp straddles 32, 256 and 1024; VEC = 4
and VEC = 1, the 16 / 32 / 64 lanes of a slot, k on both sides of 64 / 128 / 256 and P = 1, 2, 4 occur per kernel, computed from
the drawn offsets and widths as the kernels choose them; every (op, act, reduce) of edge_aggregate and every axis value of the
lookup occur; the caps never cost a special row and narrow a width only by need; every grid sum stays below 2^24 units, which
is what the bit comparisons rest on; and the twins agree with a COO product per head and a reduceat (spmm_heads), dense
einsums on the pattern (sddmm_heads, GATv2 scores), reduceat and a first extremum per row (edge_aggregate), the brute-force
dictionary (lookup) and a set-intersection dot (sampled_dot).  One assertion is weaker for one unit: the mixed group's widths
occur over all styles together, not in every style (a style has 36 of its steps, of six kinds, for 15 and 13 widths).

SEEDS = 48.  Every assertion on the first eight units holds from 40 seeds on (the later units need all 48: a head count is a
function of seed >> 2, which takes its twelve values in every style only then): with 16 the widths of K_LIST have not met every row-length style
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


def test_the_later_units_keep_their_caps_and_their_special_rows():
    """nnz * k <= 4 000 000 and nnz * H <= 2 000 000 at every step (node arrays too), reached without a special row being
    lost: test_every_bound_is_met_from_both_sides, test_forced_placements and the hub of HUB_TOP entries hold on the capped
    matrices; a width is narrowed only where its drawn value does not fit the rows that are there"""
    assert su.UNITS[:8] == ("construct", "coalesce", "sampling", "aggregate", "attention", "sddmm", "spgemm", "knn")
    assert {1, 2, 3, 4, 5, 8, 16, 32} <= set(su.H_LIST) and len(su.H_LIST) <= 12 and len(set(su.H_LIST)) == len(su.H_LIST)
    assert {su.head_pack(H) for H in su.H_LIST} == {1, 2, 4, 8, 16} and su.head_pack(32) == su.head_pack(3) == su.head_pack(1) == 1
    assert su.heads_bounds(1) == (4, 32, 64, 256, 1024, 4096, 8192) and su.heads_bounds(16) == (2, 4, 16, 64, 4096, 8192)
    assert su.heads_bounds(5) == su.heads_bounds(32) == su.heads_bounds(1) and su.heads_bounds(4) == (4, 8, 64, 256, 4096, 8192)
    for unit in ("heads", "gatv2", "edge_aggregate", "mixed"):
        for seed in range(SEEDS):
            c = su.case(seed, unit)
            rows = max(len(c["ci"]), c["m"], c["n"])
            for i, s in enumerate(c["steps"]):
                assert rows * s["k"] <= su.NNZ_K_MAX and len(c["ci"]) * s.get("H", 1) <= su.NNZ_H_MAX, (unit, seed, i)
                if s["kind"] in su.GATHER_KINDS:
                    assert s["k"] == s["H"] * s["F"] and s["F"] <= s["F_drawn"] and s["H"] == su.step_heads(seed, i)
                    wider = [f for f in su.F_LIST if s["F"] < f <= s["F_drawn"]]
                    assert all(rows * s["H"] * f > su.NNZ_K_MAX for f in wider), (unit, seed, i)       # narrowed only by need
                elif "k_drawn" in s:
                    wider = [k for k in su.K_LIST if s["k"] < k <= s["k_drawn"]]
                    assert all(rows * k > su.NNZ_K_MAX for k in wider), (unit, seed, i)
            if unit in su.HEAD_UNITS:                               # step 1 has another H: the scratch is outgrown, then under-used
                H = [s["H"] for s in c["steps"]]
                assert H[0] == H[2] != H[1] and H[0] == su.H_LIST[(seed >> 2) % len(su.H_LIST)]
    for seed in range(SEEDS):
        c = su.case(seed, "mixed")
        assert len({s["kind"] for s in c["steps"]}) == 3 and c["m"] == c["n"] and np.array_equal(c["new_va"] * 8, np.rint(c["new_va"] * 8))
        assert len(c["new_va"]) == len(c["va"]) and not np.array_equal(c["new_va"], c["va"])
    assert {su.case(seed, "mixed")["update"] for seed in range(SEEDS) if seed & 3 == 1} == {False, True}


def test_case_is_a_pure_function_of_the_seed():
    for unit in su.UNITS:
        a, b = su._MAKERS[unit](5), su._MAKERS[unit](5)
        for key in ("rp", "ci", "va"):
            if key in a:
                assert np.array_equal(a[key], b[key])
        assert su.describe(a, 1) == su.describe(b, 1) and "seed 5" in su.describe(a, 1)
        if unit in su.NEW_UNITS:                                    # (their operands are drawn at every call)
            x, y = su.step_inputs(a, 1), su.step_inputs(b, 1)
            assert x.keys() == y.keys() and all(np.array_equal(x[key], y[key]) for key in x)


@pytest.mark.parametrize("unit, b", PAIRS, ids=str)
def test_every_bound_is_met_from_both_sides(unit, b):
    lens = np.concatenate([su.case(seed, unit)["lens"] for seed in range(SEEDS)])
    assert (lens == b).any() and (lens == b + 1).any() and (lens == b - 1).any()
    if unit in su.LONG_ROW_UNITS:
        assert lens.max() == su.HUB_TOP if unit != "spgemm" else lens.max() > 2 * b


@pytest.mark.parametrize("hp", [1, 2, 4, 8, 16])
def test_heads_meet_every_bound_of_every_head_packing(hp):
    """the softmax family counts ELEMENTS len * hp: for every hp on its own, rows of b - 1, b and b + 1 entries with b * hp
    = 32, 256, 1024, beside the long-row bound and the gather engine's"""
    cases = [su.case(seed, "heads") for seed in range(SEEDS) if su.case(seed, "heads")["hp"] == hp]
    lens = np.concatenate([c["lens"] for c in cases])
    assert {su.head_pack(c["H"]) for c in cases} == {hp} and all(su.heads_bounds(c["H"]) == su.heads_bounds(hp if hp > 1 else 1) for c in cases)
    for e in su.SOFTMAX_ELEMENTS:
        assert e % hp == 0 and {e // hp - 1, e // hp, e // hp + 1} <= set(lens.tolist()), (hp, e)
        assert (lens * hp < e).any() and (lens * hp == e).any() and (lens * hp > e).any()
    for b in (su.SOFTMAX_LONG,) + su.GATHER_BOUNDS:
        assert {b - 1, b, b + 1} <= set(lens.tolist()), (hp, b)
    assert lens.max() > su.SOFTMAX_LONG + 1                         # (and HUB_TOP over all of them: test_every_bound_is_met_from_both_sides)
    if hp == 1:                                                    # one head, the slow route, and more heads than the fast route takes
        assert {c["H"] for c in cases} >= {1, 3, 5, 32}


def test_sampled_dot_meets_the_bounds_of_both_operands():
    x_lens = np.concatenate([su.case(seed, "sampled_dot")["x_lens"] for seed in range(SEEDS)])
    p_lens = np.concatenate([su.case(seed, "sampled_dot")["lens"] for seed in range(SEEDS)])
    for b in (16, 64, su.LONG):
        assert {b - 1, b, b + 1} <= set(x_lens.tolist()), b
    assert {su.LONG - 1, su.LONG, su.LONG + 1, 63, 64, 65} <= set(p_lens.tolist())
    for seed in range(SEEDS):                                       # what the kernel's contract asks of the operands
        c = su.case(seed, "sampled_dot")
        rows = np.repeat(np.arange(c["m"]), np.diff(c["y_rp"]))
        assert np.all((np.diff(c["y_ci"]) > 0) | (np.diff(rows) > 0)), "Y's rows must ascend strictly"
        assert c["x_ci"].max() < c["w"] and c["y_ci"].max() < c["w"] and c["ci"].max() < c["m"]
    c = su.case(1, "sampled_dot")
    assert len(np.unique(c["x_ci"])) < len(c["x_ci"]) and np.any(np.diff(c["x_ci"][:c["x_rp"][-1]]) < 0)   # X: repeats, unsorted


def test_linkpred_meets_every_axis_value():
    steps = [(su.case(seed, "linkpred"), i, s) for seed in range(SEEDS) for i, s in enumerate(su.case(seed, "linkpred")["steps"])]
    small = _lib_lookup_small()
    assert set(su.QUERY_COUNTS) == {1, 63, 64, 65, small - 1, small, small + 1}
    for op in ("find_edges", "negative_sample"):
        assert {s["count"] for _, _, s in steps if s["op"] == op} == set(su.QUERY_COUNTS), op
    neg = [s for _, _, s in steps if s["op"] == "negative_sample"]
    assert {s["num_neg"] for s in neg} == {1, 3} and {s["max_tries"] for s in neg} == {1, 4, 5, 32, 64}
    assert {s["exclude_self"] for s in neg} == {False, True} and {s["dtype"] for s in neg} == {"int32", "int64"}
    for seed in range(SEEDS):                                       # interleaved: never the same call twice in a row
        ops = [s["op"] for s in su.case(seed, "linkpred")["steps"]]
        assert ops[0] != ops[1] != ops[2]
    for c, i, s in steps[:30]:
        x, rp, ci, full = su.step_inputs(c, i), c["rp"], c["ci"], c["full"]
        assert np.array_equal(ci[rp[full]:rp[full + 1]], np.arange(c["n"]))            # one row stores every column
        rows = np.repeat(np.arange(c["m"]), np.diff(rp))
        assert np.all((np.diff(ci) >= 0) | (np.diff(rows) > 0)) and np.any((np.diff(ci) == 0) & (np.diff(rows) == 0))   # sorted, with repeats
        if s["op"] == "negative_sample":
            out = su.twin_step(c, i)[0]
            assert np.all(out[x["q_rows"] == full] == -1) and x["q_rows"][0] == full    # every try is refused
            assert ((x["q_rows"] < 0).any() and (x["q_rows"] >= c["m"]).any()) or s["count"] < 63
        elif s["count"] > 60:
            assert (x["q_rows"] < 0).any() and (x["q_rows"] >= c["m"]).any() and (x["q_cols"] < 0).any() and (x["q_cols"] >= c["n"]).any()
            found = su.twin_step(c, i)[0]
            assert (found >= 0).any() and (found == -1).any()


def _lib_lookup_small():
    """kLookupSmall as gcn_amd/csrc/lookup.hip defines it (it is not exported: read from the source)"""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gcn_amd", "csrc", "lookup.hip")
    shift = re.search(r"constexpr int kLookupSmall = 1 << (\d+);", open(path, encoding="utf-8").read())
    assert shift, "lookup.hip no longer defines kLookupSmall as a power of two"
    return 1 << int(shift.group(1))


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
        if c.get("transposed"):
            lens = np.bincount(c["ci"], minlength=c["n"])          # (the drawn lengths are the columns' there)
            assert np.array_equal(lens, c["lens"])
        if unit == "heads":
            top = max(su.heads_bounds(c["H"]))
        assert lens[0] > top and lens[-1] > top and lens[at["pair"]] > top and lens[at["pair2"]] > top, (unit, seed)
        if unit not in ("spgemm", "aggregate") and not c.get("transposed"):   # one of the pair holds a single repeated column
            r = at["pair2"]
            assert len(np.unique(c["ci"][c["rp"][r]:c["rp"][r + 1]])) == 1
    assert seen == {0, 1, 2, 3}                                     # combined with every row-length style


def test_a_bound_length_row_follows_an_empty_run():
    for unit in su.LONG_ROW_UNITS:
        hit = False
        for seed in range(1, SEEDS, 4):
            lens = su.case(seed, unit)["lens"]
            bounds = su.BOUNDS[unit] if unit != "heads" else su.heads_bounds(su.case(seed, unit)["H"])   # (a bound of ITS head count)
            r = np.flatnonzero(np.isin(lens[3:], bounds) &(lens[2:-1] == 0) & (lens[1:-2] == 0) & (lens[:-3] == 0))
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
    if unit in ("gatv2", "edge_aggregate"):
        for style in range(3):                                      # (the dense-ish style is never transposed, as in aggregate)
            assert {su.case(seed, unit)["transposed"] for seed in range(SEEDS) if seed & 3 == style} == {False, True}, (unit, style)
    if unit == "edge_aggregate":
        assert {(s["msg"], s["act"], s["reduce"]) for _, _, s in steps} == set(su.EDGE_TRIPLES) and len(su.EDGE_TRIPLES) == 16
        assert {(su.vec_of(s, 2), s["reduce"] in ("max", "min")) for _, _, s in steps} == {(v, sel) for v in (1, 4) for sel in (False, True)}
    if unit == "gatv2":
        assert {s["slope"] for _, _, s in steps} == {0.5, 0.25}
    if unit in su.HEAD_UNITS:
        gather = [(seed, s) for seed, _, s in steps if s["kind"] in su.GATHER_KINDS]
        for style in range(4):                                      # every head count in every style; every drawn width too
            assert {s["H"] for seed, _, s in steps if seed & 3 == style} == set(su.H_LIST), (unit, style)
            assert {s["F_drawn"] for seed, s in gather if seed & 3 == style} == set(su.F_LIST), (unit, style)
        assert {s["F_drawn"] for _, s in gather} == set(su.F_LIST) and {s["F"] for _, s in gather} <= set(su.F_LIST)
        for kind in {s["kind"] for _, s in gather}:                 # per kernel: both forms, k on both sides of the lane and tile bounds
            mine = [s for _, s in gather if s["kind"] == kind]
            operands = {"spmm_heads": 1, "sddmm_heads": 2, "gatv2_scores": 3}[kind]
            assert {su.vec_of(s, operands) for s in mine} == {1, 4}, kind
            assert any(s["F"] % 4 for s in mine) and any(s["F"] % 4 == 0 and su.vec_of(s, operands) == 1 for s in mine), kind
            for b in (64, 128, 256) if kind != "sddmm_heads" else (64,):   # (the lane and tile bounds are the row walks')
                assert any(b // 2 < s["k"] <= b for s in mine) and any(s["k"] > b for s in mine), (kind, b)
            for vec in (1, 4) if kind != "sddmm_heads" else ():     # the row walks: 16, 32, 64 lanes a slot (k / VEC <= 16, <= 32, more)
                units = {min(2, (s["k"] // vec - 1) // 16) for s in mine if su.vec_of(s, operands) == vec}
                assert units == {0, 1, 2}, (kind, vec, units)
            if kind != "spmm_heads":                                # P = 1, 2, 4 lanes an (entry, head): the lowest set bit of U = F / VEC
                lanes = {min(4, (s["F"] // su.vec_of(s, operands)) & -(s["F"] // su.vec_of(s, operands))) for s in mine}
                assert lanes == {1, 2, 4}, (kind, lanes)
                for vec in (1, 4):
                    assert {min(4, (s["F"] // vec) & -(s["F"] // vec)) for s in mine if su.vec_of(s, operands) == vec} == {1, 2, 4}, (kind, vec)
            assert {su.head_pack(s["H"]) > 1 or s["H"] == 1 for s in mine} == {False, True}, kind       # fast and slow route
    if unit == "heads":
        assert {s["perm"] for _, _, s in steps if s["op"] == "segment_sum"} == {False, True}
        assert {s["slope"] for _, _, s in steps if s["op"] == "gat_edge_softmax"} == {0.2, 1.5}
        for op in su.HEADS_OPS:                                     # every op meets every head packing
            assert {su.head_pack(s["H"]) for _, _, s in steps if s["op"] == op} == {1, 2, 4, 8, 16}, op
    if unit == "sampled_dot":
        dots = [s for _, _, s in steps if s["op"] != "product"]
        assert {(s["op"], s["x_mode"]) for s in dots} == {(o, v) for o in ("dot", "dot_by_col") for v in ("own", "given", "none")}
        assert {(s["op"], s["y_mode"]) for s in dots} == {(o, v) for o in ("dot", "dot_by_col") for v in ("own", "given", "none")}
        # (never both the operands' own values: SparseProduct.values has a backward to run at every product step)
        assert {(s["x_mode"], s["y_mode"]) for _, _, s in steps if s["op"] == "product"} == {("own", "given"), ("given", "own"), ("given", "given")}
    if unit == "mixed":
        # (a style has 36 steps of six kinds, fewer of a kind than K_LIST or F_LIST has widths: here, and only here, the
        # widths are asserted over all styles together and not in every style)
        assert {s["k_drawn"] for _, _, s in steps if "k_drawn" in s} == set(su.K_LIST)
        assert {s["F_drawn"] for _, _, s in steps if s["kind"] in su.GATHER_KINDS} == set(su.F_LIST)
        kinds = {tuple(s["kind"] for s in su.case(seed, unit)["steps"]) for seed in range(SEEDS)}
        pairs = {(a, b) for ks in kinds for a, b in zip(ks, ks[1:])}
        assert len(pairs) >= 20, pairs                              # of the 30 ordered pairs of different kinds
        for kind in su.MIXED_KINDS:                                 # every kind first, in the middle and last; after an update too
            assert {i for _, i, s in steps if s["kind"] == kind} == {0, 1, 2}, kind
            assert any(su.case(seed, unit)["update"] for seed, i, s in steps if s["kind"] == kind and i == 2), kind


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
        if unit == "heads" and b not in su.heads_bounds(c["H"]):    # (BOUNDS["heads"] is the union: b must be a bound of THIS head count)
            continue
        if (c["lens"] > b).any():
            hits += _differs(su.twin(c), su.twin(c, cut=b))
        if hits:
            break
    assert hits, (unit, b)


@pytest.mark.parametrize("unit", su.WIDTH_UNITS + su.HEAD_UNITS)
def test_outputs_depend_on_the_last_feature_column(unit):
    """(the head units: on the last column of every head)"""
    checked = 0
    for seed in range(0, SEEDS, 5):
        c = su.case(seed, unit)
        full, less = su.twin(c), su.twin(c, narrow=True)
        for s, f, g in zip(c["steps"], full, less):
            if s["k"] == 1 or (unit in su.HEAD_UNITS and (s["F"] == 1 or s["kind"] not in su.GATHER_KINDS)):
                continue
            checked += 1
            if unit in su.HEAD_UNITS and s["kind"] == "spmm_heads":  # the other columns are untouched, every head's last one is its own
                assert np.array_equal(su.drop_last_of_every_head(f[0], s["H"]), g[0]), (seed, s["k"])
                last = f[0].reshape(len(f[0]), s["H"], s["F"])
                assert not np.array_equal(last[:, :, -1], last[:, :, -2]), (seed, s["k"])
            elif unit in su.HEAD_UNITS:                             # a per-(entry, head) dot product: the values change
                dead = s["kind"] == "gatv2_scores" and not su.step_inputs(c, c["steps"].index(s))["att"][:, -1].any()
                assert f[0].shape == g[0].shape and (dead or not np.array_equal(f[0], g[0])), (unit, seed, s["k"])
                checked -= dead                                     # (every head's last weight drawn as zero)
            elif unit == "aggregate":                               # the last column's selection is its own
                assert not np.array_equal(f[1][:, -1], f[1][:, -2]) and np.array_equal(f[1][:, :-1], g[1]), (seed, s["k"])
            else:
                assert _differs([f], [g]), (unit, seed, s["k"])
    assert checked >= 6, (unit, checked)


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


# ---- the later units: their twins against independent formulations, and the exactness their bit comparisons rest on ---------------
def _pattern(c):
    rp = c["rp"].astype(np.int64)
    return rp, c["ci"].astype(np.int64), np.repeat(np.arange(c["m"]), np.diff(rp))


def _steps_of(unit, kind, limit):
    """(case, step index, step) of the first `limit` steps of that kind whose arrays are small enough for a dense check"""
    found = []
    for seed in range(SEEDS):
        c = su.case(seed, unit)
        for i, s in enumerate(c["steps"]):
            if s["kind"] == kind and len(found) < limit and max(len(c["ci"]), c["m"], c["n"]) * s.get("k", 1) <= 600_000:
                found.append((c, i, s))
    assert len(found) == limit, (unit, kind, len(found))
    return found


@pytest.mark.parametrize("unit", ["heads", "mixed"])
def test_spmm_heads_twin_is_a_scipy_product_per_head_and_a_reduceat(unit):
    for c, i, s in _steps_of(unit, "spmm_heads", 4):
        x, (rp, ci, rows), H, F = su.step_inputs(c, i), _pattern(c), s["H"], s["F"]
        out = su.twin_step(c, i)[0]
        terms = x["vals"].astype(np.float64)[:, :, None] * x["x"].astype(np.float64)[ci].reshape(len(ci), H, F)
        ne = np.diff(rp) > 0
        assert np.array_equal(out[ne], np.add.reduceat(terms.reshape(len(ci), -1), rp[:-1][ne], axis=0)) and np.all(out[~ne] == 0)
        for h in (0, H - 1):                                        # (a COO matrix: scipy adds the repeated pairs itself)
            A = sp.coo_matrix((x["vals"][:, h].astype(np.float64), (rows, ci)), shape=(c["m"], c["n"])).tocsr()
            assert np.array_equal(out[:, h * F:(h + 1) * F], A @ x["x"][:, h * F:(h + 1) * F].astype(np.float64))


def test_sddmm_heads_and_gatv2_twins_are_dense_einsums_on_the_pattern():
    for unit, kind in (("heads", "sddmm_heads"), ("gatv2", "gatv2_scores"), ("mixed", "gatv2_scores")):
        for c, i, s in _steps_of(unit, kind, 3):
            x, (rp, ci, rows), H, F = su.step_inputs(c, i), _pattern(c), s["H"], s["F"]
            R = min(c["m"], max(1, 2_000_000 // (c["n"] * s["k"])))          # the first R rows against all n columns, densely
            e = slice(0, int(rp[R]))
            out = su.twin_step(c, i)[0]
            if kind == "sddmm_heads":
                dense = np.einsum("rhf,nhf->rnh", x["a"][:R].astype(np.float64).reshape(R, H, F), x["b"].astype(np.float64).reshape(c["n"], H, F))
            else:
                t = x["hd"][:R].astype(np.float64)[:, None, :] + x["hs"].astype(np.float64)[None, :, :]
                t = np.where(t > 0, t, s["slope"] * t).reshape(R, c["n"], H, F)
                dense = np.einsum("rnhf,hf->rnh", t, x["att"].astype(np.float64))
            assert np.array_equal(out[e], dense[rows[e], ci[e]]), (unit, kind, c["seed"], i)


@pytest.mark.parametrize("unit", ["edge_aggregate", "mixed"])
def test_edge_aggregate_twin_is_reduceat_and_a_first_extremum_per_row(unit):
    import edge_aggregate_ref as ea
    seen = set()
    for c, i, s in _steps_of(unit, "edge_aggregate", 8):
        x, (rp, ci, rows) = su.step_inputs(c, i), _pattern(c)
        t = x["x"][ci] * x["w"] if s["msg"] == "mul" else x["x"][ci] + x["w"]
        msg = np.where(t < 0, np.float32(0), t) if s["act"] == "relu" else t
        ne, jj = np.diff(rp) > 0, np.arange(s["k"])[None, :]
        got = su.twin_step(c, i)
        seen.add(s["reduce"])
        if s["reduce"] in ("sum", "mean"):
            want = np.add.reduceat(msg.astype(np.float64), rp[:-1][ne], axis=0) / (np.diff(rp)[ne][:, None] if s["reduce"] == "mean" else 1)
            assert np.array_equal(got[0][ne], want) and np.all(got[0][~ne] == 0)
        else:
            red = (np.maximum if s["reduce"] == "max" else np.minimum).reduceat(msg, rp[:-1][ne], axis=0)
            out, arg = got
            assert np.array_equal(out[ne], red) and np.all(out[~ne] == 0) and np.all(arg[~ne] == -1)
            assert np.array_equal(msg[arg[ne], jj], red) and np.all(arg[ne] >= rp[:-1][ne, None]) and np.all(arg[ne] < rp[1:][ne, None])
            before = np.arange(len(ci))[:, None] < np.repeat(arg[ne], np.diff(rp)[ne], axis=0)   # no equal message earlier in the row
            assert not np.any(before & (msg == np.repeat(red, np.diff(rp)[ne], axis=0)))
            ties = np.add.reduceat((msg == np.repeat(red, np.diff(rp)[ne], axis=0)).astype(np.int64), rp[:-1][ne], axis=0)
            crowded = np.diff(rp)[ne] >= 32                         # level-valued inputs: in a row of some length the selection ties
            assert not crowded.any() or (ties[crowded] > 1).mean() > 0.75
    assert len(seen) >= 3 or unit == "mixed", seen


def test_lookup_twin_is_the_brute_force_dictionary_and_negatives_are_not_stored():
    from linkpred_ref import find_entries_brute
    done = {"find_edges": 0, "negative_sample": 0}
    for seed in range(SEEDS):
        c = su.case(seed, "linkpred")
        for i, s in enumerate(c["steps"]):
            if s["count"] > 65 or done[s["op"]] >= 6:
                continue
            done[s["op"]] += 1
            x, got = su.step_inputs(c, i), su.twin_step(c, i)[0]
            if s["op"] == "find_edges":
                assert np.array_equal(got, find_entries_brute(c["rp"], c["ci"], x["q_rows"], x["q_cols"]))
            else:
                for r, out in zip(x["q_rows"], got):
                    kept = out[out >= 0]
                    if not 0 <= r < c["m"]:
                        assert len(kept) == 0
                        continue
                    assert not np.isin(kept, c["ci"][c["rp"][r]:c["rp"][r + 1]]).any() and (kept < c["n"]).all()
                    assert not (s["exclude_self"] and (kept == r).any())
    assert min(done.values()) >= 4


@pytest.mark.parametrize("seed", [0, 1, 2, 7])
def test_sampled_dot_twin_is_a_set_intersection_dot(seed):
    c = su.case(seed, "sampled_dot")
    for i, s in enumerate(c["steps"]):
        p, np_cols, x, y, w, by_col = su.dot_operands(c, i)
        got = su.twin_step(c, i)[0]
        ones = lambda v, cnt: np.ones(cnt) if v is None else v.astype(np.float64)
        xv, yv = ones(x[2], len(x[1])), ones(y[2], len(y[1]))
        y_rows = [dict(zip(y[1][y[0][j]:y[0][j + 1]].tolist(), yv[y[0][j]:y[0][j + 1]].tolist())) for j in range(len(y[0]) - 1)]
        rows = np.repeat(np.arange(len(p[0]) - 1), np.diff(p[0]))
        for e in np.random.default_rng(seed).permutation(len(rows))[:3000]:          # (64ths: every sum is exact)
            xr, yr = (int(p[1][e]), int(rows[e])) if by_col else (int(rows[e]), int(p[1][e]))
            common = [(t, x[1][t]) for t in range(x[0][xr], x[0][xr + 1]) if x[1][t] in y_rows[yr]]
            assert got[e] == sum(xv[t] * y_rows[yr][col] for t, col in common), (seed, i, e)
        assert np.count_nonzero(got) > len(got) // 20


@pytest.mark.parametrize("unit", ["heads", "gatv2", "edge_aggregate", "mixed"])
def test_every_grid_sum_is_exact_in_fp32(unit):
    """the bit comparisons rest on this: every term is a multiple of the grid's unit and, with the longest row and the
    longest column of the case, every partial sum of any order stays below 2^24 units"""
    ranges = dict(spmm_heads=dict(x=3, vals=1, g=3), sddmm_heads=dict(a=3, b=3, g=1), gatv2_scores=dict(hd=2, hs=2, att=2, g=1),
                  edge_aggregate=dict(x=2, w=1, g=3), aggregate=dict(x=2, g=8))
    for seed in range(SEEDS):
        c = su.case(seed, unit)
        longest = max(int(np.diff(c["rp"]).max()), int(np.bincount(c["ci"], minlength=c["n"]).max()))
        nnz = len(c["ci"])
        for i, s in enumerate(c["steps"]):
            kind = s["kind"]
            if kind not in ranges:
                continue
            if seed % 6 == 0:                                       # the ranges and the grids of the drawn operands
                for name, a in su.step_inputs(c, i).items():
                    assert np.abs(a).max(initial=0) <= ranges[kind][name] and np.array_equal(a * 8, np.rint(a * 8)), (unit, seed, i, name)
            if kind == "spmm_heads":                                # terms vals * x, vals * g: eighths, |.| <= 21/8; g . x per head
                assert longest * 21 < 2 ** 24 and s["F"] * 9 < 2 ** 24
            elif kind == "sddmm_heads":                             # a . b per head; its gradients g * b, g * a: eighths, |.| <= 21/8
                assert longest * 21 < 2 ** 24 and s["F"] * 9 < 2 ** 24
            elif kind == "gatv2_scores":                            # g D and g t D: 32nds with slope 1/4, |g t D| <= 7/8 * 4; att.grad
                assert s["slope"] in (0.5, 0.25) and longest * 112 < 2 ** 24 and nnz * 112 < 2 ** 24 and s["F"] * 8 * 4 < 2 ** 24
            elif kind == "edge_aggregate":                          # messages and gradient terms: eighths, |.| <= 3 (x + w, g * w)
                assert longest * 24 < 2 ** 24
            else:                                                   # a selection's gradient: integers, |g| <= 8
                assert longest * 8 < 2 ** 24
