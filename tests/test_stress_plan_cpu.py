"""The seeded walks of tests/stress_plan.py cover what they claim — checked on the host, with no GPU, over the committed seed
range: every reconfiguration and refusal in every family it is legal in, every ordered pair of plan states as the states
of two consecutive product calls, every width class after a wider and after a narrower call, bf16 after fp32 and back,
every epilogue in every state, an SDDMM on both sides of a re-slicing, a narrow call on both sides of enable_slicing(8) and
(-1) in the `auto` family; the operands of every call meet util.assert_exact_inputs, and consecutive calls have references
that differ in every non-empty row (a stale copy of B is wrong data).  Everything is computed here from the steps
themselves, by replaying them on a fresh model, not from the generator's own bookkeeping.

SEEDS = value_free 7, weighted 7, panels 8, mutable 6, auto 3: 31 walks.  A family steers its walks to what it still owes
the sweep (stress_plan._needs), and these are the first seeds after which it owes nothing (asserted below: one seed fewer
leaves something owed).  "Every reconfiguration in every family" is asserted for the ten call NAMES; every listed ARGUMENT
value (slice counts, panel modes, tiles, gather widths, blocks per CU) is asserted over the sweep as a whole: a walk of 14
steps has no room for 22 setting values per family."""
import numpy as np
import pytest
import scipy.sparse as sp_

import stress_plan as sp
import util
from gcn_amd import _lib

SEEDS = {"value_free": 7, "weighted": 7, "panels": 8, "mutable": 6, "auto": 3}
WALKS = [(f, s) for f in sp.FAMILIES for s in range(SEEDS[f])]


def _all(family=None):
    return [sp.walk(s, f) for f, s in WALKS if family in (None, f)]


def _calls(w):
    return [s for s in w["steps"] if s["op"] == "call"]


def _call_pairs(family=None):
    """consecutive product calls of a walk, with the reconfigurations between them"""
    for w in _all(family):
        idx = [i for i, s in enumerate(w["steps"]) if s["op"] == "call"]
        for a, b in zip(idx, idx[1:]):
            yield w, w["steps"][a], w["steps"][b], w["steps"][a + 1:b]


def test_the_rules_are_the_librarys():
    """the model's twins of auto_slices agree with the library on every shape used, and the `auto` graph is the smallest
    the automatic rules act on: four slices, a narrow set of two, and neither one column fewer"""
    lib = _lib.load()
    for f in sp.FAMILIES:
        for seed in (0, 1):
            o = sp.operands(f, seed)
            for vf in (0, 1):
                assert sp.auto_slices(o["m"], o["n"], len(o["ci"]), bool(vf)) == lib.gcn_spmm_auto_slices(o["m"], o["n"], len(o["ci"]), vf)
            if f != "auto":
                assert o["m"] <= 6000 and sp.auto_slices(o["m"], o["n"], len(o["ci"]), True) == 0
    o = sp.operands("auto", 0)
    n, nnz = o["n"], len(o["ci"])
    assert o["m"] == n and nnz // n >= 128
    assert lib.gcn_spmm_auto_slices(n, n, nnz, 1) == 4 and lib.gcn_spmm_auto_slices(n, n, nnz, 0) == 4
    assert sp.narrow_slices(n, n, nnz, 4) == 2
    assert lib.gcn_spmm_auto_slices(n - 1, n - 1, nnz, 1) != 4
    assert nnz // n >= 48 and len(sp.operands("value_free", 0)["ci"]) // 6000 >= 48      # value-free pays (kVallessMinPerCol)
    assert sp.coverage_of("panels", 0) >= 0.5 and sp.coverage_of("panels", 1) >= 0.5     # enable_panels(-1) turns them on
    assert all(sp.coverage_of(f, 0) < 0.5 for f in ("value_free", "weighted", "mutable", "auto"))


def test_walks_are_pure_functions_and_replay_on_a_fresh_model():
    for f, seed in WALKS:
        w = sp.walk(seed, f)
        assert w is sp.walk(seed, f) and sp.MIN_STEPS <= len(w["steps"]) <= sp.MAX_STEPS, (f, seed)
        assert w["side_stream"] == bool(seed % 2)
        m = sp.Model(f, seed)
        for s in w["steps"]:
            if s["op"] == "reconf":
                assert m.apply(s["name"], s["arg"]) == s["expect"], (f, seed, s)
            else:
                assert s["state"] == m.state() and (s["state"] is None or s["state"] in sp.LEGAL[f]), (f, seed, s)
                if s["kind"] == "prelaid":
                    assert m.prelaid() and s["k"] % 4 == 0 and s["gap"] > 0
            assert s["readings"] == m.readings()
        calls = _calls(w)
        assert sum(c["kind"] == "wide" for c in calls) == 1, (f, seed)
        assert len({c["bseed"] for c in calls}) == len(calls)
        assert sum(s["op"] == "reconf" and s["name"] == "autotune" for s in w["steps"]) <= 1
    seeds = [c["bseed"] for w in _all() for c in _calls(w)]
    assert len(set(seeds)) == len(seeds)
    fresh = dict(sp._SCHEDULE)
    sp._SCHEDULE.clear()
    assert sp.describe(sp.walk(3, "weighted"), 99) == sp.describe(fresh["weighted"][3], 99)
    sp._SCHEDULE.update(fresh)


@pytest.mark.parametrize("family", sp.FAMILIES)
def test_the_seed_count_is_the_smallest(family):
    assert sp.walk(SEEDS[family] - 1, family)["owed"] == 0
    assert sp.walk(SEEDS[family] - 2, family)["owed"] > 0
    assert family != "auto" or SEEDS[family] <= 3


@pytest.mark.parametrize("family", sp.FAMILIES)
def test_every_reconfiguration_and_refusal_in_every_family(family):
    steps = [s for w in _all(family) for s in w["steps"] if s["op"] == "reconf"]
    ok = {s["name"] for s in steps if s["expect"] == "ok"}
    want = {"enable_slicing", "enable_panels", "set_value_factors", "set_tile_cols", "set_gather_width", "set_blocks_per_cu",
            "prepare_width", "autotune"}
    assert want <= ok, want - ok
    got = {(s["name"], s["arg"], s["expect"]) for s in steps}
    assert ("set_value_factors", None, "ok") in got
    for name, arg in (("set_tile_cols", 100), ("set_gather_width", 2), ("set_blocks_per_cu", 0), ("set_blocks_per_cu", 65),
                      ("enable_slicing", 1025)):
        assert (name, arg, "refused") in got, (name, arg)
    if family == "mutable":
        assert "update_values" in ok and ("enable_panels", 1, "refused") in got
        assert ("set_value_factors", "ok", "refused_rebuilt") in got
    else:
        assert ("update_values", None, "refused") in got
    if family in sp.NATIVE_FACTORS:
        assert ("set_value_factors", "ok", "ok") in got and ("set_value_factors", "doubled", "refused_rebuilt") in got


def test_every_listed_argument_occurs():
    got = {(s["name"], s["arg"]) for w in _all() for s in w["steps"] if s["op"] == "reconf" and s["expect"] == "ok"}
    for name, values in (("enable_slicing", sp.SLICE_COUNTS), ("enable_panels", sp.PANEL_MODES), ("set_tile_cols", sp.TILE_COLS),
                         ("set_gather_width", sp.GATHER_WIDTHS), ("set_blocks_per_cu", sp.BLOCKS_PER_CU)):
        assert {(name, v) for v in values} <= got, (name, {v for v in values if (name, v) not in got})
    assert {("prepare_width", 16), ("prepare_width", 64)} <= got


def test_every_ordered_pair_of_plan_states():
    """all 49: every state can follow every state (and itself) within one family — value_free reaches all seven"""
    got = {(a["state"], b["state"]) for _w, a, b, _r in _call_pairs()}
    want = {(a, b) for a in sp.STATES for b in sp.STATES}
    assert want <= got, sorted(want - got)
    # the state of the issue's example: sliced while the panels were on, panels off again, with factors (16-bit columns)
    assert any(b["state"] == "after_panels" and w["family"] == "value_free" and b["kind"] == "spmm" and b["k"] >= 33
               for w, _a, b, _r in _call_pairs())


def test_width_classes_dtypes_and_epilogues():
    got, dt = set(), set()
    for _w, a, b, _r in _call_pairs():
        if a["k"] != b["k"]:
            got.add((sp.width_class(b["k"]), "wider" if b["k"] < a["k"] else "narrower"))
        dt.add((a["dtype"], b["dtype"]))
    want = {(c, d) for c in sp.WIDTH_CLASSES for d in ("wider", "narrower")}
    assert want <= got, sorted(want - got)
    assert {("fp32", "bf16"), ("bf16", "fp32")} <= dt
    calls = [c for w in _all() for c in _calls(w)]
    epi = {(c["state"], c["epi"]) for c in calls if c["kind"] == "spmm"}
    want = {(s, e) for s in sp.STATES for e in range(len(util.EPILOGUES))}
    assert want <= epi, sorted(want - epi)
    assert {c["k"] for c in calls if c["kind"] in ("spmm", "wide")} >= set(sp.FP32_WIDTHS)
    assert {c["k"] for c in calls if c["kind"] == "bf16"} == set(sp.BF16_WIDTHS)
    assert {c["out"] for c in calls if c["kind"] == "bf16"} == {"fp32", "bf16"}
    assert {c["kind"] for c in calls} == {"spmm", "bf16", "prelaid", "sddmm", "transpose", "backward", "wide"}
    assert any(c["kind"] == "backward" for w in _all("mutable") for c in _calls(w))


def test_sddmm_and_narrow_calls_on_both_sides_of_a_reslicing():
    for family in sp.FAMILIES:                           # a sliced SDDMM (k >= 33), another slice count, a sliced SDDMM again
        assert any(a["kind"] == b["kind"] == "sddmm" and a["k"] == b["k"] == 64 and a["readings"]["S"] > 1 and b["readings"]["S"] > 1
                   and a["readings"]["S"] != b["readings"]["S"] and any(r["name"] == "enable_slicing" for r in between)
                   for _w, a, b, between in _call_pairs(family)), family
    narrow = lambda c: c["kind"] == "spmm" and 12 <= c["k"] <= 32
    for count in (8, -1):
        assert any(narrow(a) and narrow(b) and [(r["name"], r["arg"]) for r in between] == [("enable_slicing", count)]
                   for _w, a, b, between in _call_pairs("auto")), count
    assert any(c["builds_narrow"] for w in _all("auto") for c in _calls(w))


REBUILDS = ("enable_slicing", "set_value_factors", "enable_panels", "update_values")


@pytest.mark.parametrize("family", sp.FAMILIES[:4])
def test_what_a_reconfiguration_rebuilt_is_used_by_the_next_call(family):
    """every call that replaces streams, values or panels is somewhere the last such call before a forward product of at
    least 33 columns — the widths at which the sliced copy, the streams and the panels are what runs"""
    used, made = set(), set()
    for w in _all(family):
        last = []
        for s in w["steps"]:
            key = (s.get("name"), "S>1" if s.get("name") == "enable_slicing" and s["arg"] > 1 else s.get("arg"))
            if s["op"] == "reconf" and s["name"] in REBUILDS and s["expect"] != "refused":
                last.append(key)
                made.add(key)
            elif s["op"] == "call":
                if s["kind"] in ("spmm", "bf16", "wide", "prelaid", "backward") and s["k"] >= 33:
                    used.update(last)
                last = []
    assert made <= used, sorted(made - used, key=str)
    assert ("enable_slicing", "S>1") in made and ("enable_slicing", 0) in made


def test_mutable_values_change_under_the_streams():
    """update_values on a sliced plan between two calls that read the weighted group stream; a bf16 call after one; the
    backward while sliced (its SDDMM walks the sliced copy at k = 64), and again after an update made its transpose stale"""
    group = lambda c, kinds: c["state"] == "group" and c["kind"] in kinds and c["k"] >= 12
    update = lambda between: [r["name"] for r in between] == ["update_values"] and between[0]["expect"] == "ok"
    pairs = list(_call_pairs("mutable"))
    assert any(group(a, ("spmm",)) and group(b, ("spmm",)) and update(r) and a["values"] != b["values"] for _w, a, b, r in pairs)
    assert any(group(b, ("bf16",)) and update(r) for _w, _a, b, r in pairs)
    assert any(group(a, ("backward",)) and a["k"] == 64 and group(b, ("backward",)) and update(r) for _w, a, b, r in pairs)
    assert any(c["kind"] == "backward" and c["state"] != "group" for w in _all("mutable") for c in _calls(w))
    values = {s["vseed"] for w in _all("mutable") for s in w["steps"] if "vseed" in s}
    assert len(values) >= 8


def _dominating(o, va):
    """util.assert_exact_inputs on the operands that dominate every call's: |B| <= 8 and |bias| <= 8 element-wise, so
    |A|.|B| + |bias| of any call is at most that of B = 8, bias = 8; the dropout scale 2"""
    return util.assert_exact_inputs(o["rp"], o["ci"], va, np.full((o["n"], 1), 8.0, np.float32), extra=np.array([8.0], np.float32), scale=2.0)


def test_every_operand_set_is_exact():
    done = set()
    for w in _all():
        o = w["ops"]
        for s in w["steps"]:
            vseed = s.get("values", s.get("vseed"))
            key = (w["pattern"], vseed if w["mutable"] else None)
            if vseed is None or key in done:
                continue
            done.add(key)
            _dominating(o, sp.values_of(w, vseed))
            if s["op"] == "call" and s["kind"] in ("transpose", "backward"):      # the transpose's rows are the columns
                At = sp_.csr_matrix((np.abs(sp.values_of(w, vseed)).astype(np.float64), o["ci"], o["rp"]), shape=(o["m"], o["n"])).T
                assert float(np.asarray(At.sum(1)).max()) * 8 * 2.0 ** 6 < 2.0 ** 24
        for c in _calls(w):
            rows = o["m"] if c["kind"] in ("transpose", "backward") else o["n"]
            if c["kind"] != "wide":
                B = sp.features(c, rows)
                assert np.array_equal(B, np.rint(B)) and np.abs(B).max() <= 8
            bias = sp.epilogue_of(c)[0]
            assert bias is None or (np.array_equal(bias, np.rint(bias)) and np.abs(bias).max() <= 8)
    assert any(k[1] is not None for k in done) and len([k for k in done if k[0] == ("group", "int")]) >= 5


def test_consecutive_references_differ_in_every_non_empty_row():
    """the raw products A.B of two consecutive forward calls, on their common leading columns (at most 16: enough to tell
    them apart, and what differs there differs in the whole row)"""
    checked = 0
    for w, a, b, _r in _call_pairs():
        forward = ("spmm", "bf16", "prelaid", "wide")
        if w["family"] == "auto" or a["kind"] not in forward or b["kind"] not in forward or "wide" in (a["kind"], b["kind"]):
            continue
        o, k = w["ops"], min(a["k"], b["k"], 16)
        refs = [util.oracle_spmm(o["rp"], o["ci"], sp.values_of(w, c["values"]), np.ascontiguousarray(sp.features(c, o["n"])[:, :k]))
                for c in (a, b)]
        same = (refs[0] == refs[1]).all(axis=1) & (np.diff(o["rp"]) > 0)
        assert not same.any(), (w["family"], w["seed"], a["bseed"], b["bseed"], np.flatnonzero(same)[:5])
        checked += 1
    assert checked >= 40
    for w in _all("auto"):                               # (4.5 M entries: the features alone — different in every row)
        calls = [c for c in _calls(w) if c["kind"] in ("spmm", "bf16", "prelaid")]
        for a, b in zip(calls, calls[1:]):
            k = min(a["k"], b["k"])
            assert (sp.features(a, 64)[:, :k] != sp.features(b, 64)[:, :k]).any(axis=1).all()
