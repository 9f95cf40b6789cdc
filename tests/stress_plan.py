"""The generator of the seeded walks over an SpMM plan's reconfigurations (tests/test_stress_plan_cpu.py proves their
coverage without a GPU, tests/test_stress_plan_gpu.py runs them): ``walk(seed, family)`` returns, deterministically from
(family, seed), an operand set and 10 to 14 steps that all run on ONE CsrAdjacency.  A step is a reconfiguration (name,
argument, expected outcome) or a product call (kind, width, dtype, epilogue, the seed of its own B).

The generator keeps a model of the plan (``Model``: what plan_build.cpp drops, keeps and rebuilds at every call — slice
count, automatic or explicit, factors, panels, which stream the last rebuild left) and draws every step subject to it; the
GPU test compares the model with the plan's own answers after every step.  The walks are guided, not uniform: a family owns
a share of what the sweep has to cover (ordered pairs of plan states, epilogue x state, width class after a wider / narrower
call, every reconfiguration and refusal) and a walk steers to what its family still owes, so few seeds suffice.

Operands are util.exact_operands: every sum is exact in fp32 in any order, so every result must EQUAL its reference."""
import copy

import numpy as np

import util

FAMILIES = ("value_free", "weighted", "panels", "mutable", "auto")
STATES = ("unsliced", "group", "under_panels", "panels", "after_panels", "automatic", "forgotten")
LEGAL = {"value_free": STATES, "weighted": STATES[:6], "panels": STATES[:6], "mutable": ("unsliced", "group", "automatic"),
         "auto": STATES}
NATIVE_FACTORS = ("value_free", "auto")                  # families whose values are u[r] * u[c] with a stored diagonal
SLICE_COUNTS = (-1, 0, 2, 3, 5, 8, 16)
PANEL_MODES = (0, 1, -1)
TILE_COLS = (0, 64, 128, 256)
GATHER_WIDTHS = (0, 1, 4)
BLOCKS_PER_CU = (1, 4, 8, 32, 64)
FP32_WIDTHS = (4, 8, 16, 20, 32, 36, 41, 64, 100, 128, 200, 256)
BF16_WIDTHS = (64, 128, 200, 320)
WIDTH_CLASSES = ("le8", "12_32", "odd", "33_48", "64", "partial", "256")
# refusals that change nothing / that rebuild the streams on their way out
REFUSED_PLAIN = {"tile100": ("set_tile_cols", 100), "gather2": ("set_gather_width", 2), "bpc0": ("set_blocks_per_cu", 0),
                 "bpc65": ("set_blocks_per_cu", 65), "slicing1025": ("enable_slicing", 1025),
                 "update_fixed": ("update_values", None), "panels_mutable": ("enable_panels", 1)}
REBUILDS = ("enable_slicing", "set_value_factors", "enable_panels", "update_values")   # replace streams, values or panels
MAX_STEPS, MIN_STEPS, MAX_SEEDS = 14, 10, 16
L2_BYTES = 4 << 20


def width_class(k):
    if k <= 8:
        return "le8"
    if k % 4:
        return "odd"
    if k <= 32:
        return "12_32"
    if k <= 48:
        return "33_48"
    if k == 64:
        return "64"
    if k == 256:
        return "256"
    return "partial" if k % 64 else None


def auto_slices(m, n, nnz, value_free):
    """plan_policy.cpp, auto_slices (the CPU test compares it with gcn_spmm_auto_slices on the shapes used)"""
    if m <= 0 or nnz <= 0 or nnz // m < 128:
        return 0
    table = n * 256
    if table <= L2_BYTES:
        return 0
    if value_free:
        S = -(-table // L2_BYTES)
        narrow = (n + 32766) // 32767
        S = max(S, narrow)
        if S > 8:
            S = min(S, nnz // m // 16)
            if 8 < S <= 1024 and S >= narrow and table // S <= 2 * L2_BYTES:
                return S
    S = 2
    while S < 8 and table // S > L2_BYTES:
        S *= 2
    while S > 1 and nnz // m // S < 16:
        S //= 2
    if S < 2 or table // S > (64 << 20):
        return 0
    return S


def narrow_slices(m, n, nnz, S):
    """plan_build.cpp, maybe_build_alt: the slices of the k <= 32 set of a value-free plan on S automatic slices, 0: none"""
    S2 = max(-(-n * 128 // L2_BYTES), (n + 32766) // 32767)
    S2 = min(S2, nnz // m // 16)
    if S2 < 2 or S2 + 2 > S or -(-n // S2) > 32767:
        return 0
    return S2


def panel_coverage(rp, ci, m, n):
    """spmm_panel.hip, panel_windows_kernel: the share of the entries inside the best run of four 128-column bins of their
    128-row panel (what enable_panels(-1) decides from: panels from 0.5 on)"""
    R, W, BIN = 128, 512, 128
    rows = np.repeat(np.arange(m), np.diff(rp))
    panel, nbins, npanels = rows // R, -(-n // BIN), -(-m // R)
    hist = np.bincount(panel * nbins + ci // BIN, minlength=npanels * nbins).reshape(npanels, nbins).astype(np.int64)
    csum = np.concatenate([np.zeros((npanels, 1), np.int64), np.cumsum(hist, axis=1)], axis=1)
    b = np.arange(nbins)
    run = csum[:, b + 1] - csum[:, np.maximum(0, b - 3)]
    best_b = run.argmax(axis=1)                          # (the first maximum, as the kernel's strict > keeps it)
    w0 = np.minimum(np.maximum(0, best_b - 3) * BIN, max(0, n - W))
    inside = (ci - w0[panel] >= 0) & (ci - w0[panel] < W)
    return float(inside.sum()) / max(1, len(ci))


_OPERANDS, _COVERAGE = {}, {}


def family_pattern(family, seed):
    if family == "value_free":
        return "group_diag", "pow2"
    if family == "weighted":
        return "unsliced", "int"
    if family == "panels":
        return ("lds", "mfma")[seed % 2], "int"
    if family == "mutable":
        return "group", "int"
    return "auto_diag", "pow2"


def operands(family, seed):
    key = family_pattern(family, seed)
    if key not in _OPERANDS:
        _OPERANDS[key] = util.exact_operands(*key)
    return _OPERANDS[key]


def coverage_of(family, seed):
    key = family_pattern(family, seed)
    if key not in _COVERAGE:
        o = operands(family, seed)
        _COVERAGE[key] = panel_coverage(o["rp"], o["ci"], o["m"], o["n"])
    return _COVERAGE[key]


class Model:
    """what the plan holds after every call, from plan_build.cpp; `stream`: what the last rebuild of the sliced streams left
    ("group_vf", "group_w", "col16" or "none" — the virtual CSR alone)"""

    def __init__(self, family, seed):
        o = operands(family, seed)
        self.family, self.m, self.n, self.nnz = family, o["m"], o["n"], len(o["ci"])
        self.native = family in NATIVE_FACTORS
        self.mutable = family == "mutable"
        self.coverage = coverage_of(family, seed)
        self.S, self.auto, self.factors, self.panels, self.stream, self.unknown = 0, False, False, False, "none", False
        self.apply("enable_slicing", -1 if family == "auto" else 0)       # the constructor's slices= argument

    def _build_streams(self):
        if self.S <= 1 or self.stream != "none" or (self.panels and not self.factors):
            return
        w = -(-self.n // self.S)
        assert w <= 32767
        if not self.panels:
            self.stream = "group_vf" if self.factors and self.nnz // self.n >= 48 else "group_w"
        elif self.S <= 8:
            self.stream = "col16"

    def apply(self, name, arg):
        """-> "ok", "refused" (nothing changed) or "refused_rebuilt" (factors gone, streams built again)"""
        if name == "enable_slicing":
            if arg > 1024:
                return "refused"
            self.auto, self.S, self.stream, self.unknown = arg == -1, 0, "none", False
            if arg in (0, 1):
                return "ok"
            if self.m == self.n and not self.factors and not self.mutable and (
                    arg != -1 or auto_slices(self.m, self.n, self.nnz, False) > 1):
                self.factors = self.native               # (integer values do not factor, and none is row- or column-constant)
            S = arg if arg != -1 else auto_slices(self.m, self.n, self.nnz, not self.panels)
            if S > 1:
                self.S = S
                self._build_streams()
            return "ok"
        if name == "set_value_factors":
            if arg == "ok" and not self.mutable:
                assert self.native
                self.factors, self.stream = True, "none"
                if self.auto and auto_slices(self.m, self.n, self.nnz, not self.panels) != self.S:
                    return self.apply("enable_slicing", -1)
                self._build_streams()
                return "ok"
            self.factors, self.stream = False, "none"
            self._build_streams()
            return "ok" if arg is None else "refused_rebuilt"
        if name == "enable_panels":
            if self.mutable and arg != 0:
                return "refused"
            self.panels = arg == 1 or (arg == -1 and self.coverage >= 0.5)
            return "ok"
        if name == "set_tile_cols":
            return "ok" if arg in TILE_COLS else "refused"
        if name == "set_gather_width":
            return "ok" if arg in GATHER_WIDTHS else "refused"
        if name == "set_blocks_per_cu":
            return "ok" if 1 <= arg <= 64 else "refused"
        if name == "update_values":
            return "ok" if self.mutable else "refused"
        if name == "prepare_width":
            return "ok"
        if name == "autotune":                           # enable_slicing(-1), (8), (0), then the fastest: not the model's to know
            if self.m == self.n and not self.mutable:
                self.factors = self.factors or self.native
            self.unknown, self.stream = True, "none"
            return "ok"
        raise KeyError(name)

    def state(self):
        if self.unknown:
            return None
        if self.panels:
            return "under_panels" if self.S > 0 else "panels"
        if self.S > 0 and not self.stream.startswith("group"):
            return "after_panels"
        if self.S > 0 and self.native and not self.factors:
            return "forgotten"
        if self.auto:
            return "automatic"
        return "group" if self.S > 0 else "unsliced"

    def readings(self):
        """what the plan must answer: (num_slices, has_value_factors, panel_rows > 0, slice count automatic)"""
        return None if self.unknown else dict(S=self.S, factors=self.factors, panels=self.panels, auto=self.auto)

    def prelaid(self):
        return not self.unknown and not self.panels and self.stream == "group_vf"


def _owner(index, families):
    return families[index % len(families)]


def _needs(family):
    """what the walks of `family` owe the sweep"""
    small = FAMILIES[:4]
    need = dict(pairs=[], epi=[], width=[], names=[], args=[], rebuilt=set())
    for ia, a in enumerate(STATES):
        for ib, b in enumerate(STATES):
            cands = [f for f in small if a in LEGAL[f] and b in LEGAL[f] and (f != "value_free" or "forgotten" in (a, b))]
            cands = ["mutable"] if "mutable" in cands else cands         # (its walks have no panels to move in and out of)
            if _owner(ia * 7 + ib, cands) == family:
                need["pairs"].append((a, b))
    for ia, a in enumerate(STATES):
        for e in range(len(util.EPILOGUES)):
            cands = [f for f in small if a in LEGAL[f] and (f != "value_free" or a == "forgotten")]
            if _owner(ia + e, ["mutable"] if "mutable" in cands else cands) == family:
                need["epi"].append((a, e))
    for ic, c in enumerate(WIDTH_CLASSES):
        for idr, d in enumerate(("wider", "narrower")):
            if _owner(2 * ic + idr, small) == family:
                need["width"].append((c, d))
    names = ["set_value_factors:None", "set_tile_cols", "set_gather_width", "set_blocks_per_cu", "prepare_width",
             "tile100", "gather2", "bpc0", "bpc65", "slicing1025"]
    if family == "mutable":
        names += ["update_values", "panels_mutable", "svf_mutable", "enable_panels:0"]
    else:
        names += ["update_fixed"]
    if family in NATIVE_FACTORS:
        names += ["set_value_factors:ok", "svf_doubled"]
    need["names"] = names
    mine = lambda vals, off: [v for i, v in enumerate(vals) if family == "auto" or _owner(i + off, small) == family]
    need["args"] = ([("enable_slicing", s) for s in mine(SLICE_COUNTS, 0)] + [("set_tile_cols", t) for t in mine(TILE_COLS, 1)] +
                    [("set_gather_width", g) for g in mine(GATHER_WIDTHS, 2)] + [("set_blocks_per_cu", b) for b in mine(BLOCKS_PER_CU, 3)] +
                    [("enable_panels", p) for p in mine(PANEL_MODES, 0) if family != "mutable"])
    if family == "auto":                                 # (three seeds: the settings' values are the small families' to cover)
        need["pairs"], need["args"] = [], []
    return need


class _Builder:
    """one walk: steps are appended while the model follows"""

    def __init__(self, family, seed, need):
        self.family, self.seed, self.need = family, seed, need
        self.rng = np.random.default_rng([seed, FAMILIES.index(family), 20260])
        self.model = Model(family, seed)
        self.steps, self.last_state, self.last_k, self.ncalls, self.wide_done, self.pending = [], None, None, 0, False, []
        self.values = 100                                # the value seed in force (util.int_values; mutable family)

    # ---- reconfigurations ----
    def reconf(self, name, arg):
        m = self.model
        args = list(self.need["args"])
        out = m.apply(name, arg)
        step = dict(op="reconf", name=name, arg=arg, expect=out, readings=m.readings())
        if name == "update_values" and out == "ok":
            self.values = step["vseed"] = 7000 + 100 * self.seed + len(self.steps)
        if name == "update_values" and out != "ok":
            step["vseed"] = 7000
        self.steps.append(step)
        if name in REBUILDS and out != "refused":        # what the next call should run on: see call()
            self.pending.append((name, "S>1" if name == "enable_slicing" and arg > 1 else arg))
        if (name, arg) in args:
            self.need["args"].remove((name, arg))
        for key in (name, f"{name}:{arg}"):
            if key in self.need["names"] and out == "ok":
                self.need["names"].remove(key)
        return out

    def pick(self, name, values):
        """an argument the family still owes, else a drawn one"""
        owed = [a for n, a in self.need["args"] if n == name and a in values]
        return owed[0] if owed else values[int(self.rng.integers(len(values)))]

    def explicit(self):
        return self.pick("enable_slicing", [s for s in SLICE_COUNTS if s >= 2])

    def panels_off(self):
        if self.model.panels:
            self.reconf("enable_panels", self.pick("enable_panels", [0] + ([-1] if self.model.coverage < 0.5 and not self.model.mutable else [])))

    def panels_on(self):
        if not self.model.panels:
            self.reconf("enable_panels", self.pick("enable_panels", [1] + ([-1] if self.model.coverage >= 0.5 else [])))

    def goto(self, target):
        m, rng = self.model, self.rng
        if m.unknown:                                    # after autotune: an explicit configuration makes the plan known again
            self.reconf("enable_slicing", 0 if target in ("unsliced", "panels") else -1 if target == "automatic" else self.explicit())
            self.reconf("set_tile_cols", self.pick("set_tile_cols", list(TILE_COLS)))
        if m.state() == target:
            return
        if target in ("unsliced", "automatic", "group", "forgotten"):
            self.panels_off()
            if target == "unsliced":
                self.reconf("enable_slicing", self.pick("enable_slicing", [0]))
            elif target == "automatic":
                if not m.auto or m.state() != "automatic":
                    self.reconf("enable_slicing", -1)
            elif target == "group":
                if m.state() == "forgotten" and not m.auto and rng.random() < 0.5:
                    self.reconf("set_value_factors", "ok")
                else:
                    self.reconf("enable_slicing", self.explicit())
            else:
                if not (m.S > 0 and m.stream.startswith("group")):
                    self.reconf("enable_slicing", self.explicit())
                if m.factors:
                    if "svf_doubled" in self.need["names"]:
                        self.need["names"].remove("svf_doubled")
                        self.reconf("set_value_factors", "doubled")
                    else:
                        self.reconf("set_value_factors", None if rng.random() < 0.7 else "doubled")
        elif target == "panels":
            if m.S > 0 and rng.random() < 0.5:
                self.reconf("enable_slicing", 0)
            self.panels_on()
            if m.S > 0:
                self.reconf("enable_slicing", 0)
        elif target == "under_panels":
            if m.S > 0 and not m.panels and rng.random() < 0.5:
                self.panels_on()                         # (whatever stream the plan has stays beside the panels)
            else:
                self.panels_on()
                self.reconf("enable_slicing", self.explicit())
        elif target == "after_panels":
            self.panels_on()
            if m.S == 0 or m.stream.startswith("group") or rng.random() < 0.5:
                self.reconf("enable_slicing", self.explicit())           # sliced while the panels are on: no group stream
            self.reconf("enable_panels", 0)
        assert m.state() == target, (self.family, self.seed, target, m.state(), m.__dict__)

    def extra(self):
        """one more reconfiguration that leaves the state's class alone: what the family still owes first"""
        m, rng, names = self.model, self.rng, self.need["names"]
        cand = []
        for key in names:
            if key in REFUSED_PLAIN:
                cand.append(REFUSED_PLAIN[key])
            elif key == "svf_mutable":
                cand.append(("set_value_factors", "ok"))
            elif key == "set_value_factors:None":
                cand.append(("set_value_factors", None))
            elif key == "set_value_factors:ok":
                cand.append(("set_value_factors", "ok"))
            elif key == "enable_panels:0":
                cand.append(("enable_panels", 0))
            elif key == "prepare_width":
                cand.append(("prepare_width", (16, 64)[int(rng.integers(2))]))
            elif key == "update_values":
                cand.append(("update_values", None))
            elif key in ("set_tile_cols", "set_gather_width", "set_blocks_per_cu"):
                cand.append((key, self.pick(key, list(dict(set_tile_cols=TILE_COLS, set_gather_width=GATHER_WIDTHS,
                                                           set_blocks_per_cu=BLOCKS_PER_CU)[key]))))
        cand += [(n, a) for n, a in self.need["args"] if n.startswith("set_")]
        if not cand and not m.native:                    # (made before, but no wide forward call has run on it yet)
            cand = [c for c in (("set_value_factors", None), ("enable_panels", 0)) if c not in self.need["rebuilt"] and
                    (c[0] != "enable_panels" or m.mutable)]
        if not cand and m.mutable and m.S > 1 and rng.random() < 0.5:
            cand = [("update_values", None)]             # (fresh values under the streams that hold copies of them)
        if not cand:
            if rng.random() < (0.75 if self.need["pairs"] or self.need["epi"] else 0.4):
                return
            n = ("set_tile_cols", "set_gather_width", "set_blocks_per_cu", "prepare_width")[int(rng.integers(4))]
            vals = dict(set_tile_cols=TILE_COLS, set_gather_width=GATHER_WIDTHS, set_blocks_per_cu=BLOCKS_PER_CU, prepare_width=(16, 64))[n]
            cand = [(n, vals[int(rng.integers(len(vals)))])]
            if m.mutable:
                cand.append(("update_values", None))
        for name, arg in cand:
            trial = copy.copy(m)
            trial.apply(name, arg)
            if trial.state() == m.state():
                out = self.reconf(name, arg)
                for key, na in list(REFUSED_PLAIN.items()) + [("svf_mutable", ("set_value_factors", "ok"))]:
                    if na == (name, arg) and key in names and out != "ok":
                        names.remove(key)
                return

    # ---- product calls ----
    def call(self, kind=None, k=None, epi="draw", kernel=None):
        m, rng, need = self.model, self.rng, self.need
        state = m.state()
        # a reconfiguration that replaced streams, values or panels, not yet followed by a forward call of >= 33 columns
        fresh = [p for p in self.pending if p not in need["rebuilt"]]
        if kind is None:
            kinds, w = ["spmm", "bf16", "sddmm", "transpose"], [6, 2, 0 if fresh else 1, 0 if fresh else 3 if m.mutable else 1]
            if self.ncalls >= 1 and not self.wide_done:
                kinds, w = ["wide"], [1]
            elif m.prelaid():
                kinds, w = kinds + ["prelaid"], w + [3]
            if state is not None and any(s == state for s, _e in need["epi"]):
                w[0] += 6
            kind = kinds[int(rng.choice(len(kinds), p=np.array(w) / sum(w)))]
        if kind == "transpose" and m.mutable:
            kind = "backward"
        step = dict(op="call", kind=kind, dtype="fp32", out="fp32", epi=None, state=state, readings=m.readings(),
                    bseed=100000 * (FAMILIES.index(self.family) + 1) + 1000 * self.seed + 10 * len(self.steps))
        if kind == "bf16":
            step["dtype"] = "bf16"
            step["out"] = ("fp32", "bf16")[int(rng.integers(2))]
            widths = BF16_WIDTHS
        elif kind == "prelaid":
            widths = (16, 32, 64, 128)
        elif kind == "sddmm":
            widths = (16, 64)
        elif kind in ("wide", "transpose", "backward"):
            widths = (16, 41, 64, 100) if kind != "backward" else (16, 64)
        else:
            widths = FP32_WIDTHS
        if k is None:
            k = widths[int(rng.integers(len(widths)))]
            if self.last_k is not None:                  # a width class the family still owes after a wider / narrower call
                for c, d in need["width"]:
                    fit = [x for x in widths if width_class(x) == c and (x < self.last_k if d == "wider" else x > self.last_k)]
                    if fit:
                        k = fit[int(rng.integers(len(fit)))]
                        break
                else:                                    # none fits after the last width: the width that lets the first one fit next
                    if need["width"]:
                        k = max(widths) if need["width"][0][1] == "wider" else min(widths)
            if fresh and k < 33:
                wide = [x for x in widths if x >= 33]
                k = wide[int(rng.integers(len(wide)))]
        step["k"], step["kernel"] = k, kernel
        if kind in ("spmm", "bf16"):
            if epi == "draw":
                owed = [e for s, e in need["epi"] if s == state] if kind == "spmm" else []
                epi = owed[0] if owed else (None, int(rng.integers(len(util.EPILOGUES))))[int(rng.random() < 0.4)]
            step["epi"] = epi
        if kind == "prelaid":
            step["gap"] = int(rng.integers(100, 3000))
        if kind == "backward":
            self.values = step["vseed"] = 7000 + 100 * self.seed + len(self.steps)
        step["values"] = self.values
        fam_narrow = self.family == "auto" and m.auto and m.stream == "group_vf" and not m.panels
        step["builds_narrow"] = bool(fam_narrow and ((kind in ("spmm", "wide") and 12 <= k <= 32 and k % 4 == 0) or
                                                     (kind == "bf16" and k == 64)))
        self.steps.append(step)
        if state is not None and self.last_state is not None and (self.last_state, state) in need["pairs"]:
            need["pairs"].remove((self.last_state, state))
        if kind == "spmm" and (state, epi) in need["epi"]:
            need["epi"].remove((state, epi))
        if self.last_k is not None and k != self.last_k:
            key = (width_class(k), "wider" if k < self.last_k else "narrower")
            if key in need["width"]:
                need["width"].remove(key)
        if kind in ("spmm", "bf16", "wide", "prelaid", "backward") and k >= 33:
            need["rebuilt"].update(self.pending)
        self.pending = []
        self.last_state, self.last_k, self.ncalls = state, k, self.ncalls + 1
        self.wide_done = self.wide_done or kind == "wide"

    def next_target(self):
        legal, need, rng = LEGAL[self.family], self.need, self.rng
        owed = [b for a, b in need["pairs"] if a == self.last_state]
        if owed:                                         # the owed pair that takes the fewest reconfigurations
            cost = []
            for b in owed:
                keep = self.snapshot()
                self.goto(b)
                cost.append(len(self.steps))
                self.restore(keep)
            return owed[int(np.argmin(cost))]
        if need["pairs"]:
            return need["pairs"][0][0]
        owed = [s for s, _e in need["epi"]]
        if owed:
            return owed[0]
        return legal[int(rng.integers(len(legal)))]

    def snapshot(self):
        return (len(self.steps), copy.copy(self.model), copy.deepcopy(self.need), self.values, self.rng.bit_generator.state)

    def restore(self, keep):
        del self.steps[keep[0]:]
        self.model, self.values = keep[1], keep[3]
        self.need.clear()
        self.need.update(keep[2])
        self.rng.bit_generator.state = keep[4]

    def segment(self, target, **call):
        """the steps to `target`, one extra reconfiguration, a product call — taken back when the walk would grow too long"""
        keep = self.snapshot()
        self.goto(target)
        self.extra()
        if self.family == "auto" and self.need["names"]:   # (three seeds for its share of the refusals: two at a time)
            self.extra()
        if len(self.steps) + 1 > MAX_STEPS:
            self.restore(keep)
            return False
        self.call(**call)
        return True


def _scripted(b):
    """the parts of a family's walks that are written out: autotune once, an SDDMM on both sides of a re-slicing, and in the
    `auto` family a narrow call on both sides of enable_slicing(8) and enable_slicing(-1), the plan of the 16-bit column stream"""
    f, seed = b.family, b.seed
    if seed == 0:
        b.segment("group", kind="sddmm", k=64)
        b.reconf("enable_slicing", 5 if b.model.S != 5 else 3)
        b.goto("group")
        b.call(kind="sddmm", k=64)
        b.call()                                         # (the walk's bound-checked call)
        b.call(kind="sddmm", k=16)
        if f in NATIVE_FACTORS:                          # the pre-laid entry on both sides of a re-slicing: the layout follows
            b.call(kind="prelaid", k=64)
        if f == "value_free":
            b.reconf("enable_slicing", 2 if b.model.S != 2 else 3)
            b.call(kind="prelaid", k=16)
    if f == "value_free" and seed == 2:                  # sliced under panels with factors, panels off: the four-per-gather
        b.panels_on()                                    # kernel on 16-bit columns in slices of 2000 (elsewhere: 35 000)
        b.reconf("enable_slicing", 3)
        b.reconf("enable_panels", 0)
        b.reconf("set_gather_width", 4)
        b.reconf("set_tile_cols", 0)
        b.call(kind="spmm", k=64, epi=None, kernel="gcn::spmm_quad_kernel<16, false, true, true>")
        b.call()
        b.call(kind="spmm", k=200)
    if f == "mutable" and seed == 2:                     # fresh values under a weighted group stream, on both sides of calls
        b.segment("group", kind="spmm", k=64)            # that read them; the backward while sliced, its transpose gone stale
        b.reconf("update_values", None)
        b.call(kind="spmm", k=64, epi=None)
        b.call()
        b.reconf("update_values", None)
        b.call(kind="bf16", k=128)
        b.call(kind="backward", k=64)
        b.reconf("update_values", None)
        b.call(kind="backward", k=16)
        b.reconf("enable_slicing", 8 if b.model.S != 8 else 3)
        b.call(kind="spmm", k=100)
    if f == "auto" and seed == 1:
        b.segment("automatic", kind="spmm", k=16)
        b.reconf("enable_slicing", 8)
        b.call(kind="spmm", k=32)
        b.reconf("enable_slicing", -1)
        b.call(kind="spmm", k=20)
        b.call()
        b.reconf("prepare_width", 16)
        b.call(kind="bf16", k=64)
    if seed == (2 if f == "auto" else 1):
        b.segment(b.next_target())
        b.call()
        b.reconf("autotune", (64, 128, 200)[FAMILIES.index(f) % 3])
        b.call(kind="spmm")                              # in whatever shape the timing kept: checked, its state not modelled


_SCHEDULE = {}


def _schedule(family):
    if family not in _SCHEDULE:
        need, walks = _needs(family), []
        for seed in range(MAX_SEEDS):
            b = _Builder(family, seed, need)
            _scripted(b)
            fails = 0
            while len(b.steps) < MAX_STEPS - 1 and fails < 6:
                if not b.segment(b.next_target()):
                    fails += 1
                    if fails >= 3 and len(b.steps) < MAX_STEPS:      # no room for a move: calls in the state the plan is in
                        if b.model.unknown:
                            break
                        b.call()
            while len(b.steps) < MIN_STEPS:
                b.call()
            assert MIN_STEPS <= len(b.steps) <= MAX_STEPS, (family, seed, len(b.steps))
            o = operands(family, seed)
            walks.append(dict(family=family, seed=seed, pattern=family_pattern(family, seed), ops=o, steps=b.steps,
                              mutable=family == "mutable", side_stream=bool(seed % 2),
                              owed=sum(len(v) for key, v in need.items() if key != "rebuilt")))
        _SCHEDULE[family] = walks
    return _SCHEDULE[family]


def walk(seed, family):
    """-> dict(family, seed, pattern, ops (util.exact_operands), steps, mutable, side_stream, owed: what the family still
    owes the sweep after this walk — 0 from the seed on that completes its share)"""
    assert 0 <= seed < MAX_SEEDS
    return _schedule(family)[seed]


# ---- the operands of a step, the same on the host and on the GPU ----
def values_of(w, vseed):
    """the matrix values in force: the operand set's own, or the integers an update_values / backward step drew"""
    return w["ops"]["va"] if not w["mutable"] else util.int_values(len(w["ops"]["ci"]), vseed)


def doubled_factors(w):
    """u_row with one entry doubled (the row of the hub: it has entries) and u_col"""
    o = w["ops"]
    u = o["u_row"].copy()
    u[int(np.diff(o["rp"]).argmax())] *= 2
    return u, o["u_col"]


def features(step, rows):
    if step["kind"] == "wide":
        return util.wide_features(rows, step["k"], seed=step["bseed"])
    return util.int_features(rows, step["k"], seed=step["bseed"])


def bias_of(step):
    return np.random.default_rng(step["bseed"] + 1).integers(-8, 9, step["k"]).astype(np.float32)


def epilogue_of(step):
    """-> (bias or None, relu, dropout triple or None) of a product call"""
    e = util.EPILOGUES[step["epi"]] if step["epi"] is not None else {}
    return (bias_of(step) if e.get("bias") else None), bool(e.get("relu")), (util.EPILOGUE_DROPOUT if e.get("dropout") else None)


def apply_epilogue(step, raw, m):
    """util.epilogue_reference of a call's raw sums (fp64), and what a row without entries must hold"""
    bias, relu, drop = epilogue_of(step)
    keep = util.dropout_keep(m * step["k"], *drop).reshape(m, step["k"]) if drop else None
    return util.epilogue_reference(raw, bias, relu, keep, 2.0), util.epilogue_reference(np.zeros_like(raw), bias, relu, keep, 2.0)


def describe(w, upto, names=()):
    """the walk's steps 0 .. upto as a recipe, with the kernel name read at each call"""
    names = dict(names)
    lines = [f"walk(seed={w['seed']}, family={w['family']!r}) on {w['pattern']}, side_stream={w['side_stream']}:"]
    for i, s in enumerate(w["steps"][:upto + 1]):
        if s["op"] == "reconf":
            arg = s.get("vseed") if s["name"] == "update_values" else s["arg"]
            lines.append(f"  {i:2d} {s['name']}({arg!r}) -> {s['expect']}")
        else:
            e = util.EPILOGUES[s["epi"]] if s["epi"] is not None else None
            lines.append(f"  {i:2d} {s['kind']} k={s['k']} {s['dtype']}->{s['out']} epilogue={e} bseed={s['bseed']} state={s['state']}"
                         f"  [{names.get(i, '')}]")
    return "\n".join(lines)
