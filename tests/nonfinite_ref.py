"""The host twin of the SpMM's behaviour on non-finite feature values (tests/test_nonfinite_cpu.py proves it,
tests/test_nonfinite_gpu.py holds every route to it): pure numpy / scipy, integer counting only.

The CLASS of an output element — finite, NaN, +Inf or -Inf — does not depend on the order or the grouping of the sum, as long
as the finite part cannot overflow: a NaN term makes every partial sum that holds it NaN; without one, partial sums that hold
only +Inf terms are +Inf, only -Inf terms -Inf, and wherever the two kinds meet the sum is NaN and stays NaN.  So the class
follows from three counts per element, taken over the sign patterns of the values:
    n_nan = |pattern| @ isnan(B),   n_pos = P @ (B == +Inf) + N @ (B == -Inf),   n_neg = P @ (B == -Inf) + N @ (B == +Inf)
with P = val > 0 and N = val < 0.  NaN where n_nan > 0 or both others are; +Inf / -Inf where only n_pos / n_neg is; finite
elsewhere.  The epilogue in the order of include/gcn_spmm.h: a finite bias changes no class, ReLU maps -Inf to 0 and keeps
+Inf and NaN, a dropped element is exactly 0 (the mask selects, it does not multiply), a kept one keeps its class.

Preconditions (assert_nonfinite_inputs): no stored zero in A (0 * Inf is NaN by IEEE, and the dense panels skip zeros), positive
value factors, max |A|.|B_finite| < 2^100.  One route stores something else than the entries: a dense panel's tile holds the SUM
of the repeated entries of one (row, column), so inside such a window the counts are taken over the merged entries, and a group
that sums to zero is skipped as the kernel's entry-by-entry pass skips it (`merged`, panel_plan_twin)."""
import numpy as np
import scipy.sparse as sp

from util import EPILOGUE_DROPOUT, HUB_MIN, dropout_keep, exact_operands, int_features

FINITE, NAN, PINF, NINF, ZERO = 0, 1, 2, 3, 4
CLASS_NAMES = ("finite", "NaN", "+Inf", "-Inf", "0")
SNAN_BITS = 0x7F800001                                 # a signalling NaN whose payload lies in the 16 bits a bf16 drops
PANEL_R, PANEL_W, PANEL_BIN, PANEL_DENSE = 128, 512, 128, 0.25      # spmm_panel.hip, plan_build.cpp


def _entries(rowptr, col, val, merged=None):
    """(rows, cols, vals) of the entries the kernels multiply: the stored ones, those under `merged` summed per (row, column)
    and dropped where the sum is zero"""
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)).astype(np.int64)
    cols, vals = np.asarray(col, np.int64), np.asarray(val, np.float64)
    if merged is None or not merged.any():
        return rows, cols, vals
    n = int(cols.max()) + 1
    key, inv = np.unique(rows[merged] * n + cols[merged], return_inverse=True)
    sums = np.bincount(inv, weights=vals[merged], minlength=len(key))
    live = sums != 0
    return (np.concatenate([rows[~merged], key[live] // n]), np.concatenate([cols[~merged], key[live] % n]),
            np.concatenate([vals[~merged], sums[live]]))


def class_counts(rowptr, col, val, B, merged=None):
    """(n_nan, n_pos, n_neg, touched) [m x k]: the counts of the module's header; touched[i, j]: row i holds an entry (i, c)
    with B[c, j] non-finite"""
    B = np.asarray(B)
    m, (n, k) = len(rowptr) - 1, B.shape
    rows, cols, vals = _entries(rowptr, col, val, merged)
    bad = ~np.isfinite(B)
    J = np.flatnonzero(bad.any(0))                       # only these feature columns can hold anything
    out = [np.zeros((m, k), np.int64) for _ in range(4)]
    if len(J):
        mk = lambda sel: sp.csr_matrix((sel.astype(np.int64), (rows, cols)), shape=(m, n))
        P, N, A1 = mk(vals > 0), mk(vals < 0), mk(np.ones(len(vals), bool))
        Bj = B[:, J]
        isnan, pinf, ninf = (np.isnan(Bj).astype(np.int64), (Bj == np.inf).astype(np.int64), (Bj == -np.inf).astype(np.int64))
        out[0][:, J] = (P + N) @ isnan
        out[1][:, J] = P @ pinf + N @ ninf
        out[2][:, J] = P @ ninf + N @ pinf
        out[3][:, J] = A1 @ bad[:, J].astype(np.int64)
    return out[0], out[1], out[2], out[3] > 0


def apply_epilogue(cls, bias=None, relu=False, keep=None):
    """the class after dropout(act(. + bias)): see the module's header"""
    cls = cls.copy()
    if bias is not None:
        assert np.all(np.isfinite(bias))
    if relu:
        cls[cls == NINF] = ZERO
    if keep is not None:
        cls[~np.asarray(keep, bool)] = ZERO
    return cls


def spmm_class(rowptr, col, val, B, bias=None, relu=False, keep=None, merged=None):
    """-> (cls int8 [m x k] of FINITE / NAN / PINF / NINF / ZERO, touched bool [m x k]) of dropout(act(A.B + bias))"""
    n_nan, n_pos, n_neg, touched = class_counts(rowptr, col, val, B, merged)
    cls = np.full(n_nan.shape, FINITE, np.int8)
    cls[(n_pos > 0) & (n_neg == 0)] = PINF
    cls[(n_neg > 0) & (n_pos == 0)] = NINF
    cls[(n_nan > 0) | ((n_pos > 0) & (n_neg > 0))] = NAN
    return apply_epilogue(cls, bias, relu, keep), touched


def class_of(C):
    """the class of every element of a result (ZERO: exactly 0, either sign)"""
    C = np.asarray(C, np.float32)
    cls = np.where(C == 0, ZERO, FINITE).astype(np.int8)
    cls[np.isnan(C)], cls[C == np.inf], cls[C == -np.inf] = NAN, PINF, NINF
    return cls


def assert_contained(C_poison, C_clean, cls, touched, what="", bits=None, sentinel=None):
    """The assertions every case of the sweep makes on the results of one plan on B_clean and on B_poison:
    the clean result is finite everywhere (so all of it was written over the NaN sentinel); an untouched element has the same
    BITS in both; a touched one has the twin's class (the sign and the payload of a NaN are not compared; ZERO: exactly 0).
    bits: (poison, clean) as integer arrays where C is not fp32 (a bf16 result); sentinel: no element of the poisoned result
    still holds these bits."""
    Cp, Cc = np.asarray(C_poison, np.float32), np.asarray(C_clean, np.float32)
    assert Cp.shape == Cc.shape == cls.shape == touched.shape, (Cp.shape, Cc.shape, cls.shape, what)
    bp, bc = (Cp.view(np.int32), Cc.view(np.int32)) if bits is None else bits
    assert np.all(np.isfinite(Cc)), f"{what}: the result on finite features is not finite (or was not written)"
    if sentinel is not None:
        assert not np.any(bp == np.asarray(sentinel).astype(bp.dtype)), f"{what}: an element of the poisoned result was not written"
    leak = ~touched & (bp != bc)
    if leak.any():
        i = tuple(int(x) for x in np.argwhere(leak)[0])
        raise AssertionError(f"{what}: {int(leak.sum())} untouched elements changed, first at {i}: {float(Cc[i])!r} -> {float(Cp[i])!r}")
    assert not np.any(touched & (cls == FINITE)), f"{what}: the twin calls a touched element finite"
    wrong = touched & (class_of(Cp) != cls)
    if wrong.any():
        i = tuple(int(x) for x in np.argwhere(wrong)[0])
        raise AssertionError(f"{what}: {int(wrong.sum())} of {int(touched.sum())} touched elements have the wrong class, first at {i}: "
                             f"got {float(Cp[i])!r}, want {CLASS_NAMES[cls[i]]}")


# ---------------------------------------------------------------------------------------------------------------
# where the non-finite values go
def panel_plan_twin(rowptr, col, m, n):
    """(w0 [panels], dense [panels]) as the plan chooses them (panel_windows_kernel, gcn_spmm_plan_enable_panels): per panel of
    128 rows the FIRST best run of four 128-column bins of its column histogram, clamped to n - 512; dense when the window
    holds at least a quarter of 128 x 512 entries (repeated ones counted)"""
    panels = (m + PANEL_R - 1) // PANEL_R
    nbins = (n + PANEL_BIN - 1) // PANEL_BIN
    w0, dense = np.zeros(panels, np.int64), np.zeros(panels, bool)
    span = PANEL_W // PANEL_BIN
    for p in range(panels):
        c = np.asarray(col[rowptr[p * PANEL_R]:rowptr[min(m, (p + 1) * PANEL_R)]], np.int64)
        cum = np.concatenate([[0], np.cumsum(np.bincount(c // PANEL_BIN, minlength=nbins))])
        b = np.arange(nbins)
        run = cum[b + 1] - cum[np.maximum(b + 1 - span, 0)]
        best = int(np.argmax(run)) if len(c) else 0      # (argmax: the first maximum, as the kernel's `run > best`)
        w = max(0, best - span + 1) * PANEL_BIN if run[best] > 0 else 0
        w0[p] = max(0, n - PANEL_W) if w > n - PANEL_W else w
        dense[p] = ((c >= w0[p]) & (c < w0[p] + PANEL_W)).sum() >= PANEL_DENSE * PANEL_R * PANEL_W
    return w0, dense


def in_dense_tile(rowptr, col, m, n):
    """bool [nnz]: the entry lies inside the window of a dense panel (its value is merged into the tile)"""
    w0, dense = panel_plan_twin(rowptr, col, m, n)
    p = np.repeat(np.arange(m), np.diff(rowptr)) // PANEL_R
    c = np.asarray(col, np.int64)
    return dense[p] & (c >= w0[p]) & (c < w0[p] + PANEL_W), w0, dense


def poison(B, rowptr, col, slices, seed, val=None, windows=None):
    """-> (B with about a dozen single ELEMENTS replaced by NaN / +Inf / -Inf, [(B row, feature column, value, role)]).
    B rows: 0 and n - 1 (what padding lanes tend to gather), the first and last row of every column slice, a column of the hub
    row, a column of a single-entry row (one that no other row stores, where there is one), three columns of ordinary rows, two
    columns that one ordinary row stores with values of one sign (+Inf and -Inf in one feature column: they meet in that row), and with windows = (w0,
    dense) a column in the middle of a dense (else any) panel's window and the column of an entry outside its panel's window.
    Feature columns: 0, k - 1 (for odd k the last before a row's padded tail) and, for k > 64, 63 and 64."""
    B = np.array(B, np.float32, copy=True)
    (n, k), m = B.shape, len(rowptr) - 1
    rng = np.random.default_rng(seed)
    lens = np.diff(rowptr)
    rows_of = np.repeat(np.arange(m), lens)
    refs = np.bincount(col, minlength=n)
    hub = int(np.argmax(lens))
    fcols = list(dict.fromkeys([0, k - 1] + ([63, 64] if k > 64 else [])))
    values = [np.nan, np.inf, -np.inf, "snan"]
    placed, taken = [], set()

    def put(brow, role, j=None, v=None):
        brow = int(brow)
        if j is None:
            free = [f for f in fcols if (brow, f) not in taken]
            if not free:
                return
            j = free[len(placed) % len(free)]
        if (brow, j) in taken:
            return
        v = values[len(placed) % len(values)] if v is None else v
        taken.add((brow, j))
        if isinstance(v, str):
            B.view(np.int32)[brow, j] = SNAN_BITS
            v = np.nan
        else:
            B[brow, j] = v
        placed.append((brow, int(j), float(v), role))

    # +Inf and -Inf meeting in one ordinary row
    sgn = np.ones(len(col)) if val is None else np.sign(val)
    for r in rng.permutation(np.flatnonzero((lens >= 2) & (lens < HUB_MIN))):
        e = np.arange(rowptr[r], rowptr[r + 1])
        pos = e[sgn[e] > 0]
        cs = np.unique(col[pos])
        if len(cs) >= 2 and np.all(sgn[e][np.isin(col[e], cs[:2])] > 0):
            j = fcols[int(rng.integers(len(fcols)))]
            put(cs[0], "pair+", j, np.inf)
            put(cs[1], "pair-", j, -np.inf)
            break
    put(0, "row0")
    put(n - 1, "last_row")
    S = max(int(slices), 1)
    w = (n + S - 1) // S
    if S > 1:
        for s in range(S):
            put(s * w, f"slice{s}_first")
            put(min((s + 1) * w, n) - 1, f"slice{s}_last")
    hub_cols = np.unique(col[rowptr[hub]:rowptr[hub + 1]])
    for c in rng.permutation(hub_cols)[:3]:               # three, so that the hub row meets every kind of value
        put(c, "hub")
    for r in rng.permutation(np.flatnonzero((lens >= 2) & (lens < HUB_MIN)))[:3]:
        put(col[rowptr[r] + int(rng.integers(lens[r]))], "ordinary")
    single = np.flatnonzero(lens == 1)
    if len(single):
        sc = col[rowptr[single]]
        only = sc[refs[sc] == 1]
        put(only[0] if len(only) else sc[len(sc) // 2], "single_only" if len(only) else "single")
    if windows is not None:
        w0, dense = windows
        p_of = rows_of // PANEL_R
        cands = np.flatnonzero(dense) if dense.any() else np.arange(len(w0))
        p = int(cands[len(cands) // 2])
        inside = np.unique(col[(p_of == p) & (col >= w0[p] + 128) & (col < w0[p] + 384)])
        if len(inside):
            put(inside[len(inside) // 2], "window_in")
        far = np.flatnonzero(np.isin(p_of, cands) & ((col < w0[p_of] - 128) | (col >= w0[p_of] + PANEL_W + 128)))
        if len(far):
            put(col[far[len(far) // 2]], "window_out")
    return B, placed


def assert_nonfinite_inputs(rowptr, col, val, B_clean, B_poison, u_row=None, u_col=None, merged=None, need=()):
    """The preconditions of the class contract on a test's own inputs (the module's header), and that the inputs can tell:
    every origin of a class occurs among the touched elements (NaN from a NaN, NaN from +Inf meeting -Inf, +Inf alone, -Inf
    alone); the hub row (a row of HUB_MIN entries, where the pattern has one), a single-entry row (where it has one) and an
    ordinary row each hold a touched element; at least 90 % of the elements are untouched.  need: poison()'s list of what it placed.
    -> dict(touched, origins, rows, roles: those of `need`) for the caller's own checks and the test's log"""
    val = np.asarray(val)
    lens = np.diff(rowptr)
    assert np.all(val != 0) and np.all(np.isfinite(val)), "a stored zero (or a non-finite value) in A"
    for u in (u_row, u_col):
        assert u is None or (np.all(u > 0) and np.all(np.isfinite(u))), "value factors must be positive"
    assert np.all(np.isfinite(B_clean))
    same = np.isfinite(B_poison)
    assert np.array_equal(B_poison[same], B_clean[same])
    # max |A|.|B_finite| <= (longest row) * max |A| * max |B_finite|
    assert float(lens.max()) * float(np.abs(val).max()) * float(np.abs(B_clean).max()) < 2.0 ** 100
    n_nan, n_pos, n_neg, touched = class_counts(rowptr, col, val, B_poison, merged)
    origins = dict(nan_from_nan=n_nan > 0, nan_from_both_inf=(n_nan == 0) & (n_pos > 0) & (n_neg > 0),
                   pos_inf=(n_nan == 0) & (n_pos > 0) & (n_neg == 0), neg_inf=(n_nan == 0) & (n_neg > 0) & (n_pos == 0))
    for name, where in origins.items():
        assert (where & touched).any(), f"no touched element is a {name}"
    hub = int(np.argmax(lens))
    rows = dict(ordinary=touched[(lens >= 2) & (lens < HUB_MIN)].any())
    if lens[hub] >= HUB_MIN:
        rows["hub"] = touched[hub].any()
    if (lens == 1).any():
        rows["single_entry"] = touched[lens == 1].any()
    assert all(rows.values()), rows
    assert touched.mean() <= 0.10, touched.mean()
    roles = {r.rstrip("+-") for _b, _j, _v, r in need}
    return dict(touched=int(touched.sum()), origins={k: int((v & touched).sum()) for k, v in origins.items()}, rows=rows, roles=roles)


# ---------------------------------------------------------------------------------------------------------------
# the operands of every case of tests/test_nonfinite_gpu.py, built (and their preconditions asserted) once per process
# (pattern, kind, widths, slices handed to poison(): the plan's slice count, 0 unsliced)
NONFINITE_CASES = [("unsliced", "int", (4, 8, 15, 16, 36, 41, 64, 100, 128, 256), 0),
                   ("group_dup", "int", (16, 32, 40, 41, 64, 72, 100, 128, 260), 3),
                   ("group_dup", "pow2", (16, 21, 32, 40, 41, 64, 72, 100, 128, 260), 3),
                   ("group_diag_dup", "pow2", (16, 41, 128), 3),
                   ("group_dup", "int", (16, 64, 128), 9), ("group_dup", "pow2", (16, 64, 128), 9),
                   ("group", "pow2", (64,), 3),
                   ("vcsr", "int", (64,), 4), ("col16", "pow2", (64,), 2), ("lds", "int", (64, 100), 0),
                   ("lds_all", "int", (64, 100), 0), ("mfma", "int", (36, 64, 128), 0)]
TRANSPOSED_CASES = [("unsliced", "int", 64, 0), ("group_dup", "int", 64, 3)]
PANEL_PATTERNS = ("lds", "lds_all", "mfma")
_INPUTS = {}


def transposed(ops):
    """the operands of A^T, repeated entries kept apart (as gcn_amd's transpose keeps them), rows column-sorted"""
    At = sp.csr_matrix((ops["va"], ops["ci"], ops["rp"]), shape=(ops["m"], ops["n"])).tocsc()
    return dict(rp=At.indptr.astype(np.int32), ci=At.indices.astype(np.int32), va=At.data.astype(np.float32), m=ops["n"], n=ops["m"],
                u_row=ops["u_col"], u_col=ops["u_row"])


def nonfinite_inputs(pattern, kind, k, slices=0, transpose=False):
    """-> dict(ops, B, Bp, placed, cls, touched, bias, keep, merged, report) for one (matrix, width, slice count): B the finite
    features of util.epilogue_inputs (integers in [-8, 8]: a bf16 holds them), Bp the poisoned copy, cls / touched the twin's
    answer without an epilogue (apply_epilogue gives the others), bias / keep those of util.epilogue_inputs"""
    key = (pattern, kind, k, slices, transpose)
    if key not in _INPUTS:
        ops = exact_operands(pattern, kind)
        if transpose:
            ops = transposed(ops)
        m, n = ops["m"], ops["n"]
        B = int_features(n, k, seed=3000 + k)
        bias = np.random.default_rng(k).integers(-8, 9, k).astype(np.float32)
        merged = windows = None
        if pattern in PANEL_PATTERNS:
            merged, w0, dense = in_dense_tile(ops["rp"], ops["ci"], m, n)
            windows = (w0, dense)
        Bp, placed = poison(B, ops["rp"], ops["ci"], slices, seed=7000 + k, val=ops["va"], windows=windows)
        report = assert_nonfinite_inputs(ops["rp"], ops["ci"], ops["va"], B, Bp, ops["u_row"], ops["u_col"], merged, need=placed)
        want = {"row0", "last_row", "hub", "pair"} | ({"window_in", "window_out"} if pattern in ("lds", "mfma") else set())
        want |= {"window_in"} if pattern == "lds_all" else set()
        want -= {"hub"} if pattern == "lds_all" else set()
        want |= {f"slice{s}_{e}" for s in range(slices if slices > 1 else 0) for e in ("first", "last")}
        assert want <= report["roles"] | {"slice0_first", f"slice{slices - 1}_last"}, (key, sorted(want - report["roles"]))
        cls, touched = spmm_class(ops["rp"], ops["ci"], ops["va"], Bp, merged=merged)
        _INPUTS[key] = dict(ops=ops, B=B, Bp=Bp, placed=placed, cls=cls, touched=touched, bias=bias, merged=merged, report=report,
                            dense=None if windows is None else int(windows[1].sum()))
    return _INPUTS[key]


DROPIN_SEED, DROPIN_K = 20, 64                        # tests/stress_dropin.py: n = 20001, two slices, weighted, the group format
HEADS, HEAD_F = 4, 8


def dropin_inputs():
    """the drop-in pair's case: the smallest weighted group-format matrix of tests/stress_dropin.py (rows of 511 .. 1025 entries
    inside one slice and a 5000-entry hub row: head pieces for group_fixup_kernel), poisoned as every other case"""
    key = ("dropin", DROPIN_SEED, DROPIN_K)
    if key not in _INPUTS:
        import stress_dropin as sd
        c = sd.case(DROPIN_SEED)
        assert c["format"] == "group" and not c["factoring"] and c["layout"]["S"] == 2
        ops = dict(rp=c["rp"], ci=c["ci"], va=c["va"], m=c["m"], n=c["n"])
        B = int_features(c["n"], DROPIN_K, seed=3000 + DROPIN_K)
        Bp, placed = poison(B, ops["rp"], ops["ci"], c["layout"]["S"], seed=7000 + DROPIN_K, val=ops["va"])
        report = assert_nonfinite_inputs(ops["rp"], ops["ci"], ops["va"], B, Bp, need=placed)
        assert {"hub", "pair", "slice1_first", "slice0_last"} <= report["roles"]
        cls, touched = spmm_class(ops["rp"], ops["ci"], ops["va"], Bp)
        _INPUTS[key] = dict(ops=ops, B=B, Bp=Bp, placed=placed, cls=cls, touched=touched, report=report)
    return _INPUTS[key]


def heads_inputs():
    """spmm_heads on the unsliced pattern: H = 4 heads of F = 8 columns, per-head integer values, ONE poisoned element
    (a column of the hub row, head 2, its column 3) -> dict(ops, values [nnz x H], X, Xp, cls, touched, at)"""
    key = ("heads",)
    if key not in _INPUTS:
        from util import int_values
        ops = exact_operands("unsliced", "int")
        nnz, k = len(ops["ci"]), HEADS * HEAD_F
        values = np.stack([int_values(nnz, seed=900 + h) for h in range(HEADS)], axis=1)
        X = int_features(ops["n"], k, seed=3000 + k)
        hub = int(np.argmax(np.diff(ops["rp"])))
        c, j = int(ops["ci"][ops["rp"][hub] + 7]), 2 * HEAD_F + 3
        Xp = X.copy()
        Xp[c, j] = -np.inf
        cls, touched = np.zeros((ops["m"], k), np.int8), np.zeros((ops["m"], k), bool)
        for h in range(HEADS):
            s = slice(h * HEAD_F, (h + 1) * HEAD_F)
            cls[:, s], touched[:, s] = spmm_class(ops["rp"], ops["ci"], values[:, h], Xp[:, s])
        assert touched[hub, j] and touched[:, j].sum() >= 2 and touched.sum() == touched[:, j].sum()
        assert {int(x) for x in np.unique(cls[touched])} >= {PINF, NINF}       # values of both signs meet the -Inf
        _INPUTS[key] = dict(ops=ops, values=values, X=X, Xp=Xp, cls=cls, touched=touched, at=(c, j))
    return _INPUTS[key]


_KEEP = {}


def keep_mask(m, k):
    """the dropout mask of util.epilogue_inputs"""
    if (m, k) not in _KEEP:
        p, seed, offset = EPILOGUE_DROPOUT
        _KEEP[(m, k)] = dropout_keep(m * k, p, seed, offset).reshape(m, k)
    return _KEEP[(m, k)]
