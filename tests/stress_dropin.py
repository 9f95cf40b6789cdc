"""The generator of the seeded sweep over the drop-in pair csr2tile -> flexspmm, with cuspmm and permutate beside it
(tests/test_stress_dropin_cpu.py checks it and the host packer without a GPU, tests/test_stress_dropin_gpu.py runs it):
``case(seed)`` returns, deterministically from the seed, one m x n matrix as numpy arrays and the steps that run on it;
``twin(case)`` evaluates the fp64 oracle on every step.

Seed classes (SEEDS = 24):
  (a) 0 .. 15   plain format, m <= 1500, nnz <= 60 000.  Row-length styles by seed % 4 as in stress_units (bounds: the
                chunk size T = 64, and 65 and 129 entries: the chunks either side, a row over three or more chunks, one row
                of exactly a bound's length after a run of empty rows, empty first and last rows unless a long row is forced
                there).  Half square, half rectangular (RECT_WIDE: m < n, RECT_TALL: m > n); style 0 symmetric; even seeds
                column-sorted, odd ones shuffled inside the rows; about a quarter of the entries repeat a column; the mean
                row length lies on either side of the quad kernel's 48 (DENSE).  Seeds 3, 7 and 11 sit at csr2tile's refusal
                boundary with nnz = m + 17, m + 18, m + 19, nnz % 9 == 8 and an odd nnz / 9 (the parity step costs a
                segment): 9 * n_segs is m, m + 1, m + 2, so the first is refused and the others pack (the library's message
                asks for m + 19; the rule itself, 9 * n_segs >= m + 1, is what is asserted).
  (b) 16, 17    plain format either side of the chunk-size step: T = dropin_T(n_segs) doubles where 9 * n_segs reaches
                2^20; m = n about 20 000 at mean degree 52 (below the group rule), one hub row longer than 2 * T.
  (c) 18 .. 23  the group format's smallest shapes: n = 16385 with 9 * n_segs // n == 128 (S = 2), n = 32769 (S = 4),
                n = 20001 (S = 2, weighted), n = 17001 (S = 2, weighted, symmetric), and two plain-format neighbours that
                must NOT take the group format: n = 16384 at mean degree 140 (the table fits an L2) and n = 16390 with
                9 * n_segs // n == 127.  Each group case has virtual rows of 511, 512, 513, 1024 and 1025 entries inside one
                slice (rows that are empty in the other), a 5000-entry hub row, duplicates, and — weighted cases — empty
                first and last rows, single-entry diagonal rows in their place where the values factor.  The last row of a
                slice cannot be both empty and the hub: the hub is row m - 1 on seeds 18 and 23 and row m - 2 on 19 and 20.
Every matrix has one filler row that steers nnz: over the seeds every residue nnz % 9 meets both parities of n_segs and
both outcomes of "n_segs is nnz / 9" / "one less" (TARGETS).

Values and features make every sum exact in fp32 in any order: integers in [-4, 4] (WEIGHTED), or u[r] * u[c] with
u = 2^-e, e <= 3, and a stored positive diagonal in every row (FACTORING: csr2tile finds u itself and n_segs is odd);
features and gradients are integers in [-8, 8].  A row holds fewer than 2^15 entries, so |sum| * 2^6 < 2^24.
``ulp_case`` is the one exception (csr2tile's 4-ulp rule); ``pack`` runs csr2tile inside guarded buffers."""
import numpy as np

import stress_units as su
from util import factored_values, int_features, int_values, oracle_spmm, pow2_factors

SEEDS = 24
K_LIST = (1, 2, 3, 4, 5, 8, 9, 12, 16, 17, 33, 36, 48, 64, 65, 100, 128, 200, 256)
WIDTH_CLASSES = {"<=8": lambda k: k <= 8, "12..32": lambda k: 12 <= k <= 32, "odd<=16": lambda k: k % 2 == 1 and k <= 16,
                 "odd>16": lambda k: k % 4 != 0 and k > 16, "33..48": lambda k: 33 <= k <= 48, "64": lambda k: k == 64,
                 "partial": lambda k: k > 64 and k % 64 != 0, "256": lambda k: k == 256}
T_SMALL = 64
BOUNDS = (T_SMALL, T_SMALL + 1, 2 * T_SMALL + 1)
QUAD_MIN_ROW = 48                                      # spmm_kernels.hip: kQuadMinRowLen
GROUP_T = 512
GROUP_SPECIALS = (511, 512, 513, 1024, 1025)
GROUP_HUB = 5000
NNZ_MAX = 60000

RECT_WIDE, RECT_TALL = (2, 7, 9, 14), (3, 6, 11, 13)   # m < n, m > n
DENSE = (2, 5, 6, 9, 10, 13, 14, 15)                    # mean row length >= 48 (class (a))
BOUNDARY = {3: 17, 7: 18, 11: 19}                       # nnz - m
FACTORING = (1, 4, 5, 8, 10, 15, 17, 18, 19, 21)
WEIGHTED = tuple(s for s in range(SEEDS) if s not in FACTORING)
# seed -> (n, S or 0: a plain-format neighbour, 9 * n_segs // n wanted, hub row counted from the end)
GROUP_SHAPES = {18: (16385, 2, 128, 1), 19: (32769, 4, 128, 2), 20: (20001, 2, 130, 2), 21: (16384, 0, 140, 2),
                22: (16390, 0, 127, 2), 23: (17001, 2, 129, 1)}
GROUP_WIDTHS = {18: (3, 256, 17), 19: (4, 64, 12), 20: (9, 200, 36), 23: (5, 100, 33)}
STEP_SEEDS = (16, 17)                                   # class (b)


def _targets():
    """seed -> (nnz % 9, parity of nnz // 9).  The first nine factoring seeds get an odd nnz // 9 (n_segs is nnz / 9, odd), the
    first eight weighted ones that are free an odd one too (n_segs is one less, even; residue 8 is the boundary seeds'); the
    rest the other outcome"""
    t = {}
    for i, s in enumerate(FACTORING):
        t[s] = (i % 9, 1 if i < 9 else 0)
    free = [s for s in WEIGHTED if s not in BOUNDARY]
    for i, s in enumerate(free):
        t[s] = (i, 1) if i < 8 else (i - 7, 0)
    for s in BOUNDARY:
        t[s] = (8, 1)
    return t


TARGETS = _targets()


def symmetric(seed):
    return (seed < 16 and seed % 4 == 0) or seed == 23


def steer(nnz, res, q):
    """the smallest count >= nnz with count % 9 == res and (count // 9) % 2 == q"""
    for x in range(nnz, nnz + 18):
        if x % 9 == res and (x // 9) & 1 == q:
            return x
    raise AssertionError((nnz, res, q))


# ---- the host twins of what both csr2tile and flexspmm compute from (m, n, n_segs) (api_dropin.cpp) ------------------------------
def dropin_T(n_segs):
    """auto_chunk_nnz(9 * n_segs, 256): the largest power of two <= 9 * n_segs / 8192 within [64, 2048]"""
    per_wave, t = 9 * n_segs // (256 * 32), 64
    while t * 2 <= per_wave and t < 2048:
        t *= 2
    return t


def group_layout(m, n, n_segs):
    """dropin_group: None (plain format) or dict(S, w, total_ub, nchunks_ub, fix_off, val_off)"""
    from gcn_amd import _lib
    if m != n or n_segs <= 0:
        return None
    S = int(_lib.load().gcn_spmm_auto_slices(m, n, 9 * n_segs, 1))
    if S <= 1:
        return None
    w, T = (n + S - 1) // S, GROUP_T
    total_ub = (9 * n_segs + 17 + S * m + (S + 64) * T + 63) // (64 * T) * (64 * T) + 64 * T
    nchunks_ub = total_ub // T
    if w > 32767 or total_ub >= 2 ** 31 or (total_ub * 2 + 15) // 16 * 16 + total_ub * 4 > 72 * n_segs:
        return None
    if 16 + 2 * nchunks_ub + 4 + 4 * nchunks_ub > 9 * n_segs or n > 8 * n_segs:
        return None
    return dict(S=S, w=w, total_ub=total_ub, nchunks_ub=nchunks_ub, fix_off=(16 + 2 * nchunks_ub + 3) // 4 * 4,
                val_off=(total_ub * 2 + 15) // 16 * 4)


def expected_n_segs(m, nnz, factoring):
    """what csr2tile returns: nnz / 9, one less when its lowest bit would not say `factoring`; 0 when the row pointer or
    the chunk rows do not fit the caller's buffers"""
    ns = nnz // 9
    if (ns & 1) != (1 if factoring else 0):
        ns -= 1
    if ns <= 0 or m + 1 > 9 * ns or (nnz + dropin_T(ns) - 1) // dropin_T(ns) > 8 * ns:
        return 0
    return ns


# ---- the matrices ----------------------------------------------------------------------------------------------------------------
def _assemble(rng, m, n, lens, fixed, sym, factoring, filler, target, shuffled, dup=0.25, seed=0):
    """(rowptr, col, val, u) of an m x n matrix.  lens [m]: the entry counts of the rows whose columns are drawn freely;
    fixed: row -> (count, column range) of the rows with an exact count (a stored diagonal counts); sym: the drawn pattern
    joins its transpose (then no column is drawn in a fixed row's, the first, the last or the filler's index: their counts
    stay what they are); factoring: a diagonal entry in every row, values u[r] * u[c]; filler: the row that takes what is
    missing to `target(count so far)` entries"""
    lens = lens.copy()
    apart = set(fixed) | {filler}
    lens[list(apart)] = 0
    if factoring:
        lens = np.maximum(lens - 1, 0)                   # (the diagonal is one of the row's entries)
    if sym:
        lens = (lens + 1) // 2
        apart |= {0, m - 1}
    allowed = np.setdiff1d(np.arange(n), np.fromiter(apart, np.int64)) if sym else np.arange(n)
    rows = np.repeat(np.arange(m), lens)
    cols = allowed[rng.integers(0, len(allowed), len(rows))]
    again = np.flatnonzero((rng.random(len(rows)) < dup)[1:] & (rows[1:] == rows[:-1])) + 1
    cols[again] = cols[again - 1]                        # repeated columns (next to each other once the row is sorted)
    vals = int_values(len(rows), seed + 500)
    parts = [(rows, cols, vals)]
    if sym:
        off = rows != cols
        parts.append((cols[off], rows[off], vals[off]))
    for j, (r, (count, (lo, hi))) in enumerate(sorted(fixed.items())):
        count -= 1 if factoring and count > 0 else 0
        pool = allowed[(allowed >= lo) & (allowed < hi) & (allowed != r)]
        c = pool[rng.integers(0, len(pool), count)]
        v = int_values(count, seed + 600 + j)
        parts.append((np.full(count, r), c, v))
        if sym:
            parts.append((c, np.full(count, r), v))
    if factoring:
        parts.append((np.arange(m), np.arange(m), np.ones(m, np.float32)))
    have = sum(len(p[0]) for p in parts)
    want = target(have)
    assert want >= have, (want, have)
    extra = want - have
    pool = allowed[allowed != filler]
    if sym:                                              # pairs, and one more diagonal entry when the count is odd
        c = pool[rng.integers(0, len(pool), extra // 2)]
        v = int_values(len(c), seed + 700)
        parts += [(np.full(len(c), filler), c, v), (c, np.full(len(c), filler), v)]
        if extra & 1:
            parts.append((np.array([filler]), np.array([filler]), np.array([2.0], np.float32)))
    else:
        c = pool[rng.integers(0, len(pool), extra)]
        parts.append((np.full(extra, filler), c, int_values(extra, seed + 700)))
    rows, cols, vals = (np.concatenate([p[i] for p in parts]) for i in range(3))
    assert len(rows) == want
    order = np.lexsort((cols, rows))
    if shuffled:                                         # the rows' entries in a drawn order
        perm = rng.permutation(len(rows))
        order = perm[np.argsort(rows[perm], kind="stable")]
    rows, cols, vals = rows[order], cols[order].astype(np.int32), vals[order].astype(np.float32)
    rp = np.zeros(m + 1, np.int64)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=m))
    rp = rp.astype(np.int32)
    u = None
    if factoring:
        u = pow2_factors(n, seed + 800)
        vals = factored_values(rp, cols, u, u)
    return rp, cols, vals, u


def _small(seed):
    rng = np.random.default_rng([seed, 101])
    style, dense = su.style_of(seed), seed in DENSE
    res, q = TARGETS[seed]
    if seed in BOUNDARY:                                 # nnz = m + 17 / 18 / 19 = 18 j + 17: residue 8, an odd nnz / 9
        m = 18 * int(rng.integers(20, 60)) + 17 - BOUNDARY[seed]
        inner = rng.multinomial(m + BOUNDARY[seed], np.full(m - 2, 1.0 / (m - 2)))
        lens, filler = np.concatenate([[0], inner, [0]]).astype(np.int64), m // 2
        total = m + BOUNDARY[seed]
        target = lambda have: total                      # (the filler takes back its own draw: the total is exact)
    else:
        m = int(rng.integers(200, (440 if dense or style == 3 else 1500) + 1))
        lens, placed = su.row_lengths(rng, seed, m, BOUNDS, cap=26000 if dense else 48000)
        if not su.forced(seed):
            lens[[0, m - 1]] = 0
        cand = np.flatnonzero((lens >= 1) & (lens < 60))  # (an ordinary row: the bound-length rows hold 63 entries or more)
        cand = cand[(cand > 0) & (cand < m - 1)]
        filler = int(cand[len(cand) // 2])
        if dense:                                        # every ordinary row longer; the bound-length rows stay
            ordinary = (lens > 0) & (lens < 60)
            lens[ordinary] += rng.integers(45, 70, m)[ordinary]
        floor = m + 40 + (QUAD_MIN_ROW * m if dense else 0)
        target = lambda have: steer(max(have, floor), res, q)
    n = m
    if seed in RECT_WIDE:
        n = m + int(rng.integers(1, 2500))
    elif seed in RECT_TALL:
        n = int(rng.integers(max(8, m // 8), m))
    rp, ci, va, u = _assemble(rng, m, n, lens, {}, symmetric(seed), seed in FACTORING, filler, target, bool(seed & 1), seed=seed)
    return dict(m=m, n=n, rp=rp, ci=ci, va=va, u=u, filler=filler, bounds=BOUNDS if style == 1 and seed not in BOUNDARY else ())


def _step(seed):
    """m = n = 20 165 at mean degree 52: nnz just below / just above 2^20, where the chunk size doubles"""
    rng = np.random.default_rng([seed, 102])
    n = 20165
    res, q = TARGETS[seed]
    floor = 2 ** 20 - 40 if seed == STEP_SEEDS[0] else 2 ** 20 + 20
    lens = rng.integers(30, 72, n)
    lens[rng.random(n) < 0.02] = 0
    lens[[0, n - 1]] = 0
    hub = int(rng.integers(100, n - 100))
    filler = hub + 7
    lens = np.rint(lens * ((floor - 4000) / lens.sum())).astype(np.int64)
    fixed = {hub: (2 * 128 + 300, (0, n)), hub + 1: (T_SMALL, (0, n)), hub + 2: (T_SMALL + 1, (0, n)), hub + 3: (2 * T_SMALL, (0, n)),
             hub + 4: (2 * T_SMALL + 1, (0, n))}
    rp, ci, va, u = _assemble(rng, n, n, lens, fixed, False, seed in FACTORING, filler, lambda have: steer(max(have, floor), res, q),
                              bool(seed & 1), dup=0.1, seed=seed)
    return dict(m=n, n=n, rp=rp, ci=ci, va=va, u=u, filler=filler, hub=hub, bounds=(T_SMALL, 2 * T_SMALL))


def _group(seed):
    rng = np.random.default_rng([seed, 103])
    n, S, ratio, hub_back = GROUP_SHAPES[seed]
    res, q = TARGETS[seed]
    # 9 * n_segs lies in [nnz - 17, nnz]: `ratio` is 9 * n_segs // n when nnz - 17 >= ratio * n and nnz < (ratio + 1) * n
    floor = ratio * n + 30 if ratio != 127 else 128 * n - 40
    slices = max(S, 2)
    w = (n + slices - 1) // slices
    lens = rng.poisson(ratio - 6, n).astype(np.int64)
    lens[rng.random(n) < 0.01] = 0
    hub, filler = n - hub_back, w - 5
    ends = 1 if seed in FACTORING else 0                 # (the diagonal alone, or nothing)
    fixed = {0: (ends, (0, n)), n - 1: (ends, (0, n))}
    fixed[hub] = (GROUP_HUB, (0, n))
    at = rng.permutation(np.arange(10, w - 10))[:len(GROUP_SPECIALS)]
    for j, (r, L) in enumerate(zip(at, GROUP_SPECIALS)):  # all their columns inside one slice: the row's own (the diagonal)
        sl = j % slices
        fixed[int(r) + sl * w] = (L, (sl * w, min(n, (sl + 1) * w)))
    lens = np.rint(lens * ((floor - 3000 - sum(L for L, _ in fixed.values())) / lens.sum())).astype(np.int64)
    rp, ci, va, u = _assemble(rng, n, n, lens, fixed, symmetric(seed), seed in FACTORING, filler,
                              lambda have: steer(max(have, floor), res, q), bool(seed & 1), dup=0.1, seed=seed)
    return dict(m=n, n=n, rp=rp, ci=ci, va=va, u=u, filler=filler, hub=hub, specials={r: v for r, v in fixed.items() if v[0] in GROUP_SPECIALS},
                bounds=(GROUP_T, 2 * GROUP_T) if S else ())


def _widths(seed):
    if seed in GROUP_WIDTHS:
        return GROUP_WIDTHS[seed]
    ks = sorted(K_LIST[(3 * seed + j) % len(K_LIST)] for j in range(3))
    return ks[0], ks[2], ks[1]                         # narrow -> wide -> narrow


def _make(seed):
    c = _small(seed) if seed < 16 else _step(seed) if seed in STEP_SEEDS else _group(seed)
    m, n, nnz = c["m"], c["n"], len(c["ci"])
    rng = np.random.default_rng([seed, 104])
    c.update(seed=seed, nnz=nnz, factoring=seed in FACTORING, symmetric=symmetric(seed), shuffled=bool(seed & 1),
             cls="a" if seed < 16 else "b" if seed in STEP_SEEDS else "c", lens=np.diff(c["rp"]).astype(np.int64))
    c["n_segs"] = expected_n_segs(m, nnz, c["factoring"])
    c["layout"] = group_layout(m, n, c["n_segs"])
    c["format"] = "refused" if c["n_segs"] == 0 else "group" if c["layout"] else "plain"
    c["T"] = 0 if c["n_segs"] == 0 else GROUP_T if c["layout"] else dropin_T(c["n_segs"])
    steps = [dict(op="flexspmm", k=int(k), off_b=(seed + i) & 3, off_c=(seed + 2 * i + (seed >> 2) + 1) & 3, feat=1000 * seed + i)
             for i, k in enumerate(_widths(seed))]
    steps.append(dict(op="cuspmm", k=int(K_LIST[(5 * seed + 2) % (len(K_LIST) - 3)]), off_b=(seed + 3) & 3, off_c=(seed >> 1) & 3,
                      feat=1000 * seed + 3))
    steps.append(dict(op="permutate", k=int(K_LIST[(7 * seed + 1) % len(K_LIST)]), off_b=(seed + 2) & 3, off_c=0, feat=1000 * seed + 4,
                      perm=rng.permutation(n).astype(np.int32)))
    if c["symmetric"]:
        steps.append(dict(op="grad", k=int(K_LIST[(seed + 4) % 16]), off_b=0, off_c=0, feat=1000 * seed + 5))
    c["steps"] = steps
    return c


_CASES = {}


def case(seed):
    """everything the steps of `seed` need, as numpy arrays; the same at every call (kept: the arrays are read, never written)"""
    if seed not in _CASES:
        _CASES[seed] = _make(int(seed))
    return _CASES[seed]


def forget(seed):
    """drop a kept case (the large ones hold tens of megabytes)"""
    _CASES.pop(seed, None)


def describe(c, i):
    """(seed, class, step, drawn parameters) for an assertion message"""
    small = {k: v for k, v in c["steps"][i].items() if not isinstance(v, np.ndarray)}
    return (f"seed {c['seed']} class {c['cls']} {c['format']} step {i} shape {c['m']}x{c['n']} nnz {c['nnz']} n_segs {c['n_segs']} "
            f"T {c['T']} {'factoring' if c['factoring'] else 'weighted'} {'shuffled' if c['shuffled'] else 'sorted'} {small}")


def features(c, i):
    """the dense operand of step i: B [n x k] (flexspmm, cuspmm, permutate) or the gradient g [m x k] (grad)"""
    s = c["steps"][i]
    return int_features(c["m"] if s["op"] == "grad" else c["n"], s["k"], seed=s["feat"])


def ulp_case(ulps):
    """(e) the factoring graph of seed 18 with one more entry, (0, n // 3) beside row 0's diagonal, of value 1 (u = 1 on both)
    moved up by `ulps` ulps: inside the 4-ulp rule of csr2tile (4.8e-7 relative; an ulp above 1 is 1.19e-7) the matrix still
    factors and the kernels use u[r] * u[c] in its place; outside it the values travel, and b * (1 + ulps * 2^-23) + b' is
    exact in fp32 for |b|, |b'| <= 8"""
    c = dict(case(18))
    n = c["n"]
    r, cc = 0, n // 3
    assert c["rp"][1] == 1 and c["ci"][0] == 0           # row 0: its diagonal ...
    rows = np.concatenate([np.repeat(np.arange(n), np.diff(c["rp"])), [r]])
    cols = np.concatenate([c["ci"], [cc]])               # ... and (0, cc)
    u = c["u"].copy()
    u[[r, cc]] = 1.0
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order].astype(np.int32)
    rp = np.zeros(n + 1, np.int64)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=n))
    rp = rp.astype(np.int32)
    va = factored_values(rp, cols, u, u)
    e = int(rp[r]) + int(np.flatnonzero(cols[rp[r]:rp[r + 1]] == cc)[0])
    assert va[e] == 1.0 and rp[r + 1] - rp[r] == 2
    va[e] = (va[e:e + 1].view(np.int32) + ulps).view(np.float32)[0]
    c.update(rp=rp, ci=cols, va=va, u=u, nnz=len(cols), moved=(r, cc, e), lens=np.diff(rp).astype(np.int64), ulps=ulps,
             factoring=ulps * 2.0 ** -23 <= 4.8e-7)
    c["n_segs"] = expected_n_segs(n, c["nnz"], c["factoring"])
    c["layout"] = group_layout(n, n, c["n_segs"])
    return c


# ---- the twins -------------------------------------------------------------------------------------------------------------------
def twin(c, cut=None, narrow=False, only=None):
    """the fp64 oracle's result of every step (only: of these steps) -> list of arrays.  cut: every row keeps its first `cut`
    entries; narrow: the last feature column is dropped.  A refused case leaves C as the caller handed it over: zeros"""
    rp, ci, va = c["rp"], c["ci"], c["va"]
    if cut is not None:
        rp, ci, va = su.cut_rows(rp, cut, ci, va)
    out = []
    for i, s in enumerate(c["steps"]):
        if only is not None and i not in only:
            continue
        X = features(c, i)
        if narrow and s["k"] > 1:
            X = X[:, :-1]
        if s["op"] == "flexspmm" and c["n_segs"] == 0:
            out.append(np.zeros((c["m"], X.shape[1]), np.float32))
        elif s["op"] in ("flexspmm", "cuspmm"):
            out.append(oracle_spmm(rp, ci, va, X))
        elif s["op"] == "permutate":
            out.append(X[s["perm"]])
        else:
            trp, trow, tva = su.transpose_host(rp, ci, va, c["n"])
            out.append(oracle_spmm(trp, trow, tva, X))
    return out


# ---- csr2tile inside guarded buffers ---------------------------------------------------------------------------------------------
GUARD = 64
SENTINEL = 0x7FC12345                                  # (util.SENTINEL[4]: a NaN payload, compared as an integer)


def pack(rp, ci, va, m, n):
    """csr2tile on copies of the matrix, into buffers of the capacities gcn6.py:334-339 gives them (nnz, 2 * nnz, nnz, 256 and
    256 elements) between GUARD sentinel elements -> dict(seg_rowPtr, segNzCV, segVoMap, tail, next: the buffers as int32 /
    float32 views of their capacity, n_segs, untouched: name -> no element of the buffer was written, guards: no guard was)"""
    import ctypes
    from gcn_amd import _lib
    nnz = len(ci)
    caps = dict(segVoMap=nnz, seg_rowPtr=nnz, segNzCV=2 * nnz, tail=256, next=256)
    flat = {k: np.full(cap + 2 * GUARD, SENTINEL, np.int32) for k, cap in caps.items()}
    view = {k: f[GUARD:GUARD + caps[k]] for k, f in flat.items()}
    n_segs = np.full(1, -1, np.int32)
    ins = [np.ascontiguousarray(rp, np.int32).copy(), np.ascontiguousarray(ci, np.int32).copy(), np.ascontiguousarray(va, np.float32).copy()]
    kept = [a.copy() for a in ins]
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    vo = np.arange(n, dtype=np.int32)
    _lib.load().csr2tile(vp(ins[0]), vp(ins[1]), vp(ins[2]), m, n, nnz, vp(vo), vp(view["segVoMap"]), vp(view["seg_rowPtr"]),
                         vp(view["segNzCV"]), vp(view["tail"]), vp(view["next"]), 8, vp(n_segs))
    assert all(np.array_equal(a, b) for a, b in zip(ins, kept)), "csr2tile wrote its input"
    out = dict(view)
    out["segNzCV"] = view["segNzCV"].view(np.float32)
    out["n_segs"] = int(n_segs[0])
    out["guards"] = all(np.all(f[:GUARD] == SENTINEL) and np.all(f[GUARD + caps[k]:] == SENTINEL) for k, f in flat.items())
    out["untouched"] = {k: bool(np.all(v == SENTINEL)) for k, v in view.items()}
    return out
