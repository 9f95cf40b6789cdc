"""The generator of the random-shape sweep over the plan-free units (tests/test_stress_units_cpu.py checks it without a GPU,
tests/test_stress_units_gpu.py runs it): ``case(seed, unit)`` returns, deterministically from the seed, one matrix and three
steps with their own sub-shape and parameters, as numpy arrays; ``twin(case)`` evaluates the host twins on it.

Matrix: m, n <= 4000 (the SpGEMM's B alone is 10 240 columns wide on the seeds that reach the dense class: a row's class is
min(products, n), so no narrower B has a row above SPGEMM_BLOCK_MAX), nnz <= 60 000, columns drawn with replacement, rows
column-sorted.  Row-length styles by seed % 4, as in test_stress_gpu._case: short rows with many empty ones; lengths at
b - 1, b, b + 1 of every bound b of the unit (and one row of exactly a bound's length right after a run of empty rows);
a few hubs up to 2 * 8192 + 1; dense-ish rows.  One seed in four — one of each style in every 16 — forces a long row (longer
than the unit's largest bound) at item 0, one at item m - 1, two side by side, and makes one of them a single repeated
column.  Values are eighths, features and gradients small integers: every sum is exact in fp32 in any order."""
import numpy as np

from gcn_amd import _lib

UNITS = ("construct", "coalesce", "sampling", "aggregate", "attention", "sddmm", "spgemm", "knn")
K_LIST = (1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 64, 65, 100, 128, 200)
NNZ_MAX = 60000
HUB_TOP = 2 * 8192 + 1
LONG = _lib.SAMPLE_LONG_ROW
# the row (item) lengths at which a unit's kernels change path
BOUNDS = {"construct": (64, _lib.BUCKET_WAVE_MAX, _lib.BUCKET_BLOCK_MAX),       # entries of a bucket
          "coalesce": (64, 128, 256, LONG),
          "sampling": (64, 256, LONG),                                           # sample.hip and subgraph.hip
          "aggregate": (4, 64, 4096),
          "attention": (32, 256, 1024, 8192),
          "sddmm": (64, 256),
          "spgemm": (64, _lib.SPGEMM_WAVE_MAX, _lib.SPGEMM_BLOCK_MAX),           # products of a row of A
          "knn": (32, 64)}               # the feature chunk; KNN_TILE_Q = KNN_TILE_C = KNN_K_MAX (asserted in the CPU test)
WIDTH_UNITS = ("aggregate", "sddmm", "knn")                                      # (kNN's width is the feature count d)
TWO_DTYPES = {"construct": ("int32", "int64"), "sampling": ("int32", "int64"), "coalesce": ("int32", "int64"),
              "aggregate": ("fp32", "bf16"), "sddmm": ("fp32", "bf16")}
LONG_ROW_UNITS = ("construct", "coalesce", "sampling", "aggregate", "attention", "spgemm")
SPGEMM_WIDE_N = _lib.SPGEMM_BLOCK_MAX + _lib.SPGEMM_BLOCK_MAX // 4


def style_of(seed):
    return seed & 3


def forced(seed):
    return ((seed >> 2) & 3) == (seed & 3)


def row_lengths(rng, seed, m, bounds, cap=NNZ_MAX):
    """-> (lens int64 [m], long rows placed by force: dict name -> row).  The special rows survive the cap; ordinary rows
    are emptied at random until the total fits"""
    style, top = style_of(seed), max(bounds)
    special = {}
    if style == 0:
        lens = rng.integers(0, 4, m)
        lens[rng.random(m) < 0.4] = 0
    elif style == 1:
        lens = rng.choice([0, 1, 2, 3, 5, 8], m)
        free = rng.permutation(np.arange(4, m - 2))
        at = 0
        for b in bounds:
            for L in (b - 1, b, b + 1):
                special[int(free[at])] = L
                at += 1
        b = int(rng.choice(bounds))                     # exactly a bound's length right after an empty run
        r = int(free[at])
        for e in range(max(0, r - 3), r):
            if e not in special:
                special[e] = 0
        special[r] = b
    elif style == 2:
        lens = rng.integers(0, 6, m)
        hubs = [HUB_TOP if (seed >> 3) & 1 else int(rng.integers(top + 1, HUB_TOP + 1)), top + 1 + int(rng.integers(0, 100)),
                int(rng.integers(200, 1400))]
        for r, L in zip(rng.permutation(np.arange(1, m - 1))[:3], hubs):
            special[int(r)] = L
    else:
        lens = rng.integers(20, 90, m)
    lens[rng.random(m) < 0.15] = 0
    placed = {}
    if forced(seed):
        r = int(rng.integers(2, m - 3))
        placed = {"first": 0, "last": m - 1, "pair": r, "pair2": r + 1}
        for row in placed.values():
            special[row] = top + 1 + int(rng.integers(0, 40))
    total = 0
    for r, L in sorted(special.items(), key=lambda kv: (kv[0] not in placed.values(), kv[0])):
        if total + L > cap - 2000 and r not in placed.values():
            L = int(rng.integers(0, 8))                 # (the budget is spent: an ordinary row instead)
        lens[r] = L
        total += L
    ordinary = np.array([r for r in rng.permutation(m) if r not in special], np.int64)
    over = int(lens.sum()) - cap
    for r in ordinary:
        if over <= 0:
            break
        over -= int(lens[r])
        lens[r] = 0
    if lens.sum() == 0:
        lens[m // 2] = 3
    assert lens.sum() <= cap
    return lens.astype(np.int64), placed


def csr_of_lengths(rng, lens, n, window=False, repeats_row=None):
    """(rowptr int32, col int32) with the given row lengths, columns drawn with replacement (`window`: from a window of
    0.75 x the row's length around the diagonal, so that about half of a row's entries repeat a column and the diagonal is
    often there), rows column-sorted; the row `repeats_row` holds one column only"""
    m = len(lens)
    rows = np.repeat(np.arange(m), lens)
    if window:
        width = np.maximum(2, (0.75 * lens).astype(np.int64))[rows]
        cols = (rows + (rng.random(len(rows)) * width).astype(np.int64) - width // 2) % n
    else:
        cols = rng.integers(0, n, len(rows))
    if repeats_row is not None:
        cols[rows == repeats_row] = int(rng.integers(0, n))
    order = np.lexsort((cols, rows))
    rp = np.zeros(m + 1, np.int64)
    rp[1:] = np.cumsum(lens)
    return rp.astype(np.int32), cols[order].astype(np.int32)


def eighths(rng, count):
    """non-zero multiples of 1/8 in [-1, 1]"""
    return ((rng.integers(1, 9, count) * rng.choice([-1, 1], count)) / 8).astype(np.float32)


def sub_rows(rp, lo, hi, *per_entry):
    """the rows [lo, hi) of a CSR: (rowptr rebased, the slices of the per-entry arrays)"""
    b, e = int(rp[lo]), int(rp[hi])
    return ((rp[lo:hi + 1] - rp[lo]).astype(np.int32),) + tuple(a[b:e] if a is not None else None for a in per_entry)


def cut_rows(rp, cut, *per_entry):
    """every row cut to its first `cut` entries"""
    lens = np.minimum(np.diff(rp), cut)
    keep = (np.arange(int(rp[-1])) - np.repeat(rp[:-1], np.diff(rp))) < cut
    out = np.zeros(len(rp), np.int32)
    out[1:] = np.cumsum(lens)
    return (out,) + tuple(a[keep] if a is not None else None for a in per_entry)


def transpose_host(rp, ci, va, n):
    """(rowptr, row of each entry, values) of the transpose, a column's entries by ascending source entry"""
    order = np.argsort(ci, kind="stable")
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    trp = np.zeros(n + 1, np.int64)
    trp[1:] = np.cumsum(np.bincount(ci, minlength=n))
    return trp.astype(np.int32), rows[order].astype(np.int32), va[order]


def _common(rng, seed, i, unit):
    """the parameters every step draws: width, dtype, operand offsets, stream"""
    ks = sorted(K_LIST[(3 * seed + j) % len(K_LIST)] for j in range(3))
    k = (ks[0], ks[2], ks[1])[i]                       # narrow -> wide -> narrow
    dtypes = TWO_DTYPES.get(unit, ("fp32",))
    return dict(k=int(k), dtype=dtypes[(seed + i + (seed >> 2)) % len(dtypes)], offsets=tuple(int(o) for o in rng.integers(0, 4, 6)),
                side_stream=bool((seed + i + (seed >> 1)) & 1), philox=(int(rng.integers(0, 2 ** 40)), int(rng.integers(0, 2 ** 34))))


def _row_range(rng, m, i):
    """step 0 takes every row, the later steps a stretch of at least a third of them"""
    if i == 0 or m < 6:
        return 0, m
    lo = int(rng.integers(0, m // 3))
    return lo, int(rng.integers(lo + m // 3, m + 1))


def _base(seed, unit, square=False, window=False, m_top=1500, n_top=4000):
    rng = np.random.default_rng([seed, UNITS.index(unit)])
    m = int(rng.integers(12, (600 if style_of(seed) == 3 else m_top) + 1))
    n = m if square else int(rng.integers(1, n_top + 1))
    lens, placed = row_lengths(rng, seed, m, BOUNDS[unit])
    rp, ci = csr_of_lengths(rng, lens, n, window, placed.get("pair2"))
    c = dict(seed=seed, unit=unit, style=style_of(seed), forced=forced(seed), placed=placed, m=m, n=n, rp=rp, ci=ci,
             va=eighths(rng, len(ci)), lens=np.diff(rp).astype(np.int64), adj_offsets=tuple(int(o) for o in rng.integers(0, 4, 3)))
    return rng, c


# ---- the units --------------------------------------------------------------------------------------------------------------
def _construct(seed):
    """the matrix's entries as an edge list in a drawn order; the buckets are its rows (bucket_by_key, csr_from_edges) or,
    for transpose_csr, the columns of its transpose"""
    rng, c = _base(seed, "construct")
    rows = np.repeat(np.arange(c["m"]), c["lens"])
    order = {0: np.arange(len(rows)), 1: np.arange(len(rows))[::-1].copy(), 2: rng.permutation(len(rows))}[seed % 3]
    c.update(e_rows=rows[order].astype(np.int64), e_cols=c["ci"][order].astype(np.int64), e_vals=c["va"][order])
    ops = ("bucket_by_key", "csr_from_edges", "transpose_csr")
    c["steps"] = []
    for i in range(3):
        s = _common(rng, seed, i, "construct")
        s.update(op=ops[(seed + i) % 3], rows=_row_range(rng, c["m"], i), sort_columns=bool(rng.integers(0, 2)),
                 raw=bool(rng.integers(0, 2)))
        c["steps"].append(s)
    return c


def _coalesce(seed):
    rng, c = _base(seed, "coalesce", square=True, window=True, m_top=1200)
    perm = rng.permutation(len(c["ci"]))
    rows = np.repeat(np.arange(c["m"]), c["lens"])
    c.update(e_rows=rows[perm].astype(np.int64), e_cols=c["ci"][perm].astype(np.int64), e_vals=np.abs(c["va"])[perm])
    ops = ("coalesce_csr", "symmetrize", "normalize_csr", "gcn_adjacency")
    c["steps"] = []
    for i in range(3):
        s = _common(rng, seed, i, "coalesce")
        s.update(op=ops[(seed + (seed >> 2) + i) % 4] if i else "coalesce_csr", rows=_row_range(rng, c["m"], i),
                 reduce=("sum", "max", "min", "first")[int(rng.integers(0, 4))], diagonal=("keep", "drop", "fill", "add")[int(rng.integers(0, 4))],
                 diag_value=float(rng.integers(1, 9)) / 8, norm=("sym", "row")[int(rng.integers(0, 2))])
        if s["op"] == "symmetrize":                    # (its contract has no "first")
            s["reduce"] = ("max", "sum", "min")[int(rng.integers(0, 3))]
        c["steps"].append(s)
    return c


def _sampling(seed):
    rng, c = _base(seed, "sampling", square=True)
    ops = ("sample_neighbors", "sample_blocks", "induced_subgraph", "random_walk")
    m = c["m"]
    heavy = np.argsort(-c["lens"], kind="stable")[:4]
    c["steps"] = []
    for i in range(3):
        s = _common(rng, seed, i, "sampling")
        op = ops[(seed + (seed >> 2) + i) % 4]
        count = int(rng.integers(1, m + 1))
        ids = rng.permutation(m)[:count]
        if op == "sample_blocks":                       # distinct seeds, few of them: the frontier grows by the fanout
            ids = np.unique(np.concatenate([ids[:40], heavy[:2]]))
            ids = rng.permutation(ids)
        elif op == "induced_subgraph":
            ids = np.union1d(ids, heavy)
            ids = rng.permutation(ids) if rng.integers(0, 2) else ids
        elif op == "random_walk":
            ids = rng.integers(0, m, int(rng.choice([1, 63, 64, 65, 700])))
        else:
            ids = np.concatenate([ids, heavy, ids[:3]])  # (seeds may repeat)
        s.update(op=op, ids=ids.astype(np.int64), fanout=int(rng.choice([1, 2, 5, 63, 64, 65, 256, 257, -1])),
                 fanouts=[int(rng.choice([1, 2, 3, 5, -1])), int(rng.choice([1, 2, 3]))], length=int(rng.choice([0, 1, 3, 4, 5, 8])))
        c["steps"].append(s)
    return c


def _aggregate(seed):
    """transposed: the adjacency is the transpose of the drawn matrix, so that its COLUMNS have the drawn lengths and the
    backward's walk over the transposed pattern meets them (hub columns)"""
    rng, c = _base(seed, "aggregate")
    c["transposed"] = bool((seed >> 1) & 1) and c["style"] != 3
    if c["transposed"]:
        trp, trow, tva = transpose_host(c["rp"], c["ci"], c["va"], c["n"])
        c.update(rp=trp, ci=trow, va=tva, m=c["n"], n=c["m"])
    c["mutable"] = bool((seed >> 2) & 1)                # (a mutable adjacency keeps its own transpose and permutation)
    c["steps"] = []
    for i in range(3):
        s = _common(rng, seed, i, "aggregate")
        s.update(op=("max", "min")[(seed + i) & 1], linear=("sum", "mean")[(seed >> 1) & 1] if i == 1 else None)
        s["x"] = rng.integers(-2, 3, (c["n"], s["k"])).astype(np.float32)           # level_features: nearly every element ties
        s["g"] = rng.integers(-8, 9, (c["m"], s["k"])).astype(np.float32)           # int_grad
        c["steps"].append(s)
    return c


def _attention(seed):
    rng, c = _base(seed, "attention")
    ops = ("edge_softmax", "gat_edge_softmax", "segment_sum")
    c["steps"] = []
    for i in range(3):
        s = _common(rng, seed, i, "attention")
        nnz = len(c["ci"])
        s.update(op=ops[(seed + i) % 3], rows=_row_range(rng, c["m"], i), slope=(0.2, 1.5)[int(rng.integers(0, 2))],
                 scores=(rng.random(nnz) * 16 - 8).astype(np.float32), g=rng.integers(-8, 9, nnz).astype(np.float32),
                 a_dst=(rng.random(c["m"]) * 8 - 4).astype(np.float32), a_src=(rng.random(c["n"]) * 8 - 4).astype(np.float32),
                 perm=rng.permutation(nnz).astype(np.int32) if rng.integers(0, 2) else None)
        c["steps"].append(s)
    return c


def _sddmm(seed):
    rng, c = _base(seed, "sddmm")
    c["plan"] = (dict(slices=0), dict(slices=4), dict(), dict(slices=0, panels=1), dict(slices=2))[(seed >> 2) % 5]
    c["steps"] = []
    for i in range(3):
        s = _common(rng, seed, i, "sddmm")
        s["A"] = rng.integers(-8, 9, (c["m"], s["k"])).astype(np.float32)           # int_features
        s["B"] = rng.integers(-8, 9, (c["n"], s["k"])).astype(np.float32)
        c["steps"].append(s)
    return c


def _spgemm(seed):
    """A [m x p] · B [p x n].  B's rows 0 .. 5 have 512 distinct columns each, rows 6 .. 11 64, rows 12 .. 19 one, row 20
    none, the others 0 .. 12; a row of A whose drawn length is u gets exactly u PRODUCTS (u // 512 entries on the first
    group, then on the second, the rest on the single-column rows, in a random order) — the count that decides its class,
    as in test_spgemm_gpu.class_pair.  b_dup: B with some entries repeated, for spgemm(assume_coalesced=False)."""
    rng = np.random.default_rng([seed, UNITS.index("spgemm")])
    style = style_of(seed)
    m = int(rng.integers(12, 400))
    n = SPGEMM_WIDE_N if style in (1, 2) or forced(seed) else int(rng.integers(1, 4001))
    p = int(rng.integers(30, 300))
    targets, placed = row_lengths(rng, seed, m, BOUNDS["spgemm"], cap=70000)
    if style == 3:                                      # (fewer products on the ordinary rows: the twin is a Python loop)
        keep = np.array(sorted(placed.values()), np.int64)
        kept = targets[keep]
        targets = targets // 4
        targets[keep] = kept
    b_lens = rng.integers(0, 13, p)
    b_lens[:6], b_lens[6:12], b_lens[12:20], b_lens[20] = 512, 64, 1, 0
    b_lens = np.minimum(b_lens, n)
    b_rows = [rng.choice(n, int(L), replace=False) for L in b_lens]
    if rng.integers(0, 2):                              # B's rows need not be sorted
        b_rows = [np.sort(r) for r in b_rows]
    b_rp = np.zeros(p + 1, np.int32)
    b_rp[1:] = np.cumsum(b_lens)
    b_ci = np.concatenate(b_rows).astype(np.int32)
    a_rows, products = [], np.zeros(m, np.int64)
    L512, L64 = int(b_lens[0]), int(b_lens[6])
    for r in range(m):
        u = int(targets[r])
        if r in placed.values() or style in (1, 2) or u > 12:
            ent = []
            for L, lo, hi in ((L512, 0, 6), (L64, 6, 12), (int(b_lens[12]), 12, 20)):
                cnt, u = (divmod(u, L) if L else (0, u))
                ent += list(rng.integers(lo, hi, cnt))
            if rng.integers(0, 3) == 0:
                ent.append(20)                          # an entry on B's empty row
        else:
            ent = list(rng.integers(0, p, u))
            ent = [j for j in ent if j >= 12]           # (keeps the ordinary rows cheap)
        ent = rng.permutation(np.array(ent, np.int64))
        a_rows.append(ent)
        products[r] = int(b_lens[ent].sum()) if len(ent) else 0
    a_rp = np.zeros(m + 1, np.int32)
    a_rp[1:] = np.cumsum([len(e) for e in a_rows])
    a_ci = np.concatenate(a_rows).astype(np.int32)
    c = dict(seed=seed, unit="spgemm", style=style, forced=forced(seed), placed=placed, m=m, n=n, p=p, rp=a_rp, ci=a_ci,
             va=eighths(rng, len(a_ci)), b_rp=b_rp, b_ci=b_ci, b_va=eighths(rng, len(b_ci)), lens=products,
             adj_offsets=tuple(int(o) for o in rng.integers(0, 4, 3)))
    rep = np.where(rng.random(len(b_ci)) < 0.1, 2, 1)
    rep[b_rp[0]:b_rp[6]] = 1
    d_rp = np.zeros(p + 1, np.int32)
    d_rp[1:] = np.cumsum(np.bincount(np.repeat(np.repeat(np.arange(p), b_lens), rep), minlength=p))
    c.update(d_rp=d_rp, d_ci=np.repeat(b_ci, rep), d_va=eighths(rng, int(rep.sum())))
    ops = ("raw", "spgemm", "raw")
    c["steps"] = []
    for i in range(3):
        s = _common(rng, seed, i, "spgemm")
        s.update(op=ops[(seed + i) % 3], rows=_row_range(rng, m, i), pattern=(None, "a", "b")[int(rng.integers(0, 3))])
        c["steps"].append(s)
    return c


def _knn(seed):
    rng = np.random.default_rng([seed, UNITS.index("knn")])
    c = dict(seed=seed, unit="knn", style=style_of(seed), forced=forced(seed), placed={}, steps=[])
    dims = []
    for i in range(3):
        s = _common(rng, seed, i, "knn")
        q = int(rng.choice([1, 2, 63, 64, 65, 130]))
        n = int(rng.choice([1, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 1000]))
        d = s["k"] if (seed % 7, i) != (3, 2) else (31, 32)[(seed // 7) & 1]    # (K_LIST has neither side of the feature chunk)
        while q * n * d > 2_000_000:
            n = max(65, n // 2)
            q = min(q, 65)
        k = int(rng.choice([1, 2, 10, 63, 64]))
        s.update(op=("raw", "knn", "raw_guarded")[(seed + i) % 3], q=q, n=n, d=d, knn_k=k, splits=int(rng.choice([0, 1, 2, 3, 7])),
                 self_offset=int(rng.integers(0, n - q + 1)) if n >= q and rng.integers(0, 2) else -1,
                 ldx=d + int(rng.integers(0, 4)), ldy=d + int(rng.integers(0, 4)),
                 x=rng.integers(-8, 9, (q, d)).astype(np.float32), y=rng.integers(-8, 9, (n, d)).astype(np.float32))   # int_points
        dims += [q, n, d]
        c["steps"].append(s)
    c["lens"] = np.array(dims, np.int64)
    return c


_MAKERS = dict(construct=_construct, coalesce=_coalesce, sampling=_sampling, aggregate=_aggregate, attention=_attention,
               sddmm=_sddmm, spgemm=_spgemm, knn=_knn)
_CASES = {}


def case(seed, unit):
    """everything the three steps of (seed, unit) need, as numpy arrays; the same at every call (kept: the arrays are
    read, never written)"""
    if (seed, unit) not in _CASES:
        _CASES[(seed, unit)] = _MAKERS[unit](int(seed))
    return _CASES[(seed, unit)]


def describe(c, i):
    """(seed, group, step, drawn parameters) for an assertion message"""
    s = c["steps"][i]
    small = {k: v for k, v in s.items() if not isinstance(v, np.ndarray)}
    return f"seed {c['seed']} {c['unit']} step {i} style {c['style']} forced {c['forced']} shape {c.get('m')}x{c.get('n')} {small}"


# ---- the host twins, per unit: what the GPU steps are compared with (and what the CPU test discriminates on) -------------------
def sddmm_host(rp, ci, A, B):
    """(d*, sum_j |A_rj B_cj|) in fp64 on the host: util.sddmm_ref without a device"""
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    ref, mag = np.zeros(len(ci)), np.zeros(len(ci))
    for i in range(0, len(ci), 1 << 14):
        prod = A[rows[i:i + (1 << 14)]].astype(np.float64) * B[ci[i:i + (1 << 14)]].astype(np.float64)
        ref[i:i + (1 << 14)], mag[i:i + (1 << 14)] = prod.sum(1), np.abs(prod).sum(1)
    return ref, mag


def softmax_host(rp, s):
    """fp64 softmax over each row's entries"""
    lens = np.diff(rp.astype(np.int64))
    ne = lens > 0
    if not ne.any():
        return np.zeros(0)
    starts, seg = rp[:-1][ne].astype(np.int64), np.repeat(np.arange(int(ne.sum())), lens[ne])
    e = np.exp(s.astype(np.float64) - np.maximum.reduceat(s.astype(np.float64), starts)[seg])
    return e / np.add.reduceat(e, starts)[seg]


def select_host(rp, ci, x, op):
    """ref_select of test_aggregate_gpu.py (kept here so that the CPU test needs no GPU module)"""
    m, k = len(rp) - 1, x.shape[1]
    out, arg = np.zeros((m, k), x.dtype), np.full((m, k), -1, np.int32)
    pick, jj = (np.argmax if op == "max" else np.argmin), np.arange(k)
    for r in range(m):
        b, e = int(rp[r]), int(rp[r + 1])
        if e > b:
            slab = x[ci[b:e]]
            a = pick(slab, axis=0)
            out[r], arg[r] = slab[a, jj], b + a
    return out, arg


def step_matrix(c, i, cut=None):
    """(rowptr, col, val) a step works on: the case's matrix, cut, then the step's rows"""
    rp, ci, va = c["rp"], c["ci"], c["va"]
    if cut is not None:
        rp, ci, va = cut_rows(rp, cut, ci, va)
    lo, hi = c["steps"][i].get("rows", (0, len(rp) - 1))
    return sub_rows(rp, lo, hi, ci, va)


def twin(c, cut=None, narrow=False):
    """the twins' outputs of the three steps -> list of tuples of arrays.  cut: every row (item) cut to its first `cut`
    entries before the steps run; narrow: the last feature column dropped (the units with a width)"""
    from coalesce_ref import coalesce_ref, gcn_adjacency_ref, normalize_ref, degree_ref, symmetrize_ref
    from construct_ref import bucket_ref, csr_from_edges_ref, transpose_ref
    from knn_ref import knn_ref
    from sampling_ref import sample_blocks_ref, sample_neighbors_ref
    from spgemm_ref import sorted_merged_ref, spgemm_ref
    from subgraph_ref import induced_subgraph_ref, random_walk_ref
    unit, out = c["unit"], []
    for i, s in enumerate(c["steps"]):
        if unit == "knn":
            x, y = s["x"], s["y"]
            if cut is not None:
                x, y = x[:, :cut], y[:, :cut]
            if narrow and s["d"] > 1:
                x, y = x[:, :-1], y[:, :-1]
            out.append(knn_ref(x, y, s["knn_k"], s["self_offset"]))
            continue
        rp, ci, va = step_matrix(c, i, cut)
        m = len(rp) - 1
        if unit == "construct":
            e_rows, e_cols, e_vals = edge_list(c, i, cut)
            if s["op"] == "bucket_by_key":
                out.append(bucket_ref(e_rows, m))
            elif s["op"] == "csr_from_edges":
                out.append(csr_from_edges_ref(e_rows, e_cols, (m, c["n"]), e_vals, s["sort_columns"]))
            else:
                trp, trow, tva = transpose_host(rp, ci, va, c["n"])
                out.append(transpose_ref(trp, trow, tva, m))
        elif unit == "coalesce":
            n = c["n"]
            if s["op"] == "coalesce_csr":
                out.append(coalesce_ref(rp, ci, va, n, s["reduce"], s["diagonal"], s["diag_value"]))
            elif s["op"] == "symmetrize":
                sq = square_part(c, i, cut)
                merged = coalesce_ref(*sq, len(sq[0]) - 1, "sum")[:3]
                out.append(symmetrize_ref(*merged, s["reduce"]))
            elif s["op"] == "normalize_csr":
                sq = square_part(c, i, cut)
                va_pos = np.abs(sq[2])
                out.append((normalize_ref(sq[0], sq[1], va_pos, degree_ref(sq[0], va_pos), s["norm"]),))
            else:
                e_rows, e_cols, e_vals = edge_list(c, i, cut, square=True)
                out.append(gcn_adjacency_ref(e_rows, e_cols, s["rows"][1] - s["rows"][0], values=e_vals, reduce=s["reduce"] if s["reduce"] != "first" else "max",
                                             self_loops=s["diagonal"], norm=s["norm"]))
        elif unit == "sampling":
            rp, ci, va = (c["rp"], c["ci"], c["va"]) if cut is None else cut_rows(c["rp"], cut, c["ci"], c["va"])
            seed, offset = s["philox"]
            if s["op"] == "sample_neighbors":
                out.append(sample_neighbors_ref(rp, ci, s["ids"], s["fanout"], seed, offset))
            elif s["op"] == "sample_blocks":
                blocks, ids = sample_blocks_ref(rp, ci, va, s["ids"], s["fanouts"], seed, offset)
                out.append(tuple(b[key] for b in blocks for key in ("rowptr", "col", "eid", "src_ids")) + (ids,))
            elif s["op"] == "induced_subgraph":
                out.append(induced_subgraph_ref(rp, ci, s["ids"], c["n"]))
            else:
                out.append((random_walk_ref(rp, ci, s["ids"], s["length"], seed, offset),))
        elif unit == "aggregate":
            x = s["x"][:, :-1] if narrow and s["k"] > 1 else s["x"]
            out.append(select_host(rp, ci, x, s["op"]))
        elif unit == "attention":
            lo, hi = int(c["rp"][s["rows"][0]]), int(c["rp"][s["rows"][1]])
            if cut is None:
                sc = s["scores"][lo:hi]
            else:
                keep = (np.arange(int(c["rp"][-1])) - np.repeat(c["rp"][:-1], np.diff(c["rp"]))) < cut
                sc = s["scores"][lo:hi][keep[lo:hi]]
            out.append((softmax_host(rp, sc), np.bincount(np.repeat(np.arange(m), np.diff(rp)), weights=sc.astype(np.float64), minlength=m)))
        elif unit == "sddmm":
            A, B = (s["A"][:, :-1], s["B"][:, :-1]) if narrow and s["k"] > 1 else (s["A"], s["B"])
            out.append(sddmm_host(rp, ci, A, B))
        elif unit == "spgemm":
            if s["op"] == "spgemm":
                b = sorted_merged_ref(c["d_rp"], c["d_ci"], c["d_va"])
            else:
                b = (c["b_rp"], c["b_ci"], c["b_va"])
            a_va, b_va = (None if s["pattern"] == "a" and s["op"] == "raw" else va), (None if s["pattern"] == "b" and s["op"] == "raw" else b[2])
            if cut is not None:                         # (cut counts PRODUCTS: entries of A are dropped from the end of the row)
                rp, ci, a_va = cut_products(rp, ci, a_va, c["b_rp"] if s["op"] != "spgemm" else b[0], cut)
            out.append(spgemm_ref(rp, ci, a_va, b[0], b[1], b_va, c["p"], c["n"]))
    return out


def cut_products(rp, ci, va, b_rp, cut):
    """the entries of every row of A whose running product count stays <= cut"""
    m = len(rp) - 1
    blen = np.diff(b_rp)[ci].astype(np.int64)
    rows, csum, ne = np.repeat(np.arange(m), np.diff(rp)), np.cumsum(blen), np.diff(rp) > 0
    base = np.zeros(m, np.int64)
    base[ne] = (csum - blen)[rp[:-1][ne]]
    keep = csum - base[rows] <= cut
    out = np.zeros(m + 1, np.int32)
    out[1:] = np.cumsum(np.bincount(rows[keep], minlength=m))
    return out, ci[keep], va[keep] if va is not None else None


def edge_list(c, i, cut=None, square=False):
    """the case's edges, in their drawn order, that lie in the step's rows (rebased to them; `square`: and in its columns)"""
    lo, hi = c["steps"][i]["rows"]
    r, k, v = c["e_rows"], c["e_cols"], c["e_vals"]
    keep = (r >= lo) & (r < hi)
    if square:
        keep &= (k >= lo) & (k < hi)
    if cut is not None:                                 # the first `cut` edges of every row, in the edge list's order
        order = np.argsort(r, kind="stable")
        rank = np.empty(len(r), np.int64)
        starts = np.zeros(c["m"] + 1, np.int64)
        starts[1:] = np.cumsum(np.bincount(r, minlength=c["m"]))
        rank[order] = np.arange(len(r)) - starts[r[order]]
        keep &= rank < cut
    return r[keep] - lo, (k[keep] - lo) if square else k[keep], v[keep]


def square_part(c, i, cut=None):
    """the principal submatrix of the step's rows: (rowptr, col, val), column-sorted (what symmetrize and the symmetric
    normalisation need: a square matrix)"""
    rp, ci, va = step_matrix(c, i, cut)
    lo, hi = c["steps"][i]["rows"]
    rows = np.repeat(np.arange(hi - lo), np.diff(rp))
    keep = (ci >= lo) & (ci < hi)
    out = np.zeros(hi - lo + 1, np.int32)
    out[1:] = np.cumsum(np.bincount(rows[keep], minlength=hi - lo))
    return out, (ci[keep] - lo).astype(np.int32), va[keep]
