"""The generator of the random-shape sweep over the plan-free units (tests/test_stress_units_cpu.py checks it without a GPU,
tests/test_stress_units_gpu.py runs it): ``case(seed, unit)`` returns, deterministically from the seed, one matrix and three
steps with their own sub-shape and parameters, as numpy arrays; ``twin(case)`` evaluates the host twins on it.

Matrix: m, n <= 4000 (the SpGEMM's B alone is 10 240 columns wide on the seeds that reach the dense class: a row's class is
min(products, n), so no narrower B has a row above SPGEMM_BLOCK_MAX), nnz <= 60 000, columns drawn with replacement, rows
column-sorted.  Row-length styles by seed % 4, as in test_stress_gpu._case: short rows with many empty ones; lengths at
b - 1, b, b + 1 of every bound b of the unit (and one row of exactly a bound's length right after a run of empty rows);
a few hubs up to 2 * 8192 + 1; dense-ish rows.  One seed in four — one of each style in every 16 — forces a long row (longer
than the unit's largest bound) at item 0, one at item m - 1, two side by side, and makes one of them a single repeated
column.  Values are eighths, features and gradients small integers: every sum is exact in fp32 in any order.

The first eight units came with the sweep; the head-batched and edge units were added later, and units added later append to
``UNITS`` (``_base`` seeds its generator with the unit's index, so the earlier cases stay bit for bit):

* ``heads``: edge_softmax and gat_edge_softmax on [nnz, H], spmm_heads, sddmm_heads and segment_sum on [nnz, H], through the
  public functions and their autograd on ONE adjacency.  H is a function of the seed (``H_LIST``), step 1 takes another H.
  The softmax family changes path at len * hp = 32 / 256 / 1024 ELEMENTS (hp = H on the fast route, 1 for one head and on
  the slow route), so the bounds are ``heads_bounds(H)``: those divided by hp, 8192, and the gather engine's 4 / 64 / 4096.
  Two of the five kinds have a width: those steps take ``F_LIST`` in turn within their style, so every F meets every style.
* ``gatv2``: gatv2_scores and its four gradients on the exact grid; ``edge_aggregate``: every (op, act, reduce) with both
  gradients, level-valued operands so that the selections tie.  Both draw one seed in two transposed (hub columns).
* ``sampled_dot``: P [q x q] samples X · Yᵀ in both modes, with own, given and no values, and one step goes through
  SparseProduct.values with at least one value vector given and the backward for what is given; rows of P around 64 and SAMPLE_LONG_ROW, rows of X around 16, 64 and it.
* ``linkpred``: find_edges and negative_sample interleaved on one column-sorted matrix with repeated columns and one row that
  stores every column; the launch and the tries are proven axis by axis, as the kNN's dimensions are (a negative_sample step
  of more than 65 queries keeps num_neg = 1 and at most 5 tries: the twin draws count * num_neg * max_tries Philox words).
* ``mixed``: three DIFFERENT units in turn on one square, mutable adjacency — they share its one cached ``tpattern()`` and its
  one Scratch keeper — and, one seed in two, new values between steps 1 and 2.  Its widths are taken in turn over the seeds;
  a style has fewer steps of a kind than there are widths, so they are proven over all styles together.

The matrices of these units keep two more caps, nnz * k <= 4 000 000 and nnz * H <= 2 000 000, by emptying ordinary rows; the
special rows (bound rows, hubs, forced rows) survive, and where they alone exceed a cap the step takes the widest width that
fits (``fit_width``; node arrays keep the same cap).  One step in two keeps every operand on a 16-byte boundary, since the
16-byte forms need all of them there.  Their operands are not kept on the case: ``step_inputs(c, i)`` draws them again."""
import numpy as np

from gcn_amd import _lib

UNITS = ("construct", "coalesce", "sampling", "aggregate", "attention", "sddmm", "spgemm", "knn",
         "heads", "gatv2", "edge_aggregate", "sampled_dot", "linkpred", "mixed")     # (units added later append: _base seeds by index)
K_LIST = (1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 64, 65, 100, 128, 200)
NNZ_MAX = 60000
NNZ_K_MAX, NNZ_H_MAX = 4_000_000, 2_000_000            # elements of an [nnz, k] and of an [nnz, H] array (and of a node array)
HUB_TOP = 2 * 8192 + 1
LONG = _lib.SAMPLE_LONG_ROW
# the head counts of the head-batched units: every fast-route count of edge_softmax.hip / multihead.hip (a power of two up to
# kMaxFastHeads = 16), slow-route ones, and one above kMaxFastHeads.  H is a function of the seed; at most 12 entries, so
# that every H meets every row-length style within 48 seeds (seed >> 2 takes 12 values in every style)
# (the fast-route counts sit where seed >> 2 is 2, 3, 6, 7: there the one clustered-length seed of a head count is not a forced
# one, whose long rows use up the budget of the rows around 8192)
H_LIST = (1, 3, 2, 4, 5, 32, 8, 16, 6, 12)
# head widths: F % 4 != 0 (VEC = 1) and F % 4 == 0 (VEC = 4 when the operands are aligned); U = F / VEC odd (4, 12), 2 mod 4
# (8) and 0 mod 4 (16, 32, 64): P = 1, 2, 4 lanes an (entry, head) of sddmm_heads; k = H F on both sides of 64, 128, 256
F_LIST = (1, 2, 3, 4, 5, 8, 12, 16, 17, 32, 33, 64, 65)
SOFTMAX_ELEMENTS = (32, 256, 1024)                     # len * hp of a row at which edge_softmax.hip changes path
SOFTMAX_LONG = 8192                                    # ... and the entries from which a row is split over blocks
GATHER_BOUNDS = (4, 64, 4096)                          # gather_rows.h: a slot's batch, a fetch of indices, the chunk


def head_pack(H):
    """hp of edge_softmax.hip: the heads of an entry that adjacent lanes share — H on the fast route, 1 for one head and on
    the slow route (a pass per head)"""
    return H if H in (2, 4, 8, 16) else 1


def heads_bounds(H):
    """the row lengths, in ENTRIES, at which a head-batched call of H heads changes path: the softmax family's element
    bounds divided by hp, its long-row bound, and the gather engine's"""
    return tuple(sorted({b // head_pack(H) for b in SOFTMAX_ELEMENTS} | {SOFTMAX_LONG} | set(GATHER_BOUNDS)))


# the row (item) lengths at which a unit's kernels change path
BOUNDS = {"construct": (64, _lib.BUCKET_WAVE_MAX, _lib.BUCKET_BLOCK_MAX),       # entries of a bucket
          "coalesce": (64, 128, 256, LONG),
          "sampling": (64, 256, LONG),                                           # sample.hip and subgraph.hip
          "aggregate": (4, 64, 4096),
          "attention": (32, 256, 1024, 8192),
          "sddmm": (64, 256),
          "spgemm": (64, _lib.SPGEMM_WAVE_MAX, _lib.SPGEMM_BLOCK_MAX),           # products of a row of A
          "knn": (32, 64),               # the feature chunk; KNN_TILE_Q = KNN_TILE_C = KNN_K_MAX (asserted in the CPU test)
          "heads": tuple(sorted({b for H in (1, 2, 4, 8, 16) for b in heads_bounds(H)})),   # (a case draws heads_bounds(its H))
          "gatv2": GATHER_BOUNDS,
          "edge_aggregate": GATHER_BOUNDS,
          "sampled_dot": (16, 64, LONG),                                         # rows of X (all three) and rows of P (LONG)
          "linkpred": (64, 256, LONG),                                           # the sampling unit's
          "mixed": GATHER_BOUNDS + (SOFTMAX_LONG,)}
WIDTH_UNITS = ("aggregate", "sddmm", "knn", "edge_aggregate")                    # (kNN's width is the feature count d)
HEAD_UNITS = ("heads", "gatv2")                                                  # widths k = H F, F of F_LIST
TWO_DTYPES = {"construct": ("int32", "int64"), "sampling": ("int32", "int64"), "coalesce": ("int32", "int64"),
              "aggregate": ("fp32", "bf16"), "sddmm": ("fp32", "bf16"), "linkpred": ("int32", "int64")}
LONG_ROW_UNITS = ("construct", "coalesce", "sampling", "aggregate", "attention", "spgemm",
                  "heads", "gatv2", "edge_aggregate", "sampled_dot", "linkpred", "mixed")
SPGEMM_WIDE_N = _lib.SPGEMM_BLOCK_MAX + _lib.SPGEMM_BLOCK_MAX // 4


def style_of(seed):
    return seed & 3


def forced(seed):
    return ((seed >> 2) & 3) == (seed & 3)


def row_lengths(rng, seed, m, bounds, cap=NNZ_MAX, keep=None):
    """-> (lens int64 [m], long rows placed by force: dict name -> row).  The special rows survive the cap; ordinary rows
    are emptied at random until the total fits.  keep: a set that receives the special rows"""
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
    if keep is not None:
        keep.update(special)
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


# ---- the units added after the first sweep ------------------------------------------------------------------------------------
# Their matrices carry two more caps (nnz * k <= NNZ_K_MAX for the widest step, nnz * H <= NNZ_H_MAX), reached by emptying
# ordinary rows; the special rows survive, and where they alone exceed a cap the step narrows its width (fit_width).  The
# operands of a step are not kept on the case (one may reach 4 000 000 elements): step_inputs(c, i) draws them again.
HEADS_OPS = ("edge_softmax", "gat_edge_softmax", "spmm_heads", "sddmm_heads", "segment_sum")
GATHER_KINDS = ("spmm_heads", "sddmm_heads", "gatv2_scores")                     # the kinds whose width is k = H F
MIXED_KINDS = ("aggregate", "edge_aggregate", "spmm_heads", "gatv2_scores", "edge_softmax", "sample_neighbors")
EDGE_TRIPLES = tuple((op, act, red) for op in ("add", "mul") for act in (None, "relu") for red in ("sum", "mean", "max", "min"))
QUERY_COUNTS = (1, 63, 64, 65, 65535, 65536, 65537)                              # both sides of 64 and of lookup.hip's kLookupSmall
NEW_UNITS = UNITS[8:]


def fit_width(widths, drawn, rows, per=1):
    """the largest width of `widths` not above `drawn` with rows * per * width <= NNZ_K_MAX"""
    return max([w for w in widths if w <= drawn and rows * per * w <= NNZ_K_MAX] or [min(widths)])


def step_heads(seed, i):
    """H of step i: the case's H (a function of the seed) at steps 0 and 2, ANOTHER one at step 1, so that the adjacency's
    scratch is outgrown and then under-used"""
    at = (seed >> 2) % len(H_LIST)
    return H_LIST[at if i != 1 else (at + 1 + seed % (len(H_LIST) - 1)) % len(H_LIST)]


def step_width(seed, i):
    fs = sorted(F_LIST[(3 * seed + j) % len(F_LIST)] for j in range(3))
    return (fs[0], fs[2], fs[1])[i]                    # narrow -> wide -> narrow


def _matrix(seed, unit, bounds, k_top=1, square=False, window=False, reserve=0):
    """_base with the caps of the later units -> (rng, case, special rows)"""
    rng = np.random.default_rng([seed, UNITS.index(unit)])
    m = int(rng.integers(12, (600 if style_of(seed) == 3 else 1500) + 1))
    n = m if square else int(rng.integers(1, 4001))
    special = set()
    lens, placed = row_lengths(rng, seed, m, bounds, cap=NNZ_MAX - reserve, keep=special)
    over = int(lens.sum()) - min(NNZ_MAX, NNZ_K_MAX // k_top)
    for r in rng.permutation(m):
        if over <= 0:
            break
        if int(r) not in special:
            over -= int(lens[r])
            lens[r] = 0
    if lens.sum() == 0:
        lens[m // 2] = 3
    rp, ci = csr_of_lengths(rng, lens, n, window, placed.get("pair2"))
    c = dict(seed=seed, unit=unit, style=style_of(seed), forced=forced(seed), placed=placed, m=m, n=n, rp=rp, ci=ci,
             va=eighths(rng, len(ci)), lens=np.diff(rp).astype(np.int64), adj_offsets=tuple(int(o) for o in rng.integers(0, 4, 3)),
             transposed=False)
    return rng, c, special


def _transpose_case(c):
    """the adjacency becomes the transpose of the drawn matrix: its COLUMNS have the drawn lengths (c["lens"] stays), and
    the backward walks over the transposed pattern meet them"""
    trp, trow, tva = transpose_host(c["rp"], c["ci"], c["va"], c["n"])
    c.update(rp=trp, ci=trow, va=tva, m=c["n"], n=c["m"], transposed=True)


def _align(s, seed, i):
    """one step in two keeps every operand on a 16-byte boundary: the 16-byte forms (VEC = 4) need ALL their operands
    there, which offsets drawn one by one from 0 .. 3 give once in 4^operands"""
    s["aligned"] = bool((seed + i + (seed >> 2)) & 1)
    if s["aligned"]:
        s["offsets"] = (0,) * 6


def vec_of(s, operands):
    """VEC as the kernels choose it (edgefeat.route, multihead.hip's `wide`): 4 when a head's (or the row's) width is a
    multiple of 4 and every one of the step's first `operands` operands starts on a 16-byte boundary, else 1"""
    return 4 if s.get("F", s["k"]) % 4 == 0 and all(o % 4 == 0 for o in s["offsets"][:operands]) else 1


HEADS_F_START = (1, 4, 1, 7)                            # where each style's turn through F_LIST begins


def heads_kinds(seed):
    return [HEADS_OPS[((seed & 3) + (seed >> 2) + i) % 5] for i in range(3)]


def heads_width(seed, i):
    """F of step i of the heads unit.  Only two of its five step kinds have a width, so its gather steps take F_LIST in turn
    WITHIN their row-length style (14 or 15 of them in 48 seeds, for 13 widths): every F meets every style"""
    before = sum(kind in GATHER_KINDS for earlier in range(seed & 3, seed, 4) for kind in heads_kinds(earlier))
    before += sum(kind in GATHER_KINDS for kind in heads_kinds(seed)[:i])
    return F_LIST[(before + HEADS_F_START[seed & 3]) % len(F_LIST)]


def _head_step(s, c, seed, i, kind, width=step_width):
    H, F = step_heads(seed, i), width(seed, i)
    rows = max(len(c["ci"]), c["m"], c["n"])
    s.update(kind=kind, H=H, F_drawn=F, F=fit_width(F_LIST, F, rows, H) if kind in GATHER_KINDS else 1)
    s["k"] = H * s["F"]
    _align(s, seed, i)


def _k_top(seed, kinds, width=step_width):
    """the widest k a case's steps ask for (what its nnz is capped for)"""
    return max(step_heads(seed, i) * (width(seed, i) if kind in GATHER_KINDS else 1) for i, kind in enumerate(kinds))


def _heads(seed):
    kinds = heads_kinds(seed)
    rng, c, _ = _matrix(seed, "heads", heads_bounds(step_heads(seed, 0)), _k_top(seed, kinds, heads_width))
    c.update(H=step_heads(seed, 0), hp=head_pack(step_heads(seed, 0)), steps=[])
    for i in range(3):
        s = _common(rng, seed, i, "heads")
        _head_step(s, c, seed, i, kinds[i], heads_width)
        s.update(op=kinds[i], rows=_row_range(rng, c["m"], i), slope=(0.2, 1.5)[int(rng.integers(0, 2))], perm=bool(rng.integers(0, 2)))
        c["steps"].append(s)
    return c


def _gatv2(seed):
    rng, c, _ = _matrix(seed, "gatv2", GATHER_BOUNDS, _k_top(seed, ["gatv2_scores"] * 3))
    if (seed >> 2) & 1 and c["style"] != 3:             # (one seed in two of every style but the dense-ish one)
        _transpose_case(c)
    c["steps"] = []
    for i in range(3):
        s = _common(rng, seed, i, "gatv2")
        _head_step(s, c, seed, i, "gatv2_scores")
        s.update(op="gatv2_scores", slope=(0.5, 0.25)[(seed + i + (seed >> 3)) & 1])
        c["steps"].append(s)
    return c


def _edge_step(s, c, seed, i):
    msg, act, reduce = EDGE_TRIPLES[(3 * seed + i) % len(EDGE_TRIPLES)]
    s.update(kind="edge_aggregate", msg=msg, act=act, reduce=reduce, k_drawn=s["k"],
             k=fit_width(K_LIST, s["k"], max(len(c["ci"]), c["m"], c["n"])))
    _align(s, seed, i)


def _edge_aggregate(seed):
    k_top = max(K_LIST[(3 * seed + j) % len(K_LIST)] for j in range(3))
    rng, c, _ = _matrix(seed, "edge_aggregate", GATHER_BOUNDS, k_top)
    if (seed >> 2) & 1 and c["style"] != 3:
        _transpose_case(c)
    c["steps"] = []
    for i in range(3):
        s = _common(rng, seed, i, "edge_aggregate")
        _edge_step(s, c, seed, i)
        s["op"] = s["msg"]
        c["steps"].append(s)
    return c


def mixed_kinds(seed):
    """three DIFFERENT kinds of MIXED_KINDS, a function of the seed"""
    a = seed + (seed >> 2)
    return tuple(MIXED_KINDS[(a + o) % 6] for o in (0, 1 + ((seed >> 2) & 1), 3 + (seed >> 3) % 3))


def mixed_width(seed, i, widths=F_LIST, kinds=GATHER_KINDS):
    """the width of step i of the mixed unit: the steps of `kinds` take `widths` in turn over the seeds (a seed has three
    steps of six kinds: the narrow-wide-narrow triples of the other units would leave widths out)"""
    before = sum(k in kinds for earlier in range(seed) for k in mixed_kinds(earlier)) + sum(k in kinds for k in mixed_kinds(seed)[:i])
    return widths[before % len(widths)]


def _mixed_k(seed, i):
    return mixed_width(seed, i, K_LIST, ("aggregate", "edge_aggregate"))


def _mixed(seed):
    """one square, mutable adjacency that three different units use in turn"""
    kinds = mixed_kinds(seed)
    k_top = max([_mixed_k(seed, i) for i, kind in enumerate(kinds) if kind in ("aggregate", "edge_aggregate")] + [_k_top(seed, kinds, mixed_width)])
    rng, c, _ = _matrix(seed, "mixed", BOUNDS["mixed"], k_top, square=True)
    heavy = np.argsort(-c["lens"], kind="stable")[:4]
    c.update(steps=[], update=bool(((seed >> 2) ^ seed) & 1), new_va=eighths(rng, len(c["ci"])))
    for i, kind in enumerate(kinds):
        s = _common(rng, seed, i, "mixed")
        s["k"] = _mixed_k(seed, i)
        if kind == "edge_aggregate":
            _edge_step(s, c, seed, i)
        elif kind == "aggregate":
            s.update(kind=kind, k_drawn=s["k"], k=fit_width(K_LIST, s["k"], max(len(c["ci"]), c["m"])), select=("max", "min")[(seed + i) & 1])
            _align(s, seed, i)
        elif kind == "sample_neighbors":
            ids = np.concatenate([rng.permutation(c["m"])[:int(rng.integers(1, c["m"] + 1))], heavy])
            s.update(kind=kind, k=1, ids=ids.astype(np.int64), fanout=int(rng.choice([1, 2, 5, 63, 64, 65, 256, 257, -1])))
        else:
            _head_step(s, c, seed, i, kind, mixed_width)
            s["slope"] = (0.5, 0.25)[(seed + i) & 1]
        s["op"] = kind
        c["steps"].append(s)
    return c


def _linkpred(seed):
    """a column-sorted matrix whose rows repeat columns (the window drawing), with one row that stores EVERY column: a
    negative for it is refused at every try"""
    rng, c, special = _matrix(seed, "linkpred", BOUNDS["linkpred"], window=True, reserve=4000)
    full = next(int(r) for r in rng.permutation(np.arange(1, c["m"] - 1)) if int(r) not in special)
    rp, ci, n = c["rp"].astype(np.int64), c["ci"], c["n"]
    ci = np.concatenate([ci[:rp[full]], np.arange(n, dtype=np.int32), ci[rp[full + 1]:]])
    lens = np.diff(rp)
    lens[full] = n
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    c.update(rp=rp, ci=ci, va=eighths(rng, len(ci)), lens=lens.astype(np.int64), full=full, steps=[])
    for i in range(3):
        s = _common(rng, seed, i, "linkpred")
        op = ("find_edges", "negative_sample")[(i + (seed >> 1)) & 1]           # interleaved: f n f or n f n
        count = QUERY_COUNTS[(seed + 3 * i + (seed >> 3)) % len(QUERY_COUNTS)]
        tries = int(rng.choice([1, 4, 5, 32, 64]))
        num_neg = int(rng.choice([1, 3]))
        if op == "negative_sample" and count > 65:      # (the twin draws count * num_neg * max_tries Philox words)
            tries, num_neg = min(tries, 5), 1
        s.update(op=op, kind=op, count=count, num_neg=num_neg, max_tries=tries, exclude_self=bool(rng.integers(0, 2)))
        c["steps"].append(s)
    return c


def _sampled_dot(seed):
    """P [q x q] samples X [q x w] · Y [q x w]ᵀ: X's rows are unsorted and repeat columns, Y's ascend strictly.  The twin is a
    Python loop over (entry of P) x (entries of X's row), so P's long rows belong to, and nearly always point at, short rows
    of X (test_sampled_dot_gpu.main_case's rule).  Values are eighths: a product is a 64th, every sum is exact"""
    rng = np.random.default_rng([seed, UNITS.index("sampled_dot")])
    style = style_of(seed)
    q = int(rng.integers(40, (300 if style == 3 else 800) + 1))
    w = int(rng.integers(8, 200))
    special = set()
    p_lens, placed = row_lengths(rng, seed, q, BOUNDS["sampled_dot"], cap=30000, keep=special)
    x_lens = rng.integers(0, 9, q)
    x_lens[rng.random(q) < 0.15] = 0
    free = [int(r) for r in rng.permutation(q) if p_lens[r] <= (100 if style == 3 else 8)]
    x_bounds = (15, 16, 17, 63, 64, 65) + ((LONG - 1, LONG, LONG + 1) if style in (1, 2) else ())
    for r, L in zip(free, x_bounds):
        x_lens[r] = L
    short = np.flatnonzero(x_lens <= 17)
    p_rows = np.repeat(np.arange(q), p_lens)
    p_cols = rng.choice(short, len(p_rows))
    anywhere = rng.random(len(p_rows)) < 0.03
    p_cols[anywhere] = rng.integers(0, q, int(anywhere.sum()))
    if "pair2" in placed:
        p_cols[p_rows == placed["pair2"]] = int(rng.choice(short))
    p_cols = p_cols[np.lexsort((p_cols, p_rows))]
    ptr = lambda lens: np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    y_rows = [np.sort(rng.choice(w, int(L), replace=False)) for L in rng.integers(0, min(w, 40) + 1, q)]
    c = dict(seed=seed, unit="sampled_dot", style=style, forced=forced(seed), placed=placed, m=q, n=q, w=w, rp=ptr(p_lens),
             ci=p_cols.astype(np.int32), va=eighths(rng, len(p_cols)), lens=p_lens.astype(np.int64), x_lens=x_lens.astype(np.int64),
             x_rp=ptr(x_lens), x_ci=rng.integers(0, w, int(x_lens.sum())).astype(np.int32), y_rp=ptr([len(r) for r in y_rows]),
             y_ci=np.concatenate(y_rows).astype(np.int32), adj_offsets=tuple(int(o) for o in rng.integers(0, 4, 3)), steps=[])
    c.update(x_va=eighths(rng, len(c["x_ci"])), y_va=eighths(rng, len(c["y_ci"])))
    # the product step: A = the first ra rows of X, every row cut to 65 entries (the twin walks X's row once per entry of
    # C), B = Yᵀ, C's pattern by scipy on patterns of ones (nothing cancels)
    import scipy.sparse as sp
    ra = min(q, max(12, 20000 // q))
    sub = sub_rows(c["x_rp"], 0, ra, c["x_ci"], c["x_va"])
    a_rp, a_ci, a_va = cut_rows(sub[0], 65, sub[1], sub[2])
    ones = lambda rp_, ci_, shape: sp.csr_matrix((np.ones(len(ci_)), ci_.astype(np.int64), rp_.astype(np.int64)), shape=shape)
    C = (ones(a_rp, a_ci, (ra, w)) @ ones(c["y_rp"], c["y_ci"], (q, w)).T).tocsr()
    C.sort_indices()
    c["prod"] = dict(ra=ra, a_rp=a_rp, a_ci=a_ci, a_va=a_va, c_rp=C.indptr.astype(np.int32), c_ci=C.indices.astype(np.int32))
    for i in range(3):
        s = _common(rng, seed, i, "sampled_dot")
        op = ("dot", "dot_by_col", "product")[(seed + i + (seed >> 2)) % 3]
        xm, ym = (("own", "given", "none")[int(rng.integers(0, 3))] for _ in range(2))
        if op == "product":                             # (a_values / b_values: given, or the operand's own — never both the
            xm, ym = (v if v != "none" else "own" for v in (xm, ym))            # operands' own: a backward runs at every product step)
            if xm == ym == "own":
                xm, ym = (("given", "own"), ("own", "given"))[(seed >> 2) & 1]
        nx = len(a_ci) if op == "product" else len(c["x_ci"])
        s.update(op=op, kind=op, x_mode=xm, y_mode=ym, xv=eighths(rng, nx) if xm == "given" else None,
                 yv=eighths(rng, len(c["y_ci"])) if ym == "given" else None, g=eighths(rng, len(C.indices)))
        c["steps"].append(s)
    return c


def step_inputs(c, i):
    """the operands of step i of a later unit, drawn from (seed, unit, step) at every call -> dict of arrays.  Grids: node
    features small integers, per-entry weights eighths (halves for edge_aggregate: with five feature levels nearly every
    selection ties), softmax scores in [-8, 8)"""
    s = c["steps"][i]
    rng = np.random.default_rng([c["seed"], UNITS.index(c["unit"]), i, 1])
    m, n, nnz, kind = c["m"], c["n"], len(c["ci"]), s["kind"]
    H, k = s.get("H", 1), s.get("k", 1)
    ints = lambda top, *shape: rng.integers(-top, top + 1, shape).astype(np.float32)
    if kind in ("edge_softmax", "segment_sum"):
        return dict(scores=(rng.random((nnz, H)) * 16 - 8).astype(np.float32), g=ints(8, nnz, H), perm=rng.permutation(nnz).astype(np.int32))
    if kind == "gat_edge_softmax":
        return dict(a_dst=(rng.random((m, H)) * 8 - 4).astype(np.float32), a_src=(rng.random((n, H)) * 8 - 4).astype(np.float32),
                    g=ints(8, nnz, H))
    if kind == "spmm_heads":
        return dict(x=ints(3, n, k), vals=(rng.integers(0, 8, (nnz, H)) / 8.0).astype(np.float32), g=ints(3, m, k))
    if kind == "sddmm_heads":
        return dict(a=ints(3, m, k), b=ints(3, n, k), g=(rng.integers(-7, 8, (nnz, H)) / 8.0).astype(np.float32))
    if kind == "gatv2_scores":
        return dict(hd=ints(2, m, k), hs=ints(2, n, k), att=ints(2, H, s["F"]), g=(rng.integers(-7, 8, (nnz, H)) / 8.0).astype(np.float32))
    if kind == "edge_aggregate":
        return dict(x=ints(2, n, k), w=(rng.integers(-2, 3, (nnz, k)) / 2.0).astype(np.float32), g=ints(3, m, k))
    if kind == "aggregate":
        return dict(x=ints(2, n, k), g=ints(8, m, k))
    if kind == "find_edges":                            # stored pairs, their neighbours, the full row, ids out of range
        e = rng.integers(0, nnz, s["count"])
        rows = (np.searchsorted(c["rp"], e, side="right") - 1).astype(np.int64)
        cols = c["ci"][e].astype(np.int64) + rng.choice([0, 0, 0, 1, -1], s["count"])
        odd = rng.random(s["count"])
        rows = np.where(odd < 0.05, rng.choice([-1, m, m + 7, c["full"]], s["count"]), rows)
        cols = np.where(odd > 0.95, rng.choice([-1, n, n + 5], s["count"]), cols)
        if s["count"] >= 63:                            # (both ends of both ranges, whatever was drawn)
            rows[:2], cols[2:4] = (-1, m), (-1, n)
        return dict(q_rows=rows, q_cols=cols)
    if kind == "negative_sample":
        rows = rng.integers(0, m, s["count"])
        odd = rng.random(s["count"])
        rows = np.where(odd < 0.1, rng.choice([-1, m, m + 7, c["full"], int(np.argmax(c["lens"]))], s["count"]), rows)
        rows[0] = c["full"]
        if s["count"] >= 63:
            rows[1:3] = (-1, m)
        return dict(q_rows=rows.astype(np.int64))
    return {}


_MAKERS = dict(construct=_construct, coalesce=_coalesce, sampling=_sampling, aggregate=_aggregate, attention=_attention,
               sddmm=_sddmm, spgemm=_spgemm, knn=_knn, heads=_heads, gatv2=_gatv2, edge_aggregate=_edge_aggregate,
               sampled_dot=_sampled_dot, linkpred=_linkpred, mixed=_mixed)
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
        if unit in NEW_UNITS:
            out.append(twin_step(c, i, cut, narrow))
            continue
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


def drop_last_of_every_head(a, H):
    """[rows, H F] -> [rows, H (F - 1)]: every head loses its last column"""
    return np.ascontiguousarray(a.reshape(len(a), H, -1)[:, :, :-1].reshape(len(a), -1))


def dot_operands(c, i, cut=None):
    """a sampled_dot step as sampled_dot_ref takes it: (p = (rowptr, col), number of columns of p, x = (rowptr, col, values
    or None), y likewise, the common width, x_by_col).  The product step samples A · B on C's pattern with X = A and
    Y = Bᵀ = Y (B's stable transpose has Y's entry order again, because Y's rows ascend strictly)"""
    s = c["steps"][i]
    xv = {"own": c["x_va"], "given": s["xv"], "none": None}[s["x_mode"]]
    yv = {"own": c["y_va"], "given": s["yv"], "none": None}[s["y_mode"]]
    if s["op"] == "product":
        pr = c["prod"]
        p, x = (pr["c_rp"], pr["c_ci"]), (pr["a_rp"], pr["a_ci"], pr["a_va"] if s["x_mode"] == "own" else xv)
    else:
        p, x = (c["rp"], c["ci"]), (c["x_rp"], c["x_ci"], xv)
    if cut is not None:
        x = cut_rows(x[0], cut, x[1], x[2])
        if s["op"] != "product":
            p = cut_rows(p[0], cut, p[1])
    return p, c["n"], x, (c["y_rp"], c["y_ci"], yv), c["w"], s["op"] == "dot_by_col"


def twin_step(c, i, cut=None, narrow=False):
    """the twin of step i of a later unit -> tuple of arrays (a per-entry result is followed by its row sums, so that a cut
    changes values and not only shapes)"""
    import edge_aggregate_ref as ea
    import gatv2_ref
    import heads_ref
    from linkpred_ref import find_entries_ref, negative_sample_ref
    from sampled_dot_ref import sampled_dot_ref
    from sampling_ref import sample_neighbors_ref
    s = c["steps"][i]
    kind, H = s["kind"], s.get("H", 1)
    if c["unit"] == "sampled_dot":
        p, np_cols, x, y, w, by_col = dot_operands(c, i, cut)
        vals = sampled_dot_ref(p[0], p[1], np_cols, *x, *y, w, x_by_col=by_col)
        return vals, heads_ref.row_sums(p[0], vals[:, None])
    x = step_inputs(c, i)
    rp, ci = c["rp"], c["ci"]
    keep = np.ones(len(ci), bool)
    if cut is not None:
        keep = (np.arange(len(ci)) - np.repeat(rp[:-1].astype(np.int64), np.diff(rp))) < cut
        rp, ci = cut_rows(rp, cut, ci)
    if kind == "find_edges":
        return (find_entries_ref(rp, ci, x["q_rows"], x["q_cols"]),)
    if kind == "negative_sample":
        return (negative_sample_ref(rp, ci, c["n"], x["q_rows"], s["num_neg"], *s["philox"], s["max_tries"], s["exclude_self"]),)
    if kind == "sample_neighbors":
        return sample_neighbors_ref(rp, ci, s["ids"], s["fanout"], *s["philox"])
    if kind == "edge_softmax":
        sc = x["scores"][keep]
        return heads_ref.edge_softmax(rp, sc), heads_ref.row_sums(rp, sc)
    if kind == "gat_edge_softmax":
        sc = heads_ref.gat_scores(rp, ci, x["a_dst"], x["a_src"], s["slope"])
        return heads_ref.edge_softmax(rp, sc), heads_ref.row_sums(rp, sc)
    if kind == "segment_sum":
        sub, xs, perm = segment_operands(c, i, x, keep)
        return (heads_ref.segment_sum(sub, xs, perm),)
    if kind == "aggregate":
        return select_host(rp, ci, x["x"][:, :-1] if narrow and s["k"] > 1 else x["x"], s["select"])
    if kind == "edge_aggregate":
        xx, ww = (x["x"][:, :-1], x["w"][keep][:, :-1]) if narrow and s["k"] > 1 else (x["x"], x["w"][keep])
        return ea.forward(rp, ci, xx, ww, s["msg"], s["act"], s["reduce"])
    less = (lambda a: drop_last_of_every_head(a, H)) if narrow and s["F"] > 1 else (lambda a: a)
    if kind == "spmm_heads":
        return (heads_ref.spmm_heads(rp, ci, None, x["vals"][keep], less(x["x"]), H),)
    if kind == "sddmm_heads":
        out = heads_ref.sddmm_heads(rp, ci, less(x["a"]), less(x["b"]), H)
        return out, heads_ref.row_sums(rp, out)
    if kind == "gatv2_scores":
        att = x["att"][:, :-1] if narrow and s["F"] > 1 else x["att"]
        out = gatv2_ref.scores(rp, ci, less(x["hd"]), less(x["hs"]), att, s["slope"])
        return out, heads_ref.row_sums(rp, out)
    raise KeyError(kind)


def segment_operands(c, i, x, keep=None):
    """(rowptr of the step's rows, their entries of x [., H], the permutation to read them through or None): as in the
    attention unit, a stretch of the rows through a permutation of its own entries"""
    s, rp = c["steps"][i], c["rp"]
    lo, hi = s["rows"]
    b, e = int(rp[lo]), int(rp[hi])
    k = np.ones(e - b, bool) if keep is None else keep[b:e]
    lens = np.bincount(np.repeat(np.arange(hi - lo), np.diff(rp[lo:hi + 1]))[k], minlength=hi - lo)
    sub = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    perm = np.argsort(x["perm"][b:e][k]).astype(np.int32) if s["perm"] else None
    return sub, x["scores"][b:e][k], perm


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
