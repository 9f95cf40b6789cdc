"""Shared helpers for the tests: the oracle bindings and small graph builders.
The oracle is test infrastructure (oracle/README.md); nothing here is product code."""
import ctypes
import os

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        _oracle = ctypes.CDLL(os.path.join(ROOT, "oracle", "libspmm_oracle.so"))
    return _oracle


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def oracle_spmm(rowptr, col, val, B, fp64=True):
    """CPU oracle C = A @ B (fp64 accumulate by default), numpy arrays in/out."""
    rowptr = np.ascontiguousarray(rowptr, np.int32); col = np.ascontiguousarray(col, np.int32)
    val = np.ascontiguousarray(val, np.float32); B = np.ascontiguousarray(B, np.float32)
    m, k = len(rowptr) - 1, B.shape[1]
    C = np.empty((m, k), np.float32)
    fn = oracle().spmm_oracle_f64 if fp64 else oracle().spmm_oracle_f32
    fn(_p(rowptr), _p(col), _p(val), _p(B), _p(C), m, k)
    return C


def rel_err(C, Cref):
    """max|C - C*| / max|C*|  — the parity metric of BASELINE.md §3 (tolerance 1e-5)."""
    denom = float(np.abs(Cref).max())
    return float(np.abs(C.astype(np.float64) - Cref.astype(np.float64)).max()) / (denom if denom > 0 else 1.0)


def random_csr(m, n, nnz_target, seed, empty_rows=0.0, long_rows=(), sorted_cols=True):
    """Random CSR with optional empty rows and a few very long rows (hub rows)."""
    rng = np.random.default_rng(seed)
    lens = rng.poisson(max(nnz_target / max(m, 1), 0.01), m).astype(np.int64)
    if empty_rows > 0:
        lens[rng.random(m) < empty_rows] = 0
    for r, L in long_rows:
        lens[r] = L
    lens = np.minimum(lens, n)
    rowptr = np.zeros(m + 1, np.int64); rowptr[1:] = np.cumsum(lens)
    col = np.empty(rowptr[-1], np.int32)
    for r in range(m):
        c = rng.choice(n, size=lens[r], replace=False) if lens[r] <= n // 2 else rng.permutation(n)[:lens[r]]
        col[rowptr[r]:rowptr[r + 1]] = np.sort(c) if sorted_cols else c
    val = (rng.standard_normal(rowptr[-1]) * 0.5).astype(np.float32)
    return rowptr.astype(np.int32), col, val


def sym_norm_graph(n, e, seed):
    """Â = D^-1/2 (A+I) D^-1/2 for a random undirected graph (fp64 → fp32 like utils.py:78-90)."""
    rng = np.random.default_rng(seed)
    u, v = rng.integers(0, n, e), rng.integers(0, n, e)
    A = sp.coo_matrix((np.ones(e), (u, v)), shape=(n, n)); A = (A + A.T).tocsr()
    A.setdiag(0); A.eliminate_zeros(); A.data[:] = 1.0
    A = (A + sp.eye(n)).tocsr()
    d = np.asarray(A.sum(1)).ravel() ** -0.5
    A = (sp.diags(d) @ A @ sp.diags(d)).tocsr(); A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float32)


def ref_build_graphs():
    """the random graphs the reorderers are compared with the reference build on (tests/test_reorder.py); their
    recorded outputs are tests/golden/refbuild_<name>.npz (oracle/make_golden.py)"""
    yield "sym_2k", sym_norm_graph(2000, 20000, seed=10)
    yield "sym_sparse", sym_norm_graph(3000, 4000, seed=11)
    rng = np.random.default_rng(12)                      # skewed, asymmetric, with self-loops
    n, e = 1500, 12000
    u = np.minimum(n - 1, (n * rng.random(e) ** 2.5).astype(int)); v = rng.integers(0, n, e)
    A = sp.coo_matrix((np.ones(e), (u, v)), shape=(n, n)).tocsr(); A = (A + sp.eye(n)).tocsr()
    A.data[:] = rng.random(A.nnz) + 0.1; A.sort_indices()
    yield "directed_skewed", (A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float32))
    # R-MAT, products-shaped degree skew (hub rows, many equal dQ candidates): the case where Rabbit's
    # "first maximum in key order" tie rule and the equal-degree introsort permutation really matter
    from gcn_amd import graphgen
    rowptr, col, val, _ = graphgen.make_graph("products", device="cpu", seed=3, scale=0.006)
    yield "rmat_products_shaped", (rowptr.numpy(), col.numpy(), val.numpy())


def arrays_sha256(*arrays):
    """one digest of dtypes, shapes and bytes: how the golden files record outputs too large to store"""
    import hashlib
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype.str}{a.shape}".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def sampled_rows_oracle_err(rowptr_dev, col_dev, val_dev, B_dev, C_dev, rows):
    """rel. error of C_dev[rows] against the fp64 C oracle on a compacted copy of the sampled rows: only the rows
    of B the sample references travel to the host (full-size configs: B has tens of GB).  All *_dev are torch
    tensors on one device; rows a sorted numpy int64 array.  → (rel_err, entries_checked)"""
    import torch
    dev = C_dev.device
    r = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(dev)
    rp = rowptr_dev.long()
    start, lens = rp[r], rp[r + 1] - rp[r]
    seg = torch.repeat_interleave(torch.arange(len(rows), device=dev), lens)
    first = torch.cumsum(lens, 0) - lens
    e = start[seg] + (torch.arange(int(lens.sum()), device=dev) - first[seg])
    cols = col_dev[e].long()
    uniq, inv = torch.unique(cols, return_inverse=True)
    sub_rp = np.zeros(len(rows) + 1, np.int32)
    sub_rp[1:] = np.cumsum(lens.cpu().numpy())
    Cref = oracle_spmm(sub_rp, inv.to(torch.int32).cpu().numpy(), val_dev[e].cpu().numpy(), B_dev[uniq].cpu().numpy())
    return rel_err(C_dev[r].cpu().numpy(), Cref), int(e.numel())


# ---- operands at chosen alignments, and the dropout mask's reference ----
SENTINEL = {4: 0x7FC12345, 2: 0x7FC1}                   # NaN payloads (fp32 / bf16), compared as integers
_INT_VIEW = {4: "int32", 2: "int16"}


def _as_int(t):
    import torch
    return t.view(getattr(torch, _INT_VIEW[t.element_size()]))


def offset_view(t_or_shape, off, dtype, device, guard=64):
    """A contiguous tensor whose first element lies `off` elements past a 16-byte boundary, with `guard` sentinel
    elements on either side: → (view, flat).  `t_or_shape`: a tensor / array to copy in, or a shape (the view then
    holds sentinels too: an output that must be written everywhere)."""
    import torch
    src = None
    if isinstance(t_or_shape, (tuple, list, torch.Size)):
        shape = tuple(int(s) for s in t_or_shape)
    elif isinstance(t_or_shape, int):
        shape = (t_or_shape,)
    else:
        src = t_or_shape if isinstance(t_or_shape, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t_or_shape))
        shape = tuple(src.shape)
    numel = int(np.prod(shape, dtype=np.int64)) if shape else 1
    itemsize = torch.empty((), dtype=dtype).element_size()
    assert (guard * itemsize) % 16 == 0, "guard must keep the buffer's 16-byte phase"
    flat = torch.empty(guard + off + numel + guard, dtype=dtype, device=device)
    assert flat.data_ptr() % 16 == 0
    _as_int(flat).fill_(SENTINEL[itemsize])              # (int32 index arrays too: no valid index is that large)
    view = flat[guard + off: guard + off + numel].view(shape)
    if src is not None:
        view.copy_(src.to(device=device, dtype=dtype))
    assert view.data_ptr() % 16 == (off * itemsize) % 16
    assert view.is_contiguous()
    return view, flat


def guards_intact(flat, view):
    """every element of `flat` outside `view` still holds the sentinel's bits"""
    import torch
    itemsize = flat.element_size()
    lo = (view.data_ptr() - flat.data_ptr()) // itemsize
    hi = lo + view.numel()
    f, want = _as_int(flat), SENTINEL[itemsize]
    return bool(torch.all(f[:lo] == want)) and bool(torch.all(f[hi:] == want))


def philox4x32_10(counter_words, key_words):
    """Philox4x32-10 (Salmon et al., SC'11) on arrays: counter_words = (c0, c1, c2, c3), key_words = (k0, k1), each an
    array (or scalar) of 32-bit values → the four result words as uint64 arrays holding 32-bit values."""
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    mask, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[np.asarray(w, dtype=np.uint64) for w in (*counter_words, *key_words)])
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                        # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> sh, p0 & mask, p1 >> sh, p1 & mask
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + W0) & mask, (k1 + W1) & mask
    return c0, c1, c2, c3


def dropout_threshold(p):
    """keep iff word >= threshold (include/gcn_spmm.h): p as the float32 the C ABI receives"""
    t = float(np.float32(p)) * 4294967296.0
    return 0xFFFFFFFF if t >= 4294967295.0 else int(np.floor(t))


def dropout_keep(count, p, seed, offset):
    """keep[i] of the dropout contract of include/gcn_spmm.h: word i % 4 of Philox4x32-10 with counter (i / 4, offset)
    and key seed, kept iff >= p * 2^32"""
    seed, offset = int(seed), int(offset)
    j = np.arange((count + 3) // 4, dtype=np.uint64)
    words = philox4x32_10((j & np.uint64(0xFFFFFFFF), j >> np.uint64(32), offset & 0xFFFFFFFF, offset >> 32),
                          (seed & 0xFFFFFFFF, seed >> 32))
    w = np.stack(words, axis=1).reshape(-1)[:count]
    return w >= np.uint64(dropout_threshold(p))


def dropout_keep_at(indices, p, seed, offset):
    """keep[i] of the same contract at the given flat indices (any shape, up to 2^64) without generating the stream before them"""
    seed, offset = int(seed), int(offset)
    i = np.asarray(indices).astype(np.uint64)
    j = i >> np.uint64(2)
    words = philox4x32_10((j & np.uint64(0xFFFFFFFF), j >> np.uint64(32), offset & 0xFFFFFFFF, offset >> 32),
                          (seed & 0xFFFFFFFF, seed >> 32))
    lane = i & np.uint64(3)
    w = np.select([lane == 0, lane == 1, lane == 2], words[:3], words[3])
    return w >= np.uint64(dropout_threshold(p))


# ---- builders, references and bounds that more than one test module uses ----
def banded_csr(n, half_band, extra, seed, hub=None):
    """near-diagonal matrix (what a renumbered community graph looks like) + a few far entries"""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for r in range(n):
        lo, hi = max(0, r - half_band), min(n, r + half_band + 1)
        c = rng.choice(np.arange(lo, hi), size=min(hi - lo, int(rng.integers(0, 2 * half_band // 3 + 2))), replace=False)
        far = rng.integers(0, n, extra)
        cc = np.unique(np.concatenate([c, far]))
        if hub is not None and r == hub[0]:
            cc = np.unique(rng.choice(n, hub[1], replace=False))
        rows.append(np.full(len(cc), r)); cols.append(cc)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    A = sp.csr_matrix((rng.standard_normal(len(rows)).astype(np.float32), (rows, cols)), shape=(n, n))
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float32)


def dense_band_csr(n, half_band, density, seed, sparse_from=None):
    """rows hold `density` of the columns within +-half_band of the diagonal (rows >= sparse_from: 3 % instead),
    plus a few far entries: the 128 x 512 windows of the panels are 25-60 % dense"""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for r in range(n):
        lo, hi = max(0, r - half_band), min(n, r + half_band + 1)
        dens = density if sparse_from is None or r < sparse_from else 0.03
        c = np.flatnonzero(rng.random(hi - lo) < dens) + lo
        far = rng.integers(0, n, 2)
        c = np.unique(np.concatenate([c, far]))
        rows.append(np.full(len(c), r)); cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    A = sp.csr_matrix(((rng.standard_normal(len(rows)) * 0.5).astype(np.float32), (rows, cols)), shape=(n, n))
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float32)


def with_duplicate_entries(rp, ci, va, every=7):
    """repeat every `every`-th entry in place (duplicate (r, c) entries; rows stay column-sorted)"""
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    rep = np.ones(len(ci), dtype=np.int64)
    rep[::every] = 2
    ci2, rows2 = np.repeat(ci, rep), np.repeat(rows, rep)
    va2 = np.repeat(va, rep) * np.float32(0.5)
    rp2 = np.zeros(len(rp), dtype=np.int32)
    rp2[1:] = np.cumsum(np.bincount(rows2, minlength=len(rp) - 1))
    return rp2, ci2.astype(np.int32), va2.astype(np.float32)


_SDDMM_GRAPHS = {}


def sddmm_graph(name):
    """the graphs of tests/test_sddmm_gpu.py: (rowptr, col, val, m, n) numpy"""
    from gcn_amd import graphgen
    if name not in _SDDMM_GRAPHS:
        if name == "rect":                                   # m != n, empty rows, hub rows, duplicates
            rp, ci, va = random_csr(700, 1300, 30000, seed=5, empty_rows=0.1, long_rows=((3, 400), (10, 900)))
            rp, ci, va = with_duplicate_entries(rp, ci, va)
            _SDDMM_GRAPHS[name] = (rp, ci, va, 700, 1300)
        elif name == "sym":                                  # normalised: the values factor
            rp, ci, va = sym_norm_graph(3000, 90000, seed=2)
            _SDDMM_GRAPHS[name] = (rp, ci, va, 3000, 3000)
        else:                                                # runs the group kernels when sliced (slices=4)
            rp, ci, va, n = graphgen.make_graph("reddit", device="cpu", seed=1, scale=0.02)
            rp, ci, va = rp.numpy(), ci.numpy(), va.numpy()
            rp, ci, va = with_duplicate_entries(rp, ci, va, every=101)
            _SDDMM_GRAPHS[name] = (rp, ci, va, n, n)
    return _SDDMM_GRAPHS[name]


def sddmm_ref(rp, ci, A, B, device):
    """(d*, sum_j |A_rj B_cj|) in fp64, evaluated on the device in pieces"""
    import torch
    rows = torch.from_numpy(np.repeat(np.arange(len(rp) - 1), np.diff(rp))).to(device)
    cols = torch.from_numpy(ci.astype(np.int64)).to(device)
    Ad, Bd = (torch.from_numpy(np.ascontiguousarray(x)).to(device).double() for x in (A, B))
    ref, mag = [], []
    for i in range(0, len(ci), 1 << 18):
        p = Ad[rows[i:i + (1 << 18)]] * Bd[cols[i:i + (1 << 18)]]
        ref.append(p.sum(1))
        mag.append(p.abs().sum(1))
    if not ref:
        return np.zeros(0), np.zeros(0)
    return torch.cat(ref).cpu().numpy(), torch.cat(mag).cpu().numpy()


def check_sddmm(out, ref, mag):
    d = out.cpu().numpy().astype(np.float64)
    excess = np.abs(d - ref) - (1e-5 * mag + 1e-30)
    assert excess.max() <= 0.0, f"bound exceeded by {excess.max():.3e} at {excess.argmax()}"


BF16_EPS = 2.0 ** -8


def bf16_reference(rowptr, col, val, B):
    """(C*, |A|.|B|) in fp64 accumulation on the upcast bf16 operand"""
    Bf = B.float().cpu().numpy()
    return (oracle_spmm(rowptr, col, val, Bf).astype(np.float64),
            oracle_spmm(rowptr, col, np.abs(val), np.abs(Bf)).astype(np.float64))


def bf16_assert_bound(C, Cref, absref, bf16_out, scale=1.0):
    C = C.float().cpu().numpy().astype(np.float64)
    bound = scale * (BF16_EPS * absref + (BF16_EPS * np.abs(Cref) if bf16_out else 0.0)) + 1e-6
    excess = np.abs(C - Cref) - bound
    assert excess.max() <= 0.0, f"bound exceeded by {excess.max():.3e} at {np.unravel_index(excess.argmax(), excess.shape)}"


# ---- exact-arithmetic and element-wise checks of the fp32 / bf16 SpMM (test_exact_cpu.py, test_exact_gpu.py) ----
# Leg 1: operands whose every fp32 partial sum is exact in any order, so the result must EQUAL the fp64 oracle.
# Leg 2: operands spanning 2^+-34 in scale, every element within (L_i + 16) u of its own |A|.|B| (u = 2^-24).
def with_duplicates(rowptr, col, val, seed, frac_rows=0.5, u_row=None, u_col=None):
    """the same pattern with 2-5 copies of some entries (copies sit next to the original: rows stay column-sorted).
    Values of the copies: random (the matrix then does not factor), or u_row[r]*u_col[c] when factors are given."""
    rng = np.random.default_rng(seed)
    m = len(rowptr) - 1
    lens = np.diff(rowptr)
    rep = np.ones(len(col), np.int64)
    rows_of = np.repeat(np.arange(m), lens)
    pick_rows = rng.random(m) < frac_rows
    cand = np.flatnonzero(pick_rows[rows_of] & (rng.random(len(col)) < 0.15))
    rep[cand] = rng.integers(2, 6, len(cand))
    if len(col):                                        # the first and the last entry of the matrix too (chunk edges)
        rep[0], rep[-1] = 3, 5
    col2 = np.repeat(col, rep)
    rows2 = np.repeat(rows_of, rep)
    if u_row is not None:
        val2 = (u_row[rows2].astype(np.float64) * u_col[col2].astype(np.float64)).astype(np.float32)
    else:
        val2 = np.repeat(val, rep)
        extra = np.ones(len(col2), bool)
        extra[np.cumsum(rep) - rep] = False             # the first copy keeps the original value
        val2[extra] = (rng.standard_normal(int(extra.sum())) * 0.5).astype(np.float32)
    rp2 = np.zeros(m + 1, np.int64)
    np.add.at(rp2, rows2 + 1, 1)
    rp2 = np.cumsum(rp2)
    return rp2.astype(np.int32), col2.astype(np.int32), val2.astype(np.float32)


def reshape_rows(rowptr, col, n, seed, empty=0.05, hub=None, keep_diagonal=False, spare=()):
    """pattern only: a fraction `empty` of the rows (row 1 and the last row among them) loses its entries — all but the
    diagonal with keep_diagonal — and row hub[0] gets hub[1] distinct random columns instead of its own (and keeps its
    diagonal with keep_diagonal); the rows `spare` stay as they are -> (rowptr, col), rows column-sorted"""
    rng = np.random.default_rng(seed)
    m = len(rowptr) - 1
    rows = np.repeat(np.arange(m), np.diff(rowptr))
    drop = rng.random(m) < empty
    drop[[1, m - 1]] = True
    drop[list(spare)] = False
    if hub is not None:
        drop[hub[0]] = True                             # (its own entries go, the hub's come below)
    keep = ~drop[rows]
    if keep_diagonal:
        keep |= col == rows
    rows, cols = rows[keep], col[keep].astype(np.int64)
    if hub is not None:
        hc = rng.choice(n, hub[1], replace=False)
        if keep_diagonal:
            hc = hc[hc != hub[0]]
        rows, cols = np.concatenate([rows, np.full(len(hc), hub[0])]), np.concatenate([cols, hc])
    order = np.lexsort((cols, rows))
    rp = np.zeros(m + 1, np.int64)
    rp[1:] = np.cumsum(np.bincount(rows, minlength=m))
    return rp.astype(np.int32), cols[order].astype(np.int32)


def random_rows_csr(m, n, lens, seed):
    """pattern with the given row lengths, columns drawn with replacement (so some repeat), rows column-sorted; vectorised
    (the matrices of millions of entries)"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    rows = np.repeat(np.arange(m), lens)
    cols = rng.integers(0, n, len(rows))
    order = np.lexsort((cols, rows))
    rp = np.zeros(m + 1, np.int64)
    rp[1:] = np.cumsum(lens)
    return rp.astype(np.int32), cols[order].astype(np.int32)


def _rows_of(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def int_features(n, k, seed, top=8):
    """integers in [-top, top] (top <= 8)"""
    assert 0 < top <= 8
    return np.random.default_rng(seed).integers(-top, top + 1, (n, k)).astype(np.float32)


def int_values(nnz, seed):
    """non-zero integers in [-4, 4]"""
    rng = np.random.default_rng(seed)
    return (rng.integers(1, 5, nnz) * rng.choice([-1, 1], nnz)).astype(np.float32)


def pow2_factors(n, seed):
    """u = 2^-e, e in {0, 1, 2, 3}"""
    return (2.0 ** -np.random.default_rng(seed).integers(0, 4, n)).astype(np.float32)


def factored_values(rowptr, col, u_row, u_col):
    """val[r, c] = u_row[r] * u_col[c], the exact product rounded once to fp32 (what the fp32 product gives too)"""
    return (u_row[_rows_of(rowptr)].astype(np.float64) * u_col[col].astype(np.float64)).astype(np.float32)


def wide_features(n, k, seed):
    """standard_normal * 2^(p_c + q_j): an exponent in [-12, 12] per row of B and one per column"""
    rng = np.random.default_rng(seed)
    p, q = rng.integers(-12, 13, n), rng.integers(-12, 13, k)
    return (rng.standard_normal((n, k)) * 2.0 ** (p[:, None] + q[None, :])).astype(np.float32)


def wide_values(rowptr, seed):
    """N(0, 0.5) * 2^s_r, s_r in [-10, 10] per row"""
    rng = np.random.default_rng(seed)
    s = rng.integers(-10, 11, len(rowptr) - 1)
    return (rng.standard_normal(int(rowptr[-1])) * 0.5 * 2.0 ** s[_rows_of(rowptr)]).astype(np.float32)


def wide_factors(n, seed):
    """(0.5 + rand) * 2^a, a in [-10, 10]"""
    rng = np.random.default_rng(seed)
    return ((0.5 + rng.random(n)) * 2.0 ** rng.integers(-10, 11, n)).astype(np.float32)


def _granule_log2(x):
    """the smallest g >= 0 with x * 2^g all integers (asserted to exist below 2^-24)"""
    x = np.asarray(x, np.float64).ravel()
    for g in range(0, 25):
        y = x * 2.0 ** g
        if np.array_equal(y, np.rint(y)):
            return g
    raise AssertionError("operand is not a multiple of 2^-24")


def assert_exact_inputs(rowptr, col, val, B, extra=None, scale=1.0):
    """The precondition of the exact leg, on the test's own inputs: every product val*B is a multiple of 2^-g (g <= 6 for
    the operands of the issue: 2^-6 value products, integer features), every row holds fewer than 32768 entries and
    max_ij (|A|.|B|)_ij * 2^g < 2^24 — so every partial sum, in any order and any grouping, is an fp32 number.
    extra [k]: a bias added to every row (joins the magnitude); scale: a power of two the result is multiplied with.
    -> (the left side, the longest row)"""
    g = _granule_log2(val) + _granule_log2(B)
    if extra is not None:
        g = max(g, _granule_log2(extra))
    mag = oracle_spmm(rowptr, col, np.abs(val), np.abs(B)).astype(np.float64)
    if extra is not None:
        mag = mag + np.abs(np.asarray(extra, np.float64))[None, :]
    lhs = float(mag.max()) * scale * 2.0 ** g if mag.size else 0.0
    longest = int(np.diff(rowptr).max()) if len(rowptr) > 1 else 0
    assert longest < 32768, longest
    assert lhs < 2.0 ** 24, (lhs, g)
    return lhs, longest


def assert_exact(C, Cref, what=""):
    """value equality on every element (values, not bits: the sign of a zero may differ)"""
    C = np.asarray(C)
    Cref = np.asarray(Cref)
    assert C.shape == Cref.shape, (C.shape, Cref.shape, what)
    if not np.array_equal(C, Cref):
        bad = np.argwhere(C != Cref)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {C.size} elements differ, first at {i}: got {C[i]!r}, want {Cref[i]!r}")


U24 = 2.0 ** -24
BOUND_SLACK = 16      # 8u value-factor check + u_col*b + u_row scaling + bias add + the oracle's own rounding = 12, rounded up


def elementwise_bound(rowptr, mag, slack=BOUND_SLACK):
    """1.01 * (L_i + slack) * 2^-24 * mag_ij + 1e-37, L_i the stored length of row i (duplicates included)"""
    L = np.diff(rowptr).astype(np.float64)[:, None]
    return 1.01 * (L + slack) * U24 * np.asarray(mag, np.float64) + 1e-37


def elementwise_ratio(C, Cref, mag, rowptr, slack=BOUND_SLACK):
    """max_ij |C - C*|_ij / bound_ij (<= 1: inside the bound) and where it is reached"""
    err = np.abs(np.asarray(C, np.float64) - np.asarray(Cref, np.float64))
    ratio = err / elementwise_bound(rowptr, mag, slack)
    if ratio.size == 0:
        return 0.0, (0, 0)
    at = np.unravel_index(int(np.nanargmax(ratio)), ratio.shape)
    assert np.all(np.isfinite(np.asarray(C))), "non-finite result"
    return float(ratio[at]), tuple(int(x) for x in at)


def assert_elementwise(C, Cref, mag, rowptr, what="", slack=BOUND_SLACK):
    ratio, at = elementwise_ratio(C, Cref, mag, rowptr, slack)
    print(f"elementwise bound ratio {what}: {ratio:.4f} at {at}")
    assert ratio <= 1.0, f"{what}: |C - C*| is {ratio:.3f} x the bound at {at} (row length {int(np.diff(rowptr)[at[0]])})"
    return ratio


def spmm_references(rowptr, col, val, B, bias=None, relu=False):
    """(C*, mag) of act(A.B + bias): the fp64 oracle and oracle(|A|, |B|) (+ |bias|: the bias is one more term of every
    row, [A 1].[B; bias], and its addition rounds relative to a sum that holds it)"""
    Cref = oracle_spmm(rowptr, col, val, B).astype(np.float64)
    mag = oracle_spmm(rowptr, col, np.abs(val), np.abs(B)).astype(np.float64)
    if bias is not None:
        Cref = Cref + np.asarray(bias, np.float64)[None, :]
        mag = mag + np.abs(np.asarray(bias, np.float64))[None, :]
    if relu:
        Cref = np.maximum(Cref, 0.0)
    return Cref, mag


_EXACT_PATTERNS = {}
HUB_MIN = 1000                                         # every pattern below holds a row at least this long, and empty rows


def exact_pattern(name):
    """the sparsity patterns of the exact / element-wise tests -> (rowptr, col, m, n); each has empty rows and one hub row
    (the *_diag ones keep a stored diagonal in every row, single-entry rows in place of the empty ones: what the
    detection of u[r]*u[c] values needs)"""
    if name in _EXACT_PATTERNS:
        return _EXACT_PATTERNS[name]
    dup = lambda rp, ci, seed: with_duplicates(rp, ci, np.zeros(len(ci), np.float32), seed=seed)[:2]
    if name == "unsliced":                               # every unsliced family: 10 % empty rows, a 2000-entry row, duplicates
        m, n = 2500, 3000
        rp, ci, _ = random_csr(m, n, 50000, seed=41, empty_rows=0.1, long_rows=[(3, 2000)])
        rp, ci = dup(rp, ci, 42)
    elif name in ("group", "group_dup", "group_diag", "group_diag_dup"):   # the 15-bit slice-major stream (slices=3)
        m = n = 6000
        rp, ci, _ = sym_norm_graph(n, 260000, seed=3)
        rp, ci = reshape_rows(rp, ci, n, seed=43, hub=(4321, 2000), keep_diagonal="diag" in name)
        if name.endswith("_dup"):
            rp, ci = dup(rp, ci, 44)
    elif name == "vcsr":                                 # slices wider than the 15-bit stream: the virtual CSR, with values
        m, n = 3000, 140000
        rp, ci, _ = random_csr(m, n, 400000, seed=7, empty_rows=0.05, long_rows=[(11, 8000)])
        rp, ci = dup(rp, ci, 8)
    elif name == "col16":                                # ... value-free on the 16-bit column stream: >= 48 entries per column
        m, n = 20000, 70000
        lens = np.random.default_rng(45).poisson(180, m)
        lens[np.random.default_rng(46).random(m) < 0.03] = 0
        lens[[1, m - 1]] = 0
        lens[777] = 5000
        rp, ci = random_rows_csr(m, n, lens, seed=47)
    elif name == "lds":
        m = n = 3001
        rp, ci, _ = banded_csr(n, 150, 3, seed=5, hub=(777, 2600))
        rp, ci = reshape_rows(rp, ci, n, seed=48, spare=(777,))
        rp, ci = dup(rp, ci, 6)
    elif name == "lds_all":                              # every entry inside its panel's 128 x 512 window: nothing is left for
        m = n = 2000                                     # the accumulate pass.  No hub row (exempt from HUB_MIN): 1000 distinct
        rp, ci, _ = banded_csr(n, 100, 0, seed=3)        # columns cannot lie inside a 512-column window; empty rows it has
        rp, ci = reshape_rows(rp, ci, n, seed=52)
        rp, ci = dup(rp, ci, 9)
    elif name == "mfma":
        m = n = 2500
        rp, ci, _ = dense_band_csr(n, 200, 0.6, seed=4, sparse_from=1700)
        rp, ci = reshape_rows(rp, ci, n, seed=49, hub=(2100, 1500))
        rp, ci = dup(rp, ci, 7)
    elif name == "dropin_csr":                           # csr2tile's plain-CSR packing
        m = n = 3000
        rp, ci, _ = sym_norm_graph(n, 40000, seed=4)
        rp, ci = reshape_rows(rp, ci, n, seed=50, hub=(1234, 2000))
        rp, ci = dup(rp, ci, 1)
    elif name in ("dropin_group", "dropin_group_diag"):  # ... and its group packing (mean degree >= 128, table > one L2)
        m = n = 17000
        rp, ci, _ = sym_norm_graph(n, 1200000, seed=12)
        rp, ci = reshape_rows(rp, ci, n, seed=51, empty=0.02, hub=(9999, 3000), keep_diagonal=name.endswith("_diag"))
        rp, ci = dup(rp, ci, 2)
    elif name == "auto_diag":                            # the smallest square matrix on which the automatic rules act: n * 128 B
        m = n = 32769                                    # is just above one L2 (4 slices, narrow set of 2: tests/stress_plan.py),
        lens = np.random.default_rng(53).poisson(140, m)  # mean degree >= 128, a stored diagonal in every row
        lens[np.random.default_rng(54).random(m) < 0.02] = 0
        lens[[1, m - 1]] = 0
        lens[12345] = 3000
        rp, ci = random_rows_csr(m, n, lens, seed=55)
        rows = np.concatenate([np.repeat(np.arange(m), np.diff(rp)), np.arange(m)])
        cols = np.concatenate([ci.astype(np.int64), np.arange(m)])
        order = np.lexsort((cols, rows))
        rp = np.zeros(m + 1, np.int64)
        rp[1:] = np.cumsum(np.bincount(rows, minlength=m))
        rp, ci = rp.astype(np.int32), cols[order].astype(np.int32)
    else:
        raise KeyError(name)
    lens = np.diff(rp)
    assert (lens.max() >= HUB_MIN or name == "lds_all") and lens.max() < 32768, name
    assert (lens <= (1 if "diag" in name else 0)).sum() >= 2, name
    _EXACT_PATTERNS[name] = (rp, ci, m, n)
    return _EXACT_PATTERNS[name]


def exact_operands(pattern, kind, seed=0):
    """values for a pattern -> dict(rp, ci, va, m, n, u_row, u_col).  kind: "int" (non-zero integers in [-4, 4]: no
    factors), "pow2" (u[r]*u[c], u = 2^-e; one u when square), "pow2_row" (row-constant 2^-e_r), "wide" (N(0, 0.5) * 2^s_r),
    "wide_factored" ((0.5 + rand) * 2^a per row and per column)"""
    rp, ci, m, n = exact_pattern(pattern)
    u_row = u_col = None
    if kind == "int":
        va = int_values(len(ci), seed + 100)
    elif kind == "wide":
        va = wide_values(rp, seed + 101)
    elif kind == "pow2_row":
        u_row, u_col = pow2_factors(m, seed + 102), np.ones(n, np.float32)
        va = factored_values(rp, ci, u_row, u_col)
    else:
        gen = pow2_factors if kind == "pow2" else wide_factors
        u_col = gen(n, seed + 103)
        u_row = u_col if m == n and kind == "pow2" else gen(m, seed + 104)
        va = factored_values(rp, ci, u_row, u_col)
    return dict(rp=rp, ci=ci, va=va, m=m, n=n, u_row=u_row, u_col=u_col)


# (pattern, kind, widths) of every case test_exact_gpu.py runs: test_exact_cpu.py checks each generator without a GPU
EXACT_CASES = [("unsliced", "int", (4, 8, 15, 16, 36, 100, 128, 256)),
               ("group", "int", (16, 32, 40, 41, 64, 100, 128)), ("group_dup", "int", (16, 32, 40, 41, 64, 100, 128)),
               ("group", "pow2", (16, 32, 40, 41, 64, 100, 128, 136)), ("group_dup", "pow2", (16, 32, 40, 41, 64, 100, 128)),
               ("group_diag", "pow2", (16, 41, 128)), ("group", "pow2_row", (16, 41, 128)),
               ("vcsr", "int", (64,)), ("col16", "pow2", (64,)), ("lds", "int", (64, 100)), ("mfma", "int", (36, 64, 128)),
               ("dropin_csr", "int", (16, 41, 128)), ("dropin_group", "int", (16, 41, 128)),
               ("dropin_group_diag", "pow2", (16, 41, 128))]
WIDE_CASES = [("unsliced", "wide", (4, 8, 15, 16, 36, 100, 128, 256)),
              ("group", "wide", (16, 41, 128)), ("group_dup", "wide_factored", (16, 41, 128)),
              ("vcsr", "wide", (64,)), ("col16", "wide_factored", (64,)), ("lds", "wide", (64, 100)), ("mfma", "wide", (36, 128))]


# ---- the fused epilogue C = dropout(act(A.B + bias)) in exact arithmetic (test_exact_cpu.py, test_exact_gpu.py) ----
EPILOGUES = [dict(bias=True), dict(relu=True), dict(bias=True, relu=True), dict(bias=True, relu=True, dropout=True), dict(dropout=True)]
EPILOGUE_DROPOUT = (0.5, 0x1234567, 11)                # p (scale 1 / (1 - p) = 2 exactly), seed, offset (no multiple of 4)


def epilogue_reference(Cref64, bias, relu, keep, scale, u_row=None):
    """dropout(act(C* + bias)) in fp64, in the order of include/gcn_spmm.h: [row factor,] bias, ReLU, mask, scale.
    bias [k] or None; keep [m x k] bool (util.dropout_keep, the independent Philox twin) or None: no dropout; kept
    elements are multiplied by `scale`.  u_row [m]: Cref64 holds the sums BEFORE the row factor (what a value-free
    kernel accumulates from u_col * B); the factor goes on first, the bias after it."""
    Z = np.asarray(Cref64, np.float64)
    if u_row is not None:
        Z = Z * np.asarray(u_row, np.float64)[:, None]
    if bias is not None:
        Z = Z + np.asarray(bias, np.float64)[None, :]
    if relu:
        Z = np.maximum(Z, 0.0)
    if keep is not None:
        Z = np.where(keep, scale * Z, 0.0)
    return Z


def epilogue_inputs(m, n, k):
    """the operands of one exact epilogue case beside the matrix -> (B [n x k] integers in [-8, 8], bias [k] integers in
    [-8, 8], keep [m x k] at p = 0.5): the same on the CPU, where their discrimination is proven, and on the GPU"""
    p, seed, offset = EPILOGUE_DROPOUT
    B = int_features(n, k, seed=3000 + k)
    bias = np.random.default_rng(k).integers(-8, 9, k).astype(np.float32)
    keep = dropout_keep(m * k, p, seed, offset).reshape(m, k)
    return B, bias, keep


# (pattern, kind, widths) of every case of test_exact_gpu.py::test_exact_epilogue; the 9-slice plan runs
# EPILOGUE_NINE_SLICES[pattern] of them again
EXACT_EPILOGUE_CASES = [("unsliced", "int", (4, 8, 15, 16, 36, 41, 64, 100, 128, 256)),
                        ("group_dup", "pow2", (16, 21, 32, 40, 41, 64, 128, 136, 260)),
                        ("group_dup", "int", (16, 32, 40, 41, 64, 128, 136, 260)),
                        ("vcsr", "int", (64,)), ("col16", "pow2", (64,)), ("lds", "int", (64, 100)),
                        ("mfma", "int", (36, 64, 128)), ("lds_all", "int", (64, 100))]
EPILOGUE_NINE_SLICES = {"group_dup": (16, 64, 128)}
