"""Host-side op surface for the aggregation SpMM  C = Â · B  on MI355X.

Mirrors the two interfaces the reference reaches its SpMM through:

* B2 — ``torch.spmm(adj, dense)`` / ``torch.sparse.mm(adj, dense)`` with a
  ``torch.sparse_coo`` fp32 ``adj`` (pygcn/gcn1.py:53, gcn2.py:92,147, gcn3.py:87,146,
  gcn4.py:56,106, gcn5.py:90,135).  ``install()`` routes exactly that case (GPU
  sparse fp32 × GPU dense fp32) to the HIP kernel and leaves everything else to
  stock PyTorch, so gcn1–5 run unchanged.
* B1 — the ``flexspmm`` autograd Function of pygcn/gcn6.py:34-62 (see dropin.py).

Learnable edge weights: ``CsrAdjacency(..., mutable_values=True)`` and ``spmm(adj, dense, values=w)``; the gradient
of the values is an SDDMM on the adjacency's pattern (``CsrAdjacency.sddmm``), and ``install(sparse_grad=True)`` routes
``torch.sparse.mm`` for a grad-requiring COO operand through it.

PyTorch is plumbing here (device memory, streams, autograd); the arithmetic is
libgcnspmm.so.  There is no CPU fallback: CPU tensors raise.
"""
import ctypes
import weakref

import torch

from . import _lib
from ._lib import _ptr, _stream_ptr, call  # noqa: F401  (the two pointer helpers: tools import them from here)


class Scratch:
    """Device scratch by kind: one uint8 buffer per kind, allocated at the first call that needs it (so before a capture),
    replaced only when a call needs more bytes or another device, never shrunk.  A replaced buffer goes onto ``retired``
    and stays allocated: a captured step recorded its address and goes on writing its flag and partials there at every
    replay.  Kinds are separate buffers, so two units of one owner may run on two streams."""

    def __init__(self):
        self.buffers, self.retired = {}, []

    def get(self, kind, nbytes, device):
        ws = self.buffers.get(kind)
        if ws is None or ws.numel() < nbytes or ws.device != device:
            if ws is not None:
                self.retired.append(ws)
            ws = self.buffers[kind] = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return ws


class CsrAdjacency:
    """Device-resident CSR matrix (int32 rowptr / int32 col / fp32 val) + its cached
    SpMM plan.  The layout is the reference's own CSR hand-off (gcn6.py:302-311:
    ``to_sparse_csr()``, crow/col cast to int32).

    mutable_values=True: the values will change and the pattern will not (learned edge weights).  The plan keeps what
    ``update_values`` needs to re-lay new values in place; it has no value factors and no panels (``panels`` is
    ignored)."""

    def __init__(self, rowptr, col, val, shape, symmetric=None, chunk_nnz=0, slices="auto", panels=0,
                 mutable_values=False):
        if not (rowptr.is_cuda and col.is_cuda and val.is_cuda):
            raise _lib.GcnAmdError("CsrAdjacency needs CUDA/HIP tensors (no CPU path in gcn_amd)")
        self.rowptr = rowptr.to(torch.int32).contiguous()
        self.col = col.to(torch.int32).contiguous()
        # (a mutable adjacency owns its values: update_values writes them, and they must never be the caller's tensor)
        self.val = val.to(torch.float32).contiguous() if not mutable_values else val.detach().to(torch.float32, copy=True)
        self.m, self.n = int(shape[0]), int(shape[1])
        self.nnz = int(self.col.numel())
        if self.rowptr.numel() != self.m + 1:
            raise ValueError("rowptr must have m+1 entries")
        if self.nnz >= 2 ** 31:
            raise ValueError("nnz must fit int32 (row-partition the matrix first)")
        self.symmetric = symmetric
        self.chunk_nnz = int(chunk_nnz)
        self.slices = -1 if slices == "auto" else int(slices)    # XCD-aware column slicing
        # LDS-staged row panels: off unless asked for ("auto" = by measured window coverage) — on MI355X
        # the chunk kernel is still faster even on community-ordered graphs
        self.panels = -1 if panels == "auto" else int(bool(panels))
        self.mutable_values = bool(mutable_values)
        if self.mutable_values:
            self.panels = 0
        self._plan = None
        self._transpose = None
        self._tstale = False         # the mutable transpose needs a refresh: update_values has changed self.val since
        self._tpattern = None        # tpattern(): the one copy every backward walk and the mutable transpose read
        self._scratch = Scratch()    # the workspaces of the plan-free units, by kind: edge, gatv2, aggregate, sample
        self.values_version = 0      # counts update_values calls: a backward that reads the values checks it has not moved
        self.device = self.val.device

    # -- constructors ---------------------------------------------------------
    @classmethod
    def from_scipy(cls, mat, device="cuda", symmetric=None, chunk_nnz=0):
        mat = mat.tocsr()
        mat.sort_indices()
        dev = torch.device(device)
        return cls(torch.from_numpy(mat.indptr.astype("int32")).to(dev),
                   torch.from_numpy(mat.indices.astype("int32")).to(dev),
                   torch.from_numpy(mat.data.astype("float32")).to(dev),
                   mat.shape, symmetric=symmetric, chunk_nnz=chunk_nnz)

    @classmethod
    def from_torch_sparse(cls, adj, symmetric=None, chunk_nnz=0):
        """From a torch sparse COO/CSR tensor (the object pygcn builds in
        utils.py:243-250).  COO is coalesced and converted once."""
        if adj.layout == torch.sparse_coo:
            adj = adj.coalesce().to_sparse_csr()
        elif adj.layout != torch.sparse_csr:
            raise TypeError(f"unsupported layout {adj.layout}")
        return cls(adj.crow_indices(), adj.col_indices(), adj.values(), adj.shape,
                   symmetric=symmetric, chunk_nnz=chunk_nnz)

    # -- plan -------------------------------------------------------------------
    @property
    def plan(self):
        if self._plan is None:
            handle = ctypes.c_void_p()
            call("gcn_spmm_plan_create", ctypes.byref(handle), self.rowptr, self.m, self.n, self.nnz, self.chunk_nnz,
                 device=self.device)
            self._plan = handle
            weakref.finalize(self, _destroy_plan, handle)
            if self.mutable_values:                  # (before the slicing: it is built once, as a weighted plan)
                call("gcn_spmm_plan_set_values_mutable", handle, self.rowptr, self.col, self.val, device=self.device)
            if self.panels != 0:
                self.enable_panels(self.panels)
            if self.slices not in (0, 1) and self.panel_rows == 0:
                self.enable_slicing(self.slices)
        return self._plan

    @property
    def num_chunks(self):
        return int(_lib.load().gcn_spmm_plan_num_chunks(self.plan))

    @property
    def chunk_size(self):
        return int(_lib.load().gcn_spmm_plan_chunk_nnz(self.plan))

    def set_tile_cols(self, cols):
        """Feature-column tile per kernel pass (0 auto, 64, 128, 256)."""
        call("gcn_spmm_plan_set_tile_cols", self.plan, int(cols))

    def set_gather_width(self, nz_per_gather):
        """Non-zeros per gather instruction of the 64-column kernel: 0 auto, 1 or 4."""
        call("gcn_spmm_plan_set_gather_width", self.plan, int(nz_per_gather))

    def set_blocks_per_cu(self, blocks):
        """Main-kernel grid in blocks of 4 waves per CU (1..64, default 32 = oversubscribed); below the
        resident count (8, or 4 for the four-per-gather kernel) it leaves room for a concurrent kernel."""
        call("gcn_spmm_plan_set_blocks_per_cu", self.plan, int(blocks))

    def prepare_width(self, k):
        """Build now whatever a k-wide call would build at first use (gcn_spmm_plan_prepare_width): e.g. before a capture."""
        call("gcn_spmm_plan_prepare_width", self.plan, self.rowptr, self.col, self.val, int(k), device=self.device)

    def enable_panels(self, mode):
        """LDS-staged row panels (gcn_spmm_plan_enable_panels): 0 off, 1 on, -1 automatic."""
        call("gcn_spmm_plan_enable_panels", self.plan, self.rowptr, self.col, self.val, int(mode), device=self.device)

    @property
    def panel_rows(self):
        return int(_lib.load().gcn_spmm_plan_panel_rows(self.plan))

    @property
    def dense_panels(self):
        """panels of the plan that run as dense tiles on the matrix cores (gcn_spmm_plan_dense_panels)"""
        return int(_lib.load().gcn_spmm_plan_dense_panels(self.plan))

    @property
    def panel_coverage(self):
        return float(_lib.load().gcn_spmm_plan_panel_coverage(self.plan))

    def enable_slicing(self, slices):
        """XCD-aware column slicing (gcn_spmm_plan_enable_slicing): 0/1 off, -1 automatic."""
        call("gcn_spmm_plan_enable_slicing", self.plan, self.rowptr, self.col, self.val, int(slices), device=self.device)

    def set_value_factors(self, u_row, u_col):
        """Declare val[r, c] == u_row[r] * u_col[c] (checked on the device; GcnAmdError if an entry does not
        factor): lets the sliced main pass run without its value stream.  Square normalised adjacencies
        are detected automatically; this is for row blocks / renumbered columns.  (None, None) forgets."""
        if u_row is None and u_col is None:
            return call("gcn_spmm_plan_set_value_factors", self.plan, None, None, None, None, None, device=self.device)
        ur = u_row.to(device=self.device, dtype=torch.float32).contiguous()
        uc = u_col.to(device=self.device, dtype=torch.float32).contiguous()
        if ur.numel() != self.m or uc.numel() != self.n:
            raise ValueError("u_row needs m entries and u_col n entries")
        call("gcn_spmm_plan_set_value_factors", self.plan, self.rowptr, self.col, self.val, ur, uc, device=self.device)

    @property
    def has_value_factors(self):
        return bool(_lib.load().gcn_spmm_plan_has_value_factors(self.plan))

    @property
    def num_slices(self):
        return int(_lib.load().gcn_spmm_plan_num_slices(self.plan))

    def narrow_slices_for(self, k):
        """slices of the slice set a k-wide call runs on when that is not the plan's own (k <= 32, 33..48: built at the first
        such call of a value-free, auto-sliced plan); 0: the plan's own"""
        return int(_lib.load().gcn_spmm_plan_narrow_slices(self.plan, int(k)))

    @property
    def narrow_slices(self):
        return self.narrow_slices_for(16)

    def num_passes(self, k):
        """main-kernel launches (column passes) one k-wide SpMM issues"""
        return int(_lib.load().gcn_spmm_plan_num_passes(self.plan, int(k)))

    def prelaid_layout(self, k):
        """The slice-by-slice, column-scaled feature layout B' a k-wide SpMM of this plan gathers from
        (gcn_spmm_plan_prelaid_layout) → dict(slices, slice_cols, table_rows, ld), or None when this plan does not take
        the value-free sliced pass for that width (then matmul_raw is the only form)."""
        S, w, ld = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        rows = ctypes.c_int64(0)
        vp = lambda x: ctypes.cast(ctypes.byref(x), ctypes.c_void_p)
        try:
            call("gcn_spmm_plan_prelaid_layout", self.plan, int(k), vp(S), vp(w), vp(rows), vp(ld))
        except _lib.GcnAmdError:
            return None
        return dict(slices=S.value, slice_cols=w.value, table_rows=rows.value, ld=ld.value)

    def to_prelaid(self, dense, u_col):
        """B' for `dense` [n x k] (torch arithmetic; the first layer of a chain — later layers get theirs from
        matmul_prelaid): rows scaled by u_col, slice s at rows [s*(w+1), (s+1)*(w+1)), row w of every slice zero."""
        lay = self.prelaid_layout(int(dense.shape[1]))
        if lay is None:
            raise _lib.GcnAmdError("this plan has no pre-laid feature layout for that width")
        w, k = lay["slice_cols"], int(dense.shape[1])
        out = torch.zeros((lay["table_rows"], lay["ld"]), dtype=torch.float32, device=dense.device)
        c = torch.arange(self.n, device=dense.device)
        out[c + c // w, :k] = dense * u_col.to(dense.device)[:, None]
        return out

    def matmul_prelaid(self, Bp, out, out_scale=None, out_gap=0):
        """out[r + r // out_gap] = out_scale[r] * (Â·B)[r] with B handed over as B' (prelaid_layout): no per-call copy
        of the features, and the result lands in the B' layout of a consumer whose slices hold `out_gap` of these rows
        each (out_gap = 0: a plain [m x k] result).  gcn_spmm_csr_f32_prelaid."""
        lay = self.prelaid_layout(int(out.shape[1]))
        if lay is None or not (Bp.is_cuda and Bp.dtype == torch.float32 and Bp.is_contiguous()
                               and tuple(Bp.shape) == (lay["table_rows"], lay["ld"])):
            raise _lib.GcnAmdError("matmul_prelaid: B' must be the contiguous fp32 [table_rows x ld] array of prelaid_layout(k)")
        k = int(out.shape[1])
        need = self.m + (self.m - 1) // out_gap if (out_gap and self.m) else self.m
        if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape[0] >= need):
            raise ValueError("out must be a contiguous fp32 array with room for every (gapped) row")
        if out_scale is not None and not (out_scale.is_cuda and out_scale.dtype == torch.float32 and out_scale.is_contiguous()
                                          and out_scale.numel() == self.m):
            raise ValueError("out_scale must be a contiguous fp32 device vector with m entries")
        call("gcn_spmm_csr_f32_prelaid", self.plan, self.rowptr, self.col, self.val, Bp, out, out_scale, int(out_gap), k,
             device=self.device)
        return out

    def autotune(self, k=128, reps=3, verbose=False):
        """Measure, don't guess: time a k-wide SpMM on this matrix in the plan shapes that can win and keep the fastest —
        column slices {automatic, 8, none} and, unsliced and for k > 64, the column tile per pass {automatic, 64, 128}.
        The automatic rules (auto_slices, auto_tile_cols) are derived from unordered graphs; a matrix whose rows were
        renumbered to sit near their neighbours (Rabbit on a graph with communities) can be faster unsliced,
        and when its table is far larger than the caches, in NARROW tiles: a community's slice of a 64-column tile fits an
        L2 where its 256-column rows do not (products-sized planted partition, Rabbit order, k = 256: 15.8 ms with the
        widest tile, 13.0 ms with 64-column tiles; un-renumbered: 20.1 ms, profiles/r04r_*).
        → dict {(slices, tile_cols): ms} sorted by time; the first entry is what stays configured."""
        k = int(k)
        B = torch.randn((self.n, k), dtype=torch.float32, device=self.device)
        out = torch.empty((self.m, k), dtype=torch.float32, device=self.device)
        tried = {}
        shapes = [(-1, 0), (8, 0), (0, 0)] + ([(0, 64)] if k > 64 else []) + ([(0, 128)] if k > 128 else [])
        for S, tile in shapes:
            try:
                self.enable_slicing(S)
                self.set_tile_cols(tile)
            except _lib.GcnAmdError:
                continue                                       # (unsorted rows, S*m too large, ...)
            key = (self.num_slices, tile)
            if key in tried:
                continue
            for _i in range(2):
                self.matmul_raw(B, out=out)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _i in range(reps):
                self.matmul_raw(B, out=out)
            e1.record()
            torch.cuda.synchronize(self.device)
            tried[key] = e0.elapsed_time(e1) / reps
            if verbose:
                print(f"autotune: slices={key[0]} tile={key[1]}: {tried[key]:.4f} ms")
        best = min(tried, key=tried.get)
        self.enable_slicing(best[0])
        self.set_tile_cols(best[1])
        self.slices, self.tile_cols = best
        return dict(sorted(tried.items(), key=lambda kv: kv[1]))

    def main_kernel(self, k, epilogue=False, dtype=torch.float32):
        """name of the main kernel a k-wide SpMM on this plan launches (as rocprofv3 prints it); dtype=torch.bfloat16:
        that of a bf16 call (the fp32 kernel of the fallback where the bf16 group kernel does not apply)"""
        if dtype not in (torch.float32, torch.bfloat16):
            raise _lib.GcnAmdError(f"no SpMM for {dtype} operands (fp32 and bf16 only)")
        fn = "gcn_spmm_plan_main_kernel_bf16" if dtype == torch.bfloat16 else "gcn_spmm_plan_main_kernel"
        buf = ctypes.create_string_buffer(128)
        call(fn, self.plan, int(k), int(bool(epilogue)), buf, 128)
        return buf.value.decode()

    def profile_begin(self, capacity):
        """Record HIP-event pairs around the main kernel of the next `capacity` launches."""
        call("gcn_spmm_profile_begin", self.plan, int(capacity))
        self._prof_cap = int(capacity)

    def profile_end(self):
        """→ list of per-launch main-kernel durations in ms (synchronises)."""
        buf = (ctypes.c_float * self._prof_cap)()
        cnt = ctypes.c_int32(0)
        call("gcn_spmm_profile_end", self.plan, ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(ctypes.byref(cnt), ctypes.c_void_p))
        return [float(buf[i]) for i in range(cnt.value)]

    @property
    def values_mutable(self):
        """the plan's own answer (gcn_spmm_plan_values_mutable)"""
        return bool(_lib.load().gcn_spmm_plan_values_mutable(self.plan))

    def _device_values(self, val, what):
        if not isinstance(val, torch.Tensor) or val.dim() != 1 or val.numel() != self.nnz:
            raise ValueError(f"{what}: values must be a 1-D tensor of nnz = {self.nnz} entries in CSR order")
        if not val.is_cuda:
            raise _lib.GcnAmdError(f"{what} needs a CUDA/HIP tensor (no CPU path in gcn_amd)")
        return val.detach().to(device=self.device, dtype=torch.float32).contiguous()

    def update_values(self, val):
        """New values (nnz entries, CSR order) for a mutable adjacency: re-laid into the plan in place
        (gcn_spmm_plan_update_values: no allocation, no synchronisation — legal inside a graph capture) and copied
        into self.val (the adjacency's own copy: `val` itself is only read).  The transpose, if one exists, is refreshed
        from them at its next use.  GcnAmdError on an adjacency not made mutable (nothing changes then).
        Increments ``values_version``: the backward of a plain ``spmm(adj, x)`` whose forward saw other values raises."""
        v = self._device_values(val, "update_values")
        call("gcn_spmm_plan_update_values", self.plan, v, device=self.device)
        if v.data_ptr() != self.val.data_ptr():
            self.val.copy_(v)
        self._tstale = self._transpose is not None
        self.values_version += 1
        return self

    def sddmm(self, A, B, out=None):
        """out[e] = A[row(e)] . B[col(e)] for every stored entry e, in CSR order (gcn_sddmm_csr_f32): A is [m x k],
        B is [n x k]; fp32 accumulation, fp32 result.  bf16 operands are widened to fp32 first (correct, not fast).
        The gradient of Â·B with respect to Â's values, for grad_out = A.  A sliced plan with fixed values allocates its
        map of the virtual rows at the first call with k >= 33: before a graph capture, call it once or prepare_width(k)."""
        for t, rows, name in ((A, self.m, "A"), (B, self.n, "B")):
            if not (isinstance(t, torch.Tensor) and t.is_cuda) or t.dtype not in (torch.float32, torch.bfloat16) or t.dim() != 2:
                raise _lib.GcnAmdError(f"sddmm: {name} must be a 2-D fp32 or bf16 CUDA/HIP tensor")
            if t.shape[0] != rows:
                raise ValueError(f"sddmm: {name} needs {rows} rows, has {tuple(t.shape)}")
        if A.shape[1] != B.shape[1]:
            raise ValueError(f"sddmm: A and B need the same width, have {A.shape[1]} and {B.shape[1]}")
        A = A.to(torch.float32).contiguous()
        B = B.to(torch.float32).contiguous()
        if out is None:
            out = torch.empty(self.nnz, dtype=torch.float32, device=self.device)
        elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == self.nnz):
            raise ValueError("sddmm: out must be a contiguous fp32 device tensor of nnz entries")
        call("gcn_sddmm_csr_f32", self.plan, self.rowptr, self.col, A, B, out, int(A.shape[1]), device=self.device)
        return out

    def sddmm_kernel(self, k):
        """name of the kernel a k-wide sddmm on this plan launches (gcn_spmm_plan_sddmm_kernel)"""
        buf = ctypes.create_string_buffer(128)
        call("gcn_spmm_plan_sddmm_kernel", self.plan, int(k), buf, 128)
        return buf.value.decode()

    def _refresh_transpose(self, values):
        """re-lay values (nnz, CSR order of this adjacency) into the mutable transpose: values[tperm]"""
        t = self._mutable_transpose()
        t.update_values(values.detach().index_select(0, self.tpattern()[2]))
        return t

    def tpattern(self):
        """(trowptr int32 [n+1], trow int32 [nnz], tperm int32 [nnz]) of the transposed pattern, contiguous, built once per
        adjacency on the device (construct.py) and kept: entry t of the transpose is entry tperm[t] of this adjacency, in
        row trow[t]; duplicates stay separate entries, in their CSR order.  The one copy the backward walks of aggregate,
        spmm_heads, sddmm_heads, gatv2_scores and gat_edge_softmax read, and the mutable transpose is built from."""
        if self._tpattern is None:
            from .construct import _transpose_arrays
            trp, trow, _, eid = _transpose_arrays(self, with_values=False)
            self._tpattern = (trp, trow, eid)
        return self._tpattern

    def _transposed_pattern(self):
        """(rowptr int32 [n+1], row of each entry int32 [nnz], perm int64 [nnz]) of the transposed pattern, built on the
        device (construct.py): entry t of the transpose is entry perm[t] of this adjacency; duplicates stay separate
        entries, in their CSR order (a stable bucketing by column of entries that are already in row order)."""
        from .construct import _transpose_arrays
        trp, trow, _, eid = _transpose_arrays(self, with_values=False)
        return trp, trow, eid.long()

    def _mutable_transpose(self):
        """Âᵀ of a mutable adjacency: itself mutable, never Â (a symmetric pattern does not make learned values
        symmetric); duplicates stay separate entries, so its values are exactly self.val[tperm] of tpattern(), whose
        first two arrays are its rowptr and col."""
        if self._transpose is None:
            trp, trow, tperm = self.tpattern()
            self._transpose = CsrAdjacency(trp, trow, self.val.index_select(0, tperm), (self.n, self.m),
                                           symmetric=False, chunk_nnz=self.chunk_nnz, mutable_values=True)
        return self._transpose

    def transpose(self):
        """Âᵀ as a CsrAdjacency (cached); Â itself when flagged symmetric — the
        reference's backward reuses Â because Â is symmetric (gcn6.py:50-62).  A mutable adjacency's transpose is
        a mutable adjacency of its own (refreshed from Â's values by the autograd of spmm(values=...))."""
        if self.mutable_values:
            if self._tstale:                         # (values changed since the transpose was last refreshed)
                self._tstale = False
                return self._refresh_transpose(self.val)
            return self._mutable_transpose()
        if self.symmetric:
            return self
        if self._transpose is None:
            from .construct import transpose_csr
            self._transpose = transpose_csr(self)[0]       # (repeated entries stay separate: the same matrix)
            self._transpose._transpose = self
        return self._transpose

    # -- the op ------------------------------------------------------------------
    def matmul_raw(self, dense, out=None, bias=None, relu=False, dropout=None):
        """C = dropout(act(Â·dense + bias)) with no autograd; dense is [n x k] fp32 or bf16 on the same device.
        dropout = (p, seed, offset): the mask of gcn_spmm_csr_f32_epilogue (element i kept iff its Philox word
        passes; kept values scaled by 1/(1-p)); `dropout_rows` applies the same mask to a gradient.
        bf16 `dense` (gcn_spmm_csr_bf16_epilogue): every sum in fp32; the result is bf16 unless `out` is an fp32 tensor."""
        if not dense.is_cuda or dense.dtype not in (torch.float32, torch.bfloat16) or dense.dim() != 2:
            raise _lib.GcnAmdError("dense operand must be a 2-D fp32 or bf16 CUDA/HIP tensor")
        if dense.shape[0] != self.n:
            raise ValueError(f"shape mismatch: A is {self.m}x{self.n}, B is {tuple(dense.shape)}")
        if dense.dtype == torch.bfloat16:
            return self._matmul_raw_bf16(dense.contiguous(), out, bias, relu, dropout)
        dense = dense.contiguous()
        k = int(dense.shape[1])
        if out is None:
            out = torch.empty((self.m, k), dtype=torch.float32, device=dense.device)
        elif not (out.is_contiguous() and out.shape == (self.m, k) and out.dtype == torch.float32):
            raise ValueError("out must be a contiguous fp32 [m x k] tensor")
        if bias is not None:
            bias = bias.contiguous()
        if dropout is not None and float(dropout[0]) > 0.0:
            call("gcn_spmm_csr_f32_epilogue", self.plan, self.rowptr, self.col, self.val, dense, out, bias, 1 if relu else 0,
                 float(dropout[0]), int(dropout[1]), int(dropout[2]), k, device=self.device)
        elif bias is None and not relu:
            call("gcn_spmm_csr_f32", self.plan, self.rowptr, self.col, self.val, dense, out, k, device=self.device)
        else:
            call("gcn_spmm_csr_f32_bias_relu", self.plan, self.rowptr, self.col, self.val, dense, out, bias, 1 if relu else 0, k,
                 device=self.device)
        return out

    def _matmul_raw_bf16(self, dense, out, bias, relu, dropout):
        k = int(dense.shape[1])
        if out is None:
            out = torch.empty((self.m, k), dtype=torch.bfloat16, device=dense.device)
        elif not (out.is_contiguous() and out.shape == (self.m, k) and out.dtype in (torch.float32, torch.bfloat16)):
            raise ValueError("out must be a contiguous fp32 or bf16 [m x k] tensor")
        if bias is not None:
            bias = bias.to(dtype=torch.float32).contiguous()       # (the epilogue runs in fp32)
        c_dtype = _lib.DTYPE_BF16 if out.dtype == torch.bfloat16 else _lib.DTYPE_F32
        p, seed, offset = (float(dropout[0]), int(dropout[1]), int(dropout[2])) if dropout is not None else (0.0, 0, 0)
        call("gcn_spmm_csr_bf16_epilogue", self.plan, self.rowptr, self.col, self.val, dense, out, c_dtype, bias, 1 if relu else 0,
             p if p > 0.0 else 0.0, seed, offset, k, device=self.device)
        return out


def _values_version(adj):
    """what a forward that reads adj's own values records: the version of a mutable adjacency's values, None for fixed ones"""
    return adj.values_version if adj.mutable_values else None


def _check_values_version(adj, seen, what):
    """host-side, no copy and no synchronisation (under a graph capture it runs at capture time, like the rest of a
    backward's host code): the backward would multiply by Âᵀ of values the forward never saw"""
    if seen is not None and adj.values_version != seen:
        raise RuntimeError(f"{what}: update_values changed the adjacency's values between this forward and its backward; "
                           "the gradient of the forward's values is gone (use spmm(adj, x, values=...), which keeps them)")


def _destroy_plan(handle):
    try:
        call("gcn_spmm_plan_destroy", handle)
    except Exception:  # interpreter shutdown
        pass


class _SpmmFunction(torch.autograd.Function):
    """Autograd wrapper: grad_dense = Âᵀ · grad_out (Â itself when symmetric, as in
    gcn6.py:50-62); no gradient w.r.t. the adjacency (the reference has none either)."""

    @staticmethod
    def forward(ctx, adj, dense):
        ctx.adj, ctx.values_version = adj, _values_version(adj)
        return adj.matmul_raw(dense)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[1]:                # (a constant operand, e.g. the input features: no Âᵀ·grad to compute)
            return None, None
        _check_values_version(ctx.adj, ctx.values_version, "spmm")
        return None, ctx.adj.transpose().matmul_raw(grad_out.contiguous())


class _SpmmValuesFunction(torch.autograd.Function):
    """C = Â(values) · dense with learnable values: the forward re-lays `values` into the plan, the backward gives
    grad_values = SDDMM(grad_out, dense) on Â's pattern and grad_dense = Âᵀ · grad_out, Âᵀ refreshed from the same values."""

    @staticmethod
    def forward(ctx, adj, dense, values):
        adj.update_values(values)
        ctx.adj = adj
        ctx.save_for_backward(dense, values)
        return adj.matmul_raw(dense)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        dense, values = ctx.saved_tensors
        adj = ctx.adj
        grad_out = grad_out.contiguous()
        gd = gv = None
        if ctx.needs_input_grad[2]:
            gv = adj.sddmm(grad_out, dense)
        if ctx.needs_input_grad[1]:
            # (from the values of THIS forward: adj may have been given others since)
            gd = adj._refresh_transpose(values).matmul_raw(grad_out)
        return None, gd, gv


def spmm(adj, dense, values=None):
    """C = adj @ dense on the HIP kernel.  `adj` is a CsrAdjacency or a torch sparse
    (COO/CSR) fp32 tensor on the GPU (converted and cached per tensor object).
    values: nnz fp32 values in adj's CSR order that replace adj's own (and may require grad): adj must have been made
    with mutable_values=True; they are re-laid into its plan at every call, so values changed in place between two
    calls (an optimizer step) are picked up.
    Without `values`, the backward multiplies by the adjacency's own Âᵀ: RuntimeError if update_values ran since the forward."""
    if not isinstance(adj, CsrAdjacency):
        adj = _cached_csr(adj)
    if values is None:
        return _SpmmFunction.apply(adj, dense)
    if not isinstance(values, torch.Tensor) or values.dim() != 1 or values.numel() != adj.nnz:
        raise ValueError(f"spmm: values must be a 1-D tensor of nnz = {adj.nnz} entries in CSR order")
    if not values.is_cuda:
        raise _lib.GcnAmdError("spmm: values must be a CUDA/HIP tensor (no CPU path in gcn_amd)")
    if values.dtype != torch.float32:
        raise _lib.GcnAmdError("spmm: values must be fp32")
    if not adj.mutable_values:
        raise _lib.GcnAmdError("spmm(values=...) needs an adjacency made with mutable_values=True")
    return _SpmmValuesFunction.apply(adj, dense, values)


# --- routing of torch.spmm / torch.sparse.mm (interface B2) -----------------------
_csr_cache = {}          # id(sparse tensor) -> (weakref, CsrAdjacency)
_orig = {}


def _cached_csr(adj):
    key = id(adj)
    hit = _csr_cache.get(key)
    if hit is not None and hit[0]() is adj:
        return hit[1]
    csr = CsrAdjacency.from_torch_sparse(adj)
    _csr_cache[key] = (weakref.ref(adj, lambda _r, k=key: _csr_cache.pop(k, None)), csr)
    return csr


def _routable(a, b):
    return (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)
            and a.layout in (torch.sparse_coo, torch.sparse_csr) and a.is_cuda
            and a.dtype == torch.float32 and a.dim() == 2
            and b.layout == torch.strided and b.is_cuda and b.dtype == torch.float32 and b.dim() == 2
            and not a.requires_grad)


# torch.sparse.mm with a grad-requiring COO operand (install(sparse_grad=True)): one mutable adjacency per pattern
_pattern_cache = []      # [(indices tensor, shape, CsrAdjacency)], most recent first
_route_sparse_grad = False
_PATTERN_CACHE_SIZE = 4  # (each entry holds a plan and its transpose's: keep few)


def _routable_grad(a, b):
    return (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)
            and a.layout == torch.sparse_coo and a.is_cuda and a.dtype == torch.float32 and a.dim() == 2
            and a.requires_grad and a.is_coalesced()
            and b.layout == torch.strided and b.is_cuda and b.dtype == torch.float32 and b.dim() == 2)


def _pattern_csr(a):
    """the mutable adjacency of a coalesced COO pattern (its indices are the CSR order): reused while the pattern is
    the same — the same index storage, or equal indices — whatever the values"""
    idx = a._indices()
    shape = tuple(a.shape)
    for i, (cidx, cshape, adj) in enumerate(_pattern_cache):
        if cshape == shape and cidx.device == idx.device and cidx.shape == idx.shape and (
                cidx.data_ptr() == idx.data_ptr() or torch.equal(cidx, idx)):
            if i:
                _pattern_cache.insert(0, _pattern_cache.pop(i))
            return adj
    m, n = shape
    rowptr = torch.zeros(m + 1, dtype=torch.int64, device=idx.device)
    rowptr[1:] = torch.cumsum(torch.bincount(idx[0], minlength=m), 0)
    adj = CsrAdjacency(rowptr.to(torch.int32), idx[1].to(torch.int32), a._values().detach(), shape, mutable_values=True)
    _pattern_cache.insert(0, (idx, shape, adj))
    del _pattern_cache[_PATTERN_CACHE_SIZE:]
    return adj


class _SparseMmGrad(torch.autograd.Function):
    """torch.sparse.mm(a, b) for a coalesced COO `a` that requires grad: the gradient of `a` is a sparse COO tensor on
    a's own pattern (an SDDMM), as stock PyTorch gives it"""

    @staticmethod
    def forward(ctx, a, b, adj):
        # a copy: the values of a sparse tensor share the storage of the tensor it was made from but not its version
        # counter, so autograd's check would miss an in-place change of that tensor between forward and backward
        vals = a._values().detach().clone()
        ctx.adj = adj
        ctx.a_indices, ctx.a_shape = a._indices(), a.shape
        ctx.save_for_backward(b, vals)
        adj.update_values(vals)
        return adj.matmul_raw(b)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        b, vals = ctx.saved_tensors
        adj = ctx.adj
        grad_out = grad_out.contiguous()
        ga = gb = None
        if ctx.needs_input_grad[0]:
            gv = adj.sddmm(grad_out, b)
            ga = torch.sparse_coo_tensor(ctx.a_indices, gv, ctx.a_shape, is_coalesced=True)
        if ctx.needs_input_grad[1]:
            gb = adj._refresh_transpose(vals).matmul_raw(grad_out)
        return ga, gb, None


def install(sparse_grad=False):
    """Route ``torch.spmm`` / ``torch.sparse.mm`` for (GPU sparse fp32) × (GPU dense fp32)
    to the HIP kernel; anything else goes to the original callables.
    sparse_grad=True: ``torch.sparse.mm`` also routes a coalesced GPU fp32 COO operand that requires grad (its gradient
    is the sparse COO tensor on its pattern stock PyTorch gives, computed by an SDDMM; one plan per pattern).
    ``torch.spmm``'s gradient of such an operand is a dense m×n tensor and stays with stock PyTorch, as do CSR operands."""
    global _route_sparse_grad
    _route_sparse_grad = bool(sparse_grad)
    if _orig:
        return
    _lib.load()  # fail loudly now, not at the first layer
    _orig["spmm"] = torch.spmm
    _orig["sparse_mm"] = torch.sparse.mm

    def routed_spmm(a, b, *args, **kw):
        if not args and not kw and _routable(a, b):
            return spmm(a, b)
        return _orig["spmm"](a, b, *args, **kw)

    def routed_sparse_mm(a, b, *args, **kw):
        if not args and not kw and _routable(a, b):
            return spmm(a, b)
        if not args and not kw and _route_sparse_grad and _routable_grad(a, b):
            return _SparseMmGrad.apply(a, b, _pattern_csr(a))
        return _orig["sparse_mm"](a, b, *args, **kw)

    torch.spmm = routed_spmm
    torch.sparse.mm = routed_sparse_mm


def uninstall():
    global _route_sparse_grad
    _route_sparse_grad = False
    _pattern_cache.clear()
    if not _orig:
        return
    torch.spmm = _orig.pop("spmm")
    torch.sparse.mm = _orig.pop("sparse_mm")


def gather_rows(src, idx, out=None):
    """out[r,:] = src[idx[r],:]  (permutate.cu:3-21 counterpart), fp32 on the GPU."""
    if not (src.is_cuda and idx.is_cuda) or src.dtype != torch.float32 or src.dim() != 2:
        raise _lib.GcnAmdError("gather_rows needs a 2-D fp32 CUDA/HIP tensor and a CUDA index")
    src = src.contiguous()
    idx = idx.to(torch.int32).contiguous()
    nrows, k = int(idx.numel()), int(src.shape[1])
    if out is None:
        out = torch.empty((nrows, k), dtype=torch.float32, device=src.device)
    call("gcn_gather_rows_f32", out, src, idx, nrows, k, device=src.device)
    return out


def dropout_rows(x, p, seed, offset, out=None):
    """out = x with the dropout mask of the fused epilogue (gcn_dropout_f32): element i of the contiguous fp32 tensor
    is kept (and scaled by 1/(1-p)) iff its Philox4x32-10 word passes — the same function of (seed, offset, i) the
    SpMM epilogue uses, so applying it to a gradient is the backward of that epilogue.  bf16 tensors: the same mask
    (gcn_dropout_bf16)."""
    if not x.is_cuda or x.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.GcnAmdError("dropout_rows needs an fp32 or bf16 CUDA/HIP tensor")
    x = x.contiguous()
    if out is None:
        out = torch.empty_like(x)
    fn = "gcn_dropout_bf16" if x.dtype == torch.bfloat16 else "gcn_dropout_f32"
    call(fn, out, x, int(x.numel()), float(p), int(seed), int(offset), device=x.device)
    return out
