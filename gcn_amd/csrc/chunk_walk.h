// chunk_walk.h — what stands around the chunk loop of the four "equal-nnz chunk, partial slab, fix-up" kernels
// (spmm_chunk_kernel, spmm_quad_kernel, spmm_narrow_kernel, spmm_narrow16_dpp_kernel), written once and never asking
// which kernel calls it: the drop-in prologue, a wave's chunk range and the row cursor of a chunk.  The chunk loops
// themselves — the gathers, the cross-lane exchanges, the fast paths, the narrow kernels' step splitter and the
// reduce-and-store half of a flush — stay each kernel's own (DESIGN.md §4.29 says where the sharing stops and why).
//
// The first part (next_nonempty_row and the two row-cursor macros) is plain int arithmetic over a pointer-like row pointer
// and compiles on the host without HIP: tests/sanitize_chunk_walk.cpp drives it against a serial walk under ASan + UBSan.
#pragma once

#if defined(__HIPCC__)
#define GCN_WALK_FN __host__ __device__ __forceinline__
#else
#define GCN_WALK_FN inline
#endif

namespace gcn {

// The row walk has just stepped onto row r and found it empty (rowptr[r + 1] == pos): the first row i > r that holds an
// entry (rowptr[i + 1] > pos), or m.  Gallop, then bisect — wave-uniform scalar loads, O(log run) where the walk used to
// spend one dependent load and one store per empty row.  Reads rowptr[r + 2 .. m] only.
template <class RowPtr>
GCN_WALK_FN int next_nonempty_row(RowPtr rowptr, int r, int m, int pos) {
  int lo = r, hi = r + 1;                               // row lo is empty; is row hi?
  unsigned step = 1;
  while (hi < m && rowptr[hi + 1] == pos) {
    lo = hi;
    step <<= 1;
    hi = (step >= (unsigned)(m - hi)) ? m : hi + (int)step;
  }
  while (hi - lo > 1) {                                 // row lo empty, row hi not (or hi == m)
    const int mid = lo + ((hi - lo) >> 1);
    if (rowptr[mid + 1] == pos) lo = mid; else hi = mid;
  }
  return hi;
}

// The row cursor of one chunk [c*T, min((c+1)*T, nnz)), as TEXT: six scalars that live in the kernel's own scope under
// these names —
//   r           the row being summed                    row_end     rowptr[r + 1] (-1 past the last row: never reached)
//   row_end_nx  the row end after it, one row ahead     head        row r began in an earlier chunk
//   pos         the first entry not yet summed          last_flush  where the last row ended (pos == last_flush: empty row)
// — declared and opened by GCN_ROW_WALK_OPEN and stepped to the next row by GCN_ROW_WALK_NEXT; the chunk loops read and
// advance `pos` themselves.  They are macros because the rule for this header was the kernels' machine code: as functions
// (of a cursor struct, by value or binding the kernel's locals by reference; forced inline or not) the same statements
// gave every kernel but one other register copies and branches at its row ends.  Both are plain int
// arithmetic over a pointer-like row pointer and expand on the host as well.
#define GCN_ROW_WALK_OPEN(rowptr, chunk_row, c, T, m)                                            \
  int r = (chunk_row)[c];                                                                        \
  int row_end    = (rowptr)[r + 1];                                                              \
  int row_end_nx = (r + 1 < (m)) ? (rowptr)[r + 2] : -1;                                         \
  bool head = (rowptr)[r] < (c) * (T);                                                           \
  int pos = (c) * (T);                                                                           \
  int last_flush = (c) * (T)
// row r is finished at `pos`: on to the next row — and when that one is empty, over the whole run of empty rows (they are
// jumped, not walked).  The only text that indexes rowptr[r + 2], under r + 1 < m.
#define GCN_ROW_WALK_NEXT(rowptr, m)                                                             \
  {                                                                                              \
    head = false;                                                                                \
    last_flush = pos;                                                                            \
    ++r;                                                                                         \
    row_end = row_end_nx;                                                                        \
    if (row_end == pos) {                                                                        \
      r = gcn::next_nonempty_row(rowptr, r, m, pos);                                             \
      row_end = (r < (m)) ? (rowptr)[r + 1] : -1;                                                \
    }                                                                                            \
    row_end_nx = (r + 1 < (m)) ? (rowptr)[r + 2] : -1;                                           \
  }

#if defined(__HIPCC__)

// a wave-uniform value into an SGPR
__device__ __forceinline__ int sgpr(int v) { return __builtin_amdgcn_readfirstlane(v); }

// The value held by the lane that loaded non-zero (step UU, this lane's sub) of a transposed 64-entry block.
//   LPE = 16: lane s*16+u holds entry 4u+s   -> DPP row_newbcast:UU (lane UU of every 16-lane row)
//   LPE =  4: lane s*4+u  holds entry 16u+s  -> DPP quad_perm [UU,UU,UU,UU]
// (every lane has a source lane, so bound_ctrl is irrelevant)
template <int LPE, int UU>
__device__ __forceinline__ int quad_bcast(int v) {
  static_assert(LPE == 16 || LPE == 4, "layouts: 16 or 4 lanes per non-zero");
  if constexpr (LPE == 16) {
    return __builtin_amdgcn_mov_dpp(v, 0x150 + UU, 0xf, 0xf, true);
  } else {
    return __builtin_amdgcn_mov_dpp(v, UU | (UU << 2) | (UU << 4) | (UU << 6), 0xf, 0xf, true);
  }
}

// drop-in (flexspmm) mode: the host does not know nnz; it lives in rowptr[m] (nnz_dev), the chunk count follows from
// it, and the values follow the column indices in one buffer (api_dropin.cpp, csr2tile layout)
__device__ __forceinline__ int dropin_nchunks(int nnz, int T) { return (int)(((long long)nnz + T - 1) / T); }
template <class ValPtr>                                 // (the kernel's pointer as it is: const float* __restrict__)
__device__ __forceinline__ void dropin_shape(const int* nnz_dev, int T, int& nnz, int& nchunks, const int* col,
                                             ValPtr& val) {
  if (nnz_dev) {
    nnz = *nnz_dev;
    nchunks = dropin_nchunks(nnz, T);
    val = reinterpret_cast<const float*>(col) + nnz;
  }
}

// XCD-aware chunk ranges: blocks b and b+8 share an XCD (round-robin dispatch), so XCD x walks the contiguous chunk
// range [x*N/8, (x+1)*N/8) — neighbouring rows (which share neighbours after RCM/Gorder) meet in one 4 MiB L2 — with the
// chunks of the range strided over the XCD's waves (4 per block; wib = the wave's index in its block).  Placement only
// affects speed, never the result.
struct ChunkRange {
  int c_lo, c_hi, first, stride;
  __device__ __forceinline__ ChunkRange(int wib, int nchunks) {
    const int xcd = blockIdx.x & 7;
    c_lo   = (int)(((long long)nchunks * xcd) >> 3);
    c_hi   = (int)(((long long)nchunks * (xcd + 1)) >> 3);
    first  = c_lo + (blockIdx.x >> 3) * 4 + wib;
    stride = (gridDim.x >> 3) * 4;
  }
};

#endif  // __HIPCC__

}  // namespace gcn
