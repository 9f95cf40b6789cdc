// long_chunks.h — what the chunked long-row kernels of edge_softmax.hip, aggregate.hip and multihead.hip share: finding the
// at most two long rows that meet a chunk of consecutive entries, and the walk over the chunks that the wave-per-chunk
// kernels make (edge_softmax.hip's block-per-chunk kernels write the same loop out: through the helper one of them comes
// out with other registers and another occupancy).  The partials and what a kernel does with a segment are
// each unit's own (gather_rows.h: the engine of aggregate.hip and multihead.hip).  Also the other half of the dispatch by
// row length, the rows a wave takes whole (for_wave_rows).  Device code only; the chunk length and the long-row threshold
// are the caller's (CHUNK and LONG_ROW, at least the chunk length).
#pragma once
#include <hip/hip_runtime.h>

namespace gcn {

// the row holding entry e0 (0 <= e0 < nnz): the largest r < rows with rowptr[r] <= e0 — never an empty row.  64 probes a round.
__device__ __forceinline__ int find_row(const int* __restrict__ rowptr, int rows, int e0, int lane) {
  int lo = 0, hi = rows;                               // rowptr[lo] <= e0, and rowptr[hi] > e0 or hi == rows
  while (hi - lo > 1) {
    const int step = (hi - lo + 63) >> 6;
    const long long probe = (long long)lo + (long long)lane * step;
    const bool le = probe < hi && rowptr[probe] <= e0;
    const int cnt = __popcll(__ballot(le));            // (rowptr is monotone: the lanes that say yes are a prefix, lane 0 among them)
    lo += (cnt > 0 ? cnt - 1 : 0) * step;              // (cnt == 0 only with rowptr[0] > 0: a malformed matrix must not index backwards)
    hi = lo + step < hi ? lo + step : hi;
  }
  return lo;
}

// the part [sb, se) of long row r (entries [rb, re)) inside the chunk [e0, e1), whose first and last entries lie in rows rh
// and rt; slot 0: the row holds the chunk's first entry, slot 1: it starts later in the chunk.  A row longer than a chunk
// that meets the chunk holds its first or its last entry.
struct Segment { int r, rb, re, sb, se; };
template <int LONG_ROW>
__device__ __forceinline__ bool long_segment(const int* __restrict__ rowptr, int slot, int rh, int rt, int e0, int e1, Segment& s) {
  if (slot == 1 && rt == rh) return false;
  s.r = slot ? rt : rh;
  s.rb = rowptr[s.r];
  s.re = rowptr[s.r + 1];
  if (s.re - s.rb <= LONG_ROW) return false;
  s.sb = s.rb > e0 ? s.rb : e0;
  s.se = s.re < e1 ? s.re : e1;
  return true;
}

// the chunks first, first + stride, ... (< nchunks) of CHUNK consecutive entries, a chunk per wave: f(c, slot, segment) for
// the part of each long row inside chunk c (wave-uniform: whole waves call this, find_row votes).
template <int CHUNK, int LONG_ROW, class F>
__device__ __forceinline__ void for_long_segments(const int* __restrict__ rowptr, int rows, int nnz, int nchunks, int first,
                                                  int stride, int lane, F f) {
  for (int c = first; c < nchunks; c += stride) {
    const int e0 = c * CHUNK;
    const int e1 = (long long)e0 + CHUNK < nnz ? e0 + CHUNK : nnz;
    const int rh = find_row(rowptr, rows, e0, lane), rt = find_row(rowptr, rows, e1 - 1, lane);
    for (int slot = 0; slot < 2; ++slot) {
      Segment s;
      if (long_segment<LONG_ROW>(rowptr, slot, rh, rt, e0, e1, s)) f(c, slot, s);
    }
  }
}

// the short rows: the wave of a 256-thread block owns ROWS (<= 63) consecutive rows and takes them one after the other,
// f(r, b, n) for row r with the entries [b, b + n).  One load brings the ROWS + 1 row bounds (ROWS empty rows cost that
// load and whatever f stores for them); a row of more than LONG_ROW entries is left to the chunk kernels and the flag is
// raised.  f is wave-uniform: waves past the last row leave whole, so the shuffles here and in f see full waves.
template <int ROWS, int LONG_ROW, class F>
__device__ __forceinline__ void for_wave_rows(const int* __restrict__ rowptr, int rows, int lane, int* __restrict__ long_flag, F f) {
  const long long wave = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (wave * ROWS >= rows) return;
  const int r0 = (int)wave * ROWS;
  const int ri = r0 + lane < rows ? r0 + lane : rows;
  const int rp = rowptr[ri];                           // lanes 0..ROWS: the row bounds (later lanes repeat rowptr[rows])
  for (int q = 0; q < ROWS && r0 + q < rows; ++q) {
    const int b = __shfl(rp, q), e = __shfl(rp, q + 1);
    const int n = e - b;
    if (n > LONG_ROW) {
      if (lane == 0) *long_flag = 1;                   // (every writer writes the same word)
      continue;
    }
    f(r0 + q, b, n);
  }
}

}  // namespace gcn
