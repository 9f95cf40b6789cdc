// long_chunks.h — what the chunked long-row kernels of edge_softmax.hip and aggregate.hip share: finding the at most two
// long rows that meet a chunk of consecutive entries.  The chunk loops, the partials and the finish kernels are each unit's
// own.  Device code only; the long-row threshold is the caller's (LONG_ROW, at least the chunk length).
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

}  // namespace gcn
