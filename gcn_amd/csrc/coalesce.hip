// coalesce.hip — merging the repeated (row, column) entries of a CSR matrix on the device, with what the GCN adjacency needs
// on top of the merge (dropping, filling or adding to the diagonal) and the two kernels of its normalisation (row sums in
// fp64, and D^-1/2 A D^-1/2 or D^-1 A on the stored entries).  Plan-free like subgraph.hip: the caller's arrays, at most
// one memset node and kernels, no allocation, no host read of device data, no global atomics — every output element has one
// writer, so a call gives the same bits every time and is compared with a host twin (tests/coalesce_ref.py).  Every access
// is a 4-byte one, except the 8-byte reads and writes of deg.  The contract is written out in include/gcn_spmm.h.
//
// ---- merge ---------------------------------------------------------------------------------------------------------------------
// A RUN is a maximal stretch of consecutive entries of one row with the same column, its first entry the HEAD: entry x is a
// head iff x is the row's first entry or col[x - 1] != col[x] (one more 4-byte read of a line the wave has just fetched; no
// exchange between lanes, waves or passes is needed to find heads).  On a column-sorted row a run is one distinct (row,
// column) pair.  The output holds one entry per head (none for a diagonal run under DROP), in entry order, plus an inserted
// diagonal under FILL / ADD when no entry of the row has col == r.
// Two calls, as for the induced subgraph: COUNT writes out_len[r], the caller scans, FILL writes the entries; both run the
// same code (CoalesceOp<FILL>::row).  A row's output positions are a running count of heads over the row.
//
// The unit is subgraph.hip's: ONE ROW PER WORKGROUP, one wave for a row of at most kSampleLongRow entries and four waves
// (256 threads) for a longer one.  Inside a wave the running count is a ballot and a popcount; the waves of a workgroup
// exchange their counts of a pass through ordered_slots (row_dispatch.h: one barrier per pass).  The row is read twice: once
// for its three counts (heads, entries on the diagonal, heads left of the diagonal) — which give the length, whether a
// diagonal is inserted and where — and, in the fill, once more to write (from the caches).
// seg needs no run walk: an entry that is not dropped belongs to the last head at or before it, i.e. to output entry
// (inclusive head count - 1), shifted by one behind an inserted diagonal.
// VALUES: THE HEAD'S LANE WALKS ITS RUN, left to right — the fold order of the contract — so a run costs its length in one
// lane.  Real inputs (an edge list with its mirror, repeated edges of a multigraph) have runs of 1-3 entries; a run of
// thousands is correct and slow (its lane reads the run entry by entry while the other lanes of the wave wait).
//
// Long rows: the dispatch (the wave kernel, the flag, the long kernel's screening of the rows) is row_dispatch.h's, shared
// with sample.hip and subgraph.hip; the merge, the degrees and the normalisation are three ops over it.
//
// ---- degrees and normalisation -------------------------------------------------------------------------------------------------
// The same decomposition, a wave per row and a 256-thread workgroup per row of more than kSampleLongRow entries, because
// both are per-row work with a row-constant operand (the row's sum; the row's scale) and no expanded row array exists to
// hang a lane per entry on.  These calls have no workspace, hence no flag: the long kernel always screens the row pointer
// (4 * m bytes, read once) unless nnz <= kSampleLongRow.  Degree: lane t adds entries t, t + THREADS, ... in fp64, the
// lanes of a wave are added by a xor butterfly (32, 16, ..., 1) and the waves in wave order — a fixed order, the same bits
// at every call.  Normalise: out[x] = (float)(s_r * v * s_c) or (float)(v * t_r) in fp64, a zero degree scales by zero.
#include <hip/hip_runtime.h>

#include "row_dispatch.h"
#include "spmm_kernels.h"

namespace gcn {
namespace {

struct RowRange { int b, e; };

// the row [b, e) of row i, or false when its row pointer is not usable
__device__ __forceinline__ bool row_range(const int* rowptr, int nnz, int i, RowRange& r) {
  r.b = rowptr[i];
  r.e = rowptr[i + 1];
  return r.b >= 0 && r.e >= r.b && r.e <= nnz;
}

// ---- merge ---------------------------------------------------------------------------------------------------------------------
struct CoalesceArgs {
  const int* rowptr;
  const int* col;
  const float* val;
  int* out_len;                                        // COUNT
  const int* out_rowptr;                               // FILL
  int* out_col;
  float* out_val;
  int* out_first;
  int* seg;
  int count, n, nnz, reduce, diagonal;                 // count: rows
  float diag_value;
};

enum : int { kValid = 1, kKept = 2, kHead = 4, kDiag = 8, kLow = 16 };     // what look() says about a thread's entry

template <bool FILL>
struct CoalesceOp : CoalesceArgs {
  using Row = RowRange;
  template <int THREADS>
  struct Scratch {
    int wsum[THREADS / 64][3];                         // the waves' counts of a whole row: heads, diagonal entries, heads left of it
    int cnt[2][THREADS / 64];                          // per pass parity and wave: heads (ordered_slots)
  };
  __device__ bool locate(int i, Row& r) const { return row_range(rowptr, nnz, i, r); }

  // the value of the run that starts at entry x (column c), folded left to right in fp32
  __device__ __forceinline__ float fold(long long x, int e, int c) const {
    float acc = val[x];
    if (reduce != kCoalesceFirst) {
      for (long long j = x + 1; j < e && col[j] == c; ++j) {
        const float v = val[j];
        if (reduce == kCoalesceSum) acc += v;
        else if (reduce == kCoalesceMax) acc = (v > acc || v != v) ? v : acc;
        else acc = (v < acc || v != v) ? v : acc;
      }
    }
    return acc;
  }

  // one row on a workgroup of THREADS threads (every thread of the workgroup calls it with the same arguments)
  template <int THREADS>
  __device__ __forceinline__ void row(int r, const Row& rr, Scratch<THREADS>& L) const {
    constexpr int WAVES = THREADS / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = rr.b, e = rr.e;
    const int passes = (int)(((long long)e - b + THREADS - 1) / THREADS);
    const bool has_diag = r < n;                       // (a row r >= n has no diagonal column)
    const bool dropping = diagonal == kDiagDrop && has_diag;
    const bool inserting = (diagonal == kDiagFill || diagonal == kDiagAdd) && has_diag;
    auto look = [&](int p, int& c) {                   // this thread's entry of pass p: its flags (0 past the row) and column
      const long long x = (long long)b + (long long)p * THREADS + tid;
      if (x >= e) return 0;
      c = col[x];
      const bool head = x == b || col[x - 1] != c;
      const bool diag = has_diag && c == r;
      const bool kept = !(dropping && diag);
      return kValid | (kept ? kKept : 0) | (head && kept ? kHead : 0) | (diag ? kDiag : 0) | (head && kept && c < r ? kLow : 0);
    };

    // ---- the row's counts (wave-uniform, then workgroup-uniform) ----------------------------------------------------------------
    int heads = 0, diags = 0, lows = 0;
    for (int p = 0; p < passes; ++p) {
      int c = 0;
      const int f = look(p, c);
      heads += __popcll(__ballot(f & kHead));
      diags += __popcll(__ballot(f & kDiag));
      lows += __popcll(__ballot(f & kLow));
    }
    if constexpr (WAVES > 1) {
      if (lane == 0) {
        L.wsum[wave][0] = heads;
        L.wsum[wave][1] = diags;
        L.wsum[wave][2] = lows;
      }
      __syncthreads();
      heads = diags = lows = 0;
      for (int w = 0; w < WAVES; ++w) {
        heads += L.wsum[w][0];
        diags += L.wsum[w][1];
        lows += L.wsum[w][2];
      }
    }
    const bool insert = inserting && diags == 0;       // the diagonal goes in at output position `lows`
    const int total = heads + (insert ? 1 : 0);
    if constexpr (!FILL) {
      if (tid == 0) out_len[r] = total;
      return;
    } else {
      const int o = out_rowptr[r];
      if (o < 0 || out_rowptr[r + 1] - o != total) return;              // (workgroup-uniform)
      if (insert && tid == 0) {
        out_col[o + lows] = r;
        if (out_val) out_val[o + lows] = diag_value;
        if (out_first) out_first[o + lows] = -1;
      }

      // ---- the heads, in entry order ---------------------------------------------------------------------------------------------
      const unsigned long long upto = lane == 63 ? ~0ull : (2ull << lane) - 1ull;      // this lane and the lanes below
      int run = 0;                                     // heads of the passes so far
      for (int p = 0; p < passes; ++p) {
        int c = 0;
        const int f = look(p, c);
        const unsigned long long mask = __ballot(f & kHead);
        const int base = ordered_slots<WAVES>(mask, p, L.cnt, run);
        if (!(f & kValid)) continue;
        const long long x = (long long)b + (long long)p * THREADS + tid;
        // an entry that is kept belongs to the last head at or before it (a kept entry's head is kept: the same column)
        int k = -1;
        if (f & kKept) {
          k = base + __popcll(mask & upto) - 1;
          if (insert && k >= lows) ++k;
        }
        if (k >= total) continue;                      // (never: exactly `total` entries are written)
        if (seg) seg[x] = k < 0 ? -1 : o + k;
        if (f & kHead) {
          out_col[o + k] = c;
          if (out_first) out_first[o + k] = (int)x;
          if (out_val) {
            float acc = fold(x, e, c);
            if (diagonal == kDiagAdd && has_diag && c == r) acc += diag_value;
            out_val[o + k] = acc;
          }
        }
      }
    }
  }
};

// ---- degrees -------------------------------------------------------------------------------------------------------------------
struct DegreeOp {
  const int* rowptr;
  const float* val;
  double* deg;
  int count, nnz;                                      // count: rows

  using Row = RowRange;
  template <int THREADS>
  struct Scratch {
    double dsum[THREADS / 64];                         // the waves' partial row sums
  };
  __device__ bool locate(int i, Row& r) const { return row_range(rowptr, nnz, i, r); }

  template <int THREADS>
  __device__ __forceinline__ void row(int r, const Row& rr, Scratch<THREADS>& L) const {
    constexpr int WAVES = THREADS / 64;
    const int tid = threadIdx.x;
    const int b = rr.b, e = rr.e;
    if (!val) {                                        // a pattern: the row's length
      if (tid == 0) deg[r] = (double)(e - b);
      return;
    }
    double acc = 0.0;
    for (long long x = (long long)b + tid; x < e; x += THREADS) acc += (double)val[x];
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if constexpr (WAVES > 1) {
      if ((tid & 63) == 0) L.dsum[tid >> 6] = acc;
      __syncthreads();
      acc = 0.0;
      for (int w = 0; w < WAVES; ++w) acc += L.dsum[w];
    }
    if (tid == 0) deg[r] = acc;
  }
};

// ---- normalisation -------------------------------------------------------------------------------------------------------------
struct NormalizeOp {
  const int* rowptr;
  const int* col;
  const float* val;
  const double* deg;
  float* out;
  int count, n, nnz, mode;                             // count: rows

  using Row = RowRange;
  template <int THREADS>
  struct Scratch {};
  __device__ bool locate(int i, Row& r) const { return row_range(rowptr, nnz, i, r); }

  static __device__ __forceinline__ double inv_sqrt(double d) { return d == 0.0 ? 0.0 : 1.0 / sqrt(d); }

  template <int THREADS>
  __device__ __forceinline__ void row(int r, const Row& rr, Scratch<THREADS>&) const {
    const int b = rr.b, e = rr.e;
    const double d = deg[r];
    const double sr = mode == kNormSym ? inv_sqrt(d) : (d == 0.0 ? 0.0 : 1.0 / d);
    for (long long x = (long long)b + threadIdx.x; x < e; x += THREADS) {
      const double v = val ? (double)val[x] : 1.0;
      if (mode == kNormSym) {
        const int c = col[x];
        const double sc = c >= 0 && c < n ? inv_sqrt(deg[c]) : 0.0;      // (a column outside [0, n) is not followed)
        out[x] = (float)(sr * v * sc);
      } else {
        out[x] = (float)(v * sr);
      }
    }
  }
};

}  // namespace

hipError_t launch_csr_coalesce_count(const int* rowptr, const int* col, int m, int n, int nnz, int diagonal, int* out_len,
                                     void* ws, hipStream_t st) {
  CoalesceOp<false> op;
  static_cast<CoalesceArgs&>(op) = CoalesceArgs{rowptr, col, nullptr, out_len, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                m, n, nnz, kCoalesceFirst, diagonal, 0.0f};
  return launch_rows(op, static_cast<int*>(ws), st);
}

hipError_t launch_csr_coalesce_fill(const int* rowptr, const int* col, const float* val, int m, int n, int nnz, int reduce,
                                    int diagonal, float diag_value, const int* out_rowptr, int* out_col, float* out_val,
                                    int* out_first, int* seg, void* ws, hipStream_t st) {
  CoalesceOp<true> op;
  static_cast<CoalesceArgs&>(op) = CoalesceArgs{rowptr, col, val, nullptr, out_rowptr, out_col, out_val, out_first, seg,
                                                m, n, nnz, reduce, diagonal, diag_value};
  return launch_rows(op, static_cast<int*>(ws), st);
}

hipError_t launch_csr_degree(const int* rowptr, const float* val, int m, int nnz, double* deg, hipStream_t st) {
  return launch_rows(DegreeOp{rowptr, val, deg, m, nnz}, nullptr, st);
}

hipError_t launch_csr_normalize(const int* rowptr, const int* col, const float* val, int m, int n, int nnz, const double* deg,
                                int mode, float* out_val, hipStream_t st) {
  return launch_rows(NormalizeOp{rowptr, col, val, deg, out_val, m, n, nnz, mode}, nullptr, st);
}

}  // namespace gcn
