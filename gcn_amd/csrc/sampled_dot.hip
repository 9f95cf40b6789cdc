// sampled_dot.hip — the product of two CSR matrices SAMPLED ON A GIVEN PATTERN: for every entry (i, j) of a pattern P the
// sparse dot product of a row of X and a row of Y over their common columns (the SDDMM of sddmm.hip with sparse operands).
// It is what a gradient through spgemm.hip needs — dC/dA on A's pattern, dC/dB on B's — and, run on C's own pattern with
// X = A and Y = Bᵀ, it gives the values of C bit for bit as the fill does, with no count, no scan and no host read.
// Plan-free like coalesce.hip: the caller's arrays, one memset node and two kernels, no allocation, no host read of device
// data, no atomic; every output element has one writer.  Every access is a 4-byte one.  The contract (the rows of an entry,
// the order of its products, what a bad operand does) is written out in include/gcn_spmm.h; tests/sampled_dot_ref.py is its
// numpy twin, bit for bit.
//
// ---- the decomposition ----------------------------------------------------------------------------------------------------------
// P is walked BY ROWS through row_dispatch.h: a wave for a row of at most kSampleLongRow entries, a 256-thread workgroup for a
// longer one, so neither a hub row of P nor the screening for one is written here.  Inside a row the unit is a wave, and a
// wave takes FOUR ENTRIES of P a pass.
//   X rows of at most kSampledGroupMax (64) entries — every workload at hand: 10 to 16 — are taken by a 16-LANE GROUP per
//   entry, 16 entries of X a step: a lane loads its entry of X (a coalesced 64-byte piece per group), looks its column up in
//   Y's row by binary search, and holds fl32(x * y) when the column is there.
//   When one of the four X rows is longer, the WHOLE WAVE takes the four entries one after another, 64 entries of X a step,
//   the row bounds handed round by lane broadcast.  No lane ever walks a row alone.
// THE FOLD.  The contract adds the matched products in X's entry order.  The matches of a step are found in parallel; their
// ballot is then walked bit by bit — the lowest set bit of the group's part of the mask names the lane whose product is next,
// a lane broadcast fetches it, every lane of the group adds it to its own copy of the accumulator.  The loop runs while any
// group of the wave has a bit left, so the broadcasts sit in wave-uniform control flow; a C entry of the workloads has one
// to three products, so the serial part is short.  Steps follow each other in order, so chunk boundaries do not show.
// THE SEARCH is a lower bound over [yb, ye): at most 32 probes, every probe inside the row, whatever the row holds — on a
// row that is not ascending the result is some entry or none (the contract leaves those values open), never a fault.
//
// Not staged in LDS: in either mode one operand row is shared by all entries of a P row (X's when x_by_col == 0, Y's
// otherwise) and could be kept on chip; here the groups of a wave re-read it through the vector L1, which the rows of the
// workloads (at most a few hundred bytes) stay resident in.  DESIGN §4.21 has the byte model and what was measured.
#include <hip/hip_runtime.h>

#include "row_dispatch.h"
#include "spmm_kernels.h"

// every product and every sum is rounded once (see spgemm.hip): plain operators, contraction off for this file
#pragma clang fp contract(off)

namespace gcn {
namespace {

constexpr int kSampledGroupMax = 64;                   // X rows up to this length: a 16-lane group; longer: the whole wave

struct PRow { int b, e; };

struct SampledDotOp {
  const int* p_rowptr; const int* p_col;
  const int* x_rowptr; const int* x_col; const float* x_val;
  const int* y_rowptr; const int* y_col; const float* y_val;
  float* out;
  int count, np, nnz, nnz_x, nnz_y, w, x_by_col;       // count: rows of P; nnz: entries of P

  using Row = PRow;
  template <int THREADS>
  struct Scratch { int unused; };

  __device__ bool locate(int i, Row& r) const {
    r.b = p_rowptr[i];
    r.e = p_rowptr[i + 1];
    return r.b >= 0 && r.e >= r.b && r.e <= nnz;
  }

  // the entries [b, e) of row r of an operand — none when its row pointer is not usable
  static __device__ __forceinline__ void operand_row(const int* rowptr, int nnz_op, int r, int& b, int& e) {
    b = rowptr[r];
    e = rowptr[r + 1];
    if (b < 0 || e < b || e > nnz_op) b = e = 0;
  }

  // The dot product of X's entries [xb, xe) with Y's row [yb, ye) on a group of W lanes (16: four groups of a wave, each
  // with its own rows; 64: the wave).  Every lane of the wave calls it; returns the value in every lane of the group.
  template <int W>
  __device__ __forceinline__ float dot(int xb, int xe, int yb, int ye, int lane) const {
    const int sub = lane & (W - 1), base = lane & ~(W - 1);
    const int len = xe - xb;
    int steps = len / W + (len % W != 0);
    if constexpr (W < 64)
      for (int off = W; off < 64; off <<= 1) {           // the wave walks as long as its longest group
        const int other = __shfl_xor(steps, off, 64);
        steps = other > steps ? other : steps;
      }
    float acc = 0.0f;
    bool any = false;
    for (int s = 0; s < steps; ++s) {                    // (wave-uniform)
      const long long t = (long long)xb + (long long)s * W + sub;
      bool found = false;
      float prod = 0.0f;
      if (t < xe) {
        const int c = x_col[t];
        if (c >= 0 && c < w) {
          int lo = yb, hi = ye;
          while (lo < hi) {                              // the first entry of Y's row with a column >= c
            const int mid = lo + ((hi - lo) >> 1);
            if (y_col[mid] < c) lo = mid + 1;
            else hi = mid;
          }
          if (lo < ye && y_col[lo] == c) {
            found = true;
            prod = (x_val ? x_val[t] : 1.0f) * (y_val ? y_val[lo] : 1.0f);
          }
        }
      }
      unsigned long long m = __ballot(found) >> base;
      if constexpr (W < 64) m &= (1ull << W) - 1ull;
      while (__ballot(m != 0ull) != 0ull) {              // (wave-uniform: the broadcast below is met by all 64 lanes)
        const int src = m != 0ull ? base + __builtin_ctzll(m) : lane;
        const float v = __shfl(prod, src, 64);
        if (m != 0ull) {
          acc = any ? acc + v : v;                       // the first product, not 0 + it: a lone -0.0 stays -0.0
          any = true;
          m &= m - 1ull;
        }
      }
    }
    return any ? acc : 0.0f;
  }

  // one row of P on a workgroup of THREADS threads (every thread of the workgroup calls it with the same arguments)
  template <int THREADS>
  __device__ __forceinline__ void row(int i, const Row& rr, Scratch<THREADS>&) const {
    constexpr int GROUPS = THREADS / 16;
    const int tid = threadIdx.x, lane = tid & 63, group = tid >> 4;
    const int passes = (int)(((long long)rr.e - rr.b + GROUPS - 1) / GROUPS);
    for (int p = 0; p < passes; ++p) {                   // (workgroup-uniform; no barrier inside)
      const long long pe = (long long)rr.b + (long long)p * GROUPS + group;    // this group's entry of P
      const bool live = pe < rr.e;
      int xb = 0, xe = 0, yb = 0, ye = 0;
      if (live) {
        const int j = p_col[pe];
        if (j >= 0 && j < np) {                          // (a column out of range: no rows, the value +0.0)
          operand_row(x_rowptr, nnz_x, x_by_col ? j : i, xb, xe);
          operand_row(y_rowptr, nnz_y, x_by_col ? i : j, yb, ye);
          if (yb == ye) xe = xb;                         // (nothing can match)
        }
      }
      int longest = xe - xb;
      for (int off = 16; off < 64; off <<= 1) {
        const int other = __shfl_xor(longest, off, 64);
        longest = other > longest ? other : longest;
      }
      if (longest <= kSampledGroupMax) {                 // (wave-uniform)
        const float v = dot<16>(xb, xe, yb, ye, lane);
        if (live && (lane & 15) == 0) out[pe] = v;
      } else {
        for (int q = 0; q < 4; ++q) {
          const int src = q * 16;
          const int qxb = __shfl(xb, src, 64), qxe = __shfl(xe, src, 64), qyb = __shfl(yb, src, 64), qye = __shfl(ye, src, 64);
          const int qlive = __shfl((int)live, src, 64);
          if (!qlive) break;                             // (wave-uniform; the entries of a wave are live from the front)
          const float v = dot<64>(qxb, qxe, qyb, qye, lane);
          if (lane == src) out[pe] = v;
        }
      }
    }
  }
};

}  // namespace

hipError_t launch_csr_sampled_dot(const int* p_rowptr, const int* p_col, int mp, int np, int nnz_p, const int* x_rowptr,
                                  const int* x_col, const float* x_val, int nnz_x, const int* y_rowptr, const int* y_col,
                                  const float* y_val, int nnz_y, int w, int x_by_col, float* out, void* ws, hipStream_t st) {
  const SampledDotOp op{p_rowptr, p_col, x_rowptr, x_col, x_val, y_rowptr, y_col, y_val, out,
                        mp, np, nnz_p, nnz_x, nnz_y, w, x_by_col != 0};
  return launch_rows(op, static_cast<int*>(ws), st);
}

}  // namespace gcn
