// aggregate_quantile.hip — order statistics of every CSR row's neighbourhood (the median of Median-GCN / DeepRobust's
// MedianGCN, PyG's MedianAggregation and QuantileAggregation(interpolation="lower")): for a row of d entries, a column j
// and up to four quantiles q[i],
//
//   out[r, i k + j] = the element of rank t = floor(q[i] (d - 1)) of { x[col[e], j] : e an entry of row r }, ordered
//                     ascending by (value, entry index), -0.0 equal to +0.0, +-inf ordinary values: its bits
//   arg[r, i k + j] = that entry's index into col          (an empty row: 0 and -1)
//   a column that holds a NaN gets the first NaN entry's bits and index in every plane (gcn_aggregate_csr's rule)
//
// A selection: nothing is rounded, and the gradient goes to the selected entry through gcn_aggregate_backward_csr.  max and
// min fold one entry at a time into a (value, entry) state; an order statistic needs the whole column of a neighbourhood at
// once, so nothing of gather_rows.h's wave (entry slots x columns, states merged by a butterfly) carries over.  Here A LANE
// OWNS A COLUMN: a wave covers 64 consecutive columns of one row (k wider than 64 is tiled over blockIdx.y), every gather
// of an entry is one contiguous 256-byte read of x by the wave, and everything a lane selects from is private to it: no
// cross-lane traffic, no atomics, and the same bits at every call.  The matrix cores have no part in it: a selection does
// no multiply-accumulate.  Plan-free like the sibling units: the caller's CSR, kernels only (the two flag words are
// cleared by a kernel), the host never reads a row length.  Three classes by row length, chosen inside the kernels:
//
//   d <= 32 (kQuantileShort)   quantile_short_kernel, a wave per row.  The d values of the lane's column go into registers
//       as 64-bit words (monotone key << 32 | local index << 1 | "was -0.0"), padded with a sentinel that sorts last, and
//       through Batcher's odd-even merge network of 4, 8, 16 or 32 inputs, written as constant-bound loops that unroll
//       into compare-exchanges on named registers.  All nq ranks are read off the one sort.  No LDS, no workspace.  This
//       kernel also writes the empty rows and raises the flags for the two classes below.
//   d <= 2048 (kSampleLongRow) quantile_medium_kernel, a wave per row: an MSB-first radix select on the 32-bit key, 4 bits
//       a pass.  The lane's histogram is 16 words of LDS per rank at [rank][bin][lane]: the bank is the lane, so no
//       conflicts and no atomics, and 4 KiB a rank and wave instead of the 64 KiB of an 8-bit digit, which would leave
//       two waves on a CU.  The row is re-gathered once per digit (8 passes) and once more to find the entry whose ordinal
//       among the entries of the selected key is what is left of the rank: that ordinal is the tie rule.  The nq ranks
//       are taken one after the other (kRanksPerWalk).
//   longer                     the same select by a 256-thread workgroup through long_rows_kernel (row_dispatch.h): the
//       four waves take contiguous quarters of the row, each its own histograms, which every wave sums after a barrier.
//       The counts are 32 bits (d < 2^31).  The last digit's per-wave counts are the numbers of entries of the selected
//       key in the earlier quarters, so the final walk needs no counting pass: the one wave whose quarter holds the
//       ordinal writes.
//
// Element accesses only: with a column per lane a 16-byte access would put four columns' sort state (4 x 64 registers)
// into a lane, and the wave's read of a row is already one contiguous request.  Any alignment of x, out and arg.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <type_traits>

#include "aggregate_multi.h"
#include "aggregate_quantile.h"
#include "row_dispatch.h"
#include "spmm_kernels.h"

namespace gcn {
namespace {

using u64 = unsigned long long;

struct QuantileArgs {
  const int *rowptr, *col;
  const float* x;
  float* out;
  int* arg;
  int m, k, nq;
  double q[kQuantileMax];
};

// ascending in the key = ascending in the value, -0.0 and +0.0 the same key (a NaN gets some key: its column is overruled)
__device__ __forceinline__ unsigned to_key(float v) {
  unsigned u = __float_as_uint(v);
  u = (u << 1) == 0 ? 0u : u;
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float from_key(unsigned key, bool negzero) {
  const unsigned u = (key >> 31) ? key ^ 0x80000000u : ~key;
  return __uint_as_float(negzero ? 0x80000000u : u);
}
// one multiply in double, as the host reference does it (d >= 1)
__device__ __forceinline__ int rank_of(double q, int d) { return (int)floor(q * (double)(d - 1)); }

__device__ __forceinline__ void store_planes(const QuantileArgs& a, int r, int j, int i, float v, int e) {
  const size_t at = (size_t)r * a.nq * a.k + (size_t)i * a.k + j;
  a.out[at] = v;
  a.arg[at] = e;
}

// ---- short rows: a sorting network in registers ----------------------------------------------------------------------------
// Batcher's odd-even merge sort of N words, ascending; every bound is a constant, so the loops unroll into compare-exchanges
// of named registers
template <int N>
__device__ __forceinline__ void sort_network(u64 (&w)[N]) {
#pragma unroll
  for (int p = 1; p < N; p <<= 1) {
#pragma unroll
    for (int s = p; s >= 1; s >>= 1) {
#pragma unroll
      for (int j = s % p; j + s < N; j += 2 * s) {
#pragma unroll
        for (int i = 0; i < s; ++i) {
          if (i + j + s < N && (i + j) / (2 * p) == (i + j + s) / (2 * p)) {
            const u64 lo = w[i + j], hi = w[i + j + s];
            const bool swap = lo > hi;
            w[i + j] = swap ? hi : lo;
            w[i + j + s] = swap ? lo : hi;
          }
        }
      }
    }
  }
}

// a row of 1 <= d <= N entries starting at b: lane `lane` has column j
template <int N>
__device__ __forceinline__ void short_row(const QuantileArgs& a, int r, int b, int d, int lane, int j, bool jok) {
  const int jl = jok ? j : 0;                          // (lanes past k gather column 0 and keep nothing)
  const int mine = a.col[b + (lane < d ? lane : 0)];   // (d <= 64: one coalesced load of the row's indices)
  float v[N];
#pragma unroll
  for (int s = 0; s < N; ++s)                          // (past the end: the last entry again, all N loads in flight)
    v[s] = a.x[(size_t)__builtin_amdgcn_readlane(mine, s < d ? s : d - 1) * a.k + jl];
  u64 w[N];
  int nan_at = N;
  float nan_v = 0.f;
#pragma unroll
  for (int s = 0; s < N; ++s) {
    const bool isnan = s < d && v[s] != v[s];
    nan_v = isnan && nan_at == N ? v[s] : nan_v;
    nan_at = isnan && nan_at == N ? s : nan_at;
    const unsigned low = (unsigned)(s << 1) | (__float_as_uint(v[s]) == 0x80000000u ? 1u : 0u);
    w[s] = s < d ? ((u64)to_key(v[s]) << 32) | low : ~0ull;                      // (the sentinel: above every entry)
  }
  sort_network<N>(w);
  for (int i = 0; i < a.nq; ++i) {
    const int t = rank_of(a.q[i], d);
    u64 sel = w[0];
#pragma unroll
    for (int s = 1; s < N; ++s) sel = s == t ? w[s] : sel;                       // (t is wave-uniform; no indexed register)
    const unsigned low = (unsigned)sel;
    const bool nan = nan_at < N;
    if (jok) store_planes(a, r, j, i, nan ? nan_v : from_key((unsigned)(sel >> 32), low & 1u), b + (nan ? nan_at : (int)(low >> 1)));
  }
}

__global__ void __launch_bounds__(256) quantile_short_kernel(QuantileArgs a, int* __restrict__ flags) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.m) return;
  const int r = (int)row, j = blockIdx.y * 64 + lane;
  const bool jok = j < a.k;
  const int b = a.rowptr[r], d = a.rowptr[r + 1] - b;
  if (d > kQuantileShort) {                             // (every writer writes the same word)
    if (lane == 0) flags[d > kSampleLongRow ? 1 : 0] = 1;
  } else if (d > 16) {
    short_row<32>(a, r, b, d, lane, j, jok);
  } else if (d > 8) {
    short_row<16>(a, r, b, d, lane, j, jok);
  } else if (d > 4) {
    short_row<8>(a, r, b, d, lane, j, jok);
  } else if (d > 0) {
    short_row<4>(a, r, b, d, lane, j, jok);
  } else if (jok) {
    for (int i = 0; i < a.nq; ++i) store_planes(a, r, j, i, 0.f, -1);
  }
}

// ---- medium and long rows: a radix select, 4 bits a pass ------------------------------------------------------------------
struct NoWords {};
template <int NQ, int WAVES>
struct RadixScratch {
  unsigned hist[WAVES][NQ][16][64];                    // [wave][rank][bin][lane]: a lane's words are its own, bank = lane
  [[no_unique_address]] std::conditional_t<(WAVES > 1), int[WAVES][64], NoWords> nan;   // a wave's first NaN entry
};

// f(e, x[col[e], jl]) for the entries e of [sb, se) in ascending order: 64 indices per coalesced load, eight gathers in
// flight; the control flow is wave-uniform
template <class F>
__device__ __forceinline__ void walk_column(const QuantileArgs& a, unsigned sb, unsigned se, int lane, int jl, F&& f) {
  for (unsigned e0 = sb; e0 < se; e0 += 64) {          // (unsigned: se may be within 64 of 2^31)
    const int cnt = se - e0 < 64 ? (int)(se - e0) : 64;
    const int mine = a.col[e0 + (lane < cnt ? lane : 0)];
    for (int i0 = 0; i0 < cnt; i0 += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        v[u] = a.x[(size_t)__builtin_amdgcn_readlane(mine, i0 + u < cnt ? i0 + u : cnt - 1) * a.k + jl];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (i0 + u < cnt) f((int)(e0 + i0 + u), v[u]);
    }
  }
}

// the ranks i0 .. i0 + NQ - 1 (those below a.nq) of row r = the d entries from b, by WAVES waves of one workgroup, every
// thread of which calls this with the same arguments (WAVES == 1: no barrier, a wave for itself)
template <int NQ, int WAVES>
__device__ __forceinline__ void radix_row(const QuantileArgs& a, int r, int b, int d, int i0, RadixScratch<NQ, WAVES>& S) {
  const int lane = threadIdx.x & 63, wave = WAVES > 1 ? (int)(threadIdx.x >> 6) : 0;
  unsigned(&H)[WAVES][NQ][16][64] = S.hist;
  unsigned(&mineH)[NQ][16][64] = WAVES > 1 ? H[wave] : H[0];
  const int j = blockIdx.y * 64 + lane;
  const bool jok = j < a.k;
  const int jl = jok ? j : 0;
  unsigned sb = (unsigned)b, se = (unsigned)b + (unsigned)d;
  if constexpr (WAVES > 1) {                            // contiguous parts, whole 64-entry loads each
    const unsigned part = ((((unsigned)d + WAVES - 1) / WAVES) + 63u) & ~63u;
    const unsigned lo = (unsigned)wave * part < (unsigned)d ? (unsigned)wave * part : (unsigned)d;
    const unsigned hi = lo + part < (unsigned)d ? lo + part : (unsigned)d;
    sb = (unsigned)b + lo;
    se = (unsigned)b + hi;
  }
  unsigned prefix[NQ], left[NQ], before[NQ];           // the key's digits so far; the rank among what is left; (below)
  bool live[NQ];
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    live[i] = i0 + i < a.nq;
    prefix[i] = 0u;
    left[i] = live[i] ? (unsigned)rank_of(a.q[i0 + i], d) : 0u;
    before[i] = 0u;
  }
  int nan_e = INT_MAX;                                 // the column's first NaN entry
  for (int p = 0; p < 8; ++p) {
    const int shift = 28 - 4 * p;
    const unsigned mask = p ? 0xffffffffu << (shift + 4) : 0u;                   // the digits already fixed
#pragma unroll
    for (int i = 0; i < NQ; ++i)
#pragma unroll
      for (int bin = 0; bin < 16; ++bin) mineH[i][bin][lane] = 0u;
    walk_column(a, sb, se, lane, jl, [&](int e, float v) {
      const unsigned key = to_key(v);
      if (p == 0) nan_e = v != v && nan_e == INT_MAX ? e : nan_e;
#pragma unroll
      for (int i = 0; i < NQ; ++i)
        if (live[i] && ((key ^ prefix[i]) & mask) == 0u) mineH[i][(key >> shift) & 15u][lane] += 1u;
    });
    if constexpr (WAVES > 1) {
      if (p == 0) S.nan[wave][lane] = nan_e;
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < NQ; ++i) {                     // the bin that holds rank left[i]; every wave finds the same
      unsigned below = 0u, digit = 15u;
      bool found = false;
#pragma unroll
      for (unsigned bin = 0; bin < 16; ++bin) {
        unsigned h = 0u;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) h += H[w][i][bin][lane];
        const bool here = !found && below + h > left[i];
        digit = here ? bin : digit;
        found = found || here;
        below = found ? below : below + h;
      }
      left[i] -= below;
      prefix[i] |= digit << shift;
      if (p == 7) {                                    // entries of the selected key in the earlier waves' parts
#pragma unroll
        for (int w = 0; w < WAVES; ++w) before[i] += w < wave ? H[w][i][digit][lane] : 0u;
      }
    }
    if constexpr (WAVES > 1) {
      if (p == 0) {
#pragma unroll
        for (int w = 0; w < WAVES; ++w) nan_e = S.nan[w][lane] < nan_e ? S.nan[w][lane] : nan_e;
      }
      __syncthreads();                                 // (the next pass clears what the other waves have just read)
    }
  }
  // the entry number left[i] - before[i] of the key, in this wave's part.  EVERY lane walks, the lanes of a NaN column too:
  // the walk hands the indices out by readlane, which must find every lane's load done
  unsigned seen[NQ];
  int at[NQ];
  float val[NQ];
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    seen[i] = 0u;
    at[i] = -1;
    val[i] = 0.f;
  }
  walk_column(a, sb, se, lane, jl, [&](int e, float v) {
    const unsigned key = to_key(v);
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const bool same = key == prefix[i];
      const bool hit = same && seen[i] == left[i] - before[i];                   // (a wave before or past the ordinal: never)
      at[i] = hit ? e : at[i];
      val[i] = hit ? v : val[i];
      seen[i] += same ? 1u : 0u;
    }
  });
  const bool nan = nan_e != INT_MAX;                   // the first NaN entry overrules every plane; wave 0 writes it
  float nan_v = 0.f;
  if (nan) nan_v = a.x[(size_t)a.col[nan_e] * a.k + jl];
#pragma unroll
  for (int i = 0; i < NQ; ++i)
    if (jok && live[i] && (nan ? wave == 0 : at[i] >= 0)) store_planes(a, r, j, i0 + i, nan ? nan_v : val[i], nan ? nan_e : at[i]);
}

// NQ, the ranks a walk serves, is 1 in both kernels below: three ranks off one walk measured 3.6 times one rank on the
// Reddit-shaped graph, three walks 3.0 (the lane's read-add-write of LDS per entry and rank bounds the pass,
// not the gather, and 48 KiB of histograms leave three waves a SIMD)
constexpr int kRanksPerWalk = 1;

__global__ void __launch_bounds__(256) quantile_medium_kernel(QuantileArgs a, const int* __restrict__ flags) {
  __shared__ RadixScratch<kRanksPerWalk, 1> S[4];       // one per wave; no wave reads another's
  if (flags[0] == 0) return;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.m) return;
  const int r = (int)row, b = a.rowptr[r], d = a.rowptr[r + 1] - b;
  if (d <= kQuantileShort || d > kSampleLongRow) return;
  for (int i0 = 0; i0 < a.nq; i0 += kRanksPerWalk) radix_row<kRanksPerWalk, 1>(a, r, b, d, i0, S[threadIdx.x >> 6]);
}

// the op of long_rows_kernel (row_dispatch.h), whose grid gets the column tiles as its y extent
struct QuantileLongOp {
  QuantileArgs a;
  int count, nnz;
  struct Row { int b, e; };
  template <int THREADS> using Scratch = RadixScratch<kRanksPerWalk, THREADS / 64>;
  __device__ __forceinline__ bool locate(int i, Row& r) const {
    r.b = a.rowptr[i];
    r.e = a.rowptr[i + 1];
    return true;
  }
  template <int THREADS>
  __device__ __forceinline__ void row(int i, const Row& r, Scratch<THREADS>& L) const {
    for (int i0 = 0; i0 < a.nq; i0 += kRanksPerWalk) radix_row<kRanksPerWalk, THREADS / 64>(a, i, r.b, r.e - r.b, i0, L);
  }
};

}  // namespace

hipError_t launch_aggregate_quantile(const int* rowptr, const int* col, int m, int nnz, const float* x, int k, const double* q,
                                     int nq, float* out, int* arg, void* ws, hipStream_t st) {
  QuantileArgs a{rowptr, col, x, out, arg, m, k, nq, {0., 0., 0., 0.}};
  for (int i = 0; i < nq; ++i) a.q[i] = q[i];
  const long long tiles = ((long long)k + 63) / 64;
  if (tiles > 65535) return hipErrorInvalidValue;      // (the grid's y extent)
  int* flags = static_cast<int*>(ws);
  if (hipError_t e = launch_fill_words(flags, 2, 0u, st); e != hipSuccess) return e;
  const dim3 grid((unsigned)(((long long)m + 3) / 4), (unsigned)tiles);
  quantile_short_kernel<<<grid, 256, 0, st>>>(a, flags);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  if (nnz <= kQuantileShort) return hipSuccess;        // (no row can be longer)
  quantile_medium_kernel<<<grid, 256, 0, st>>>(a, flags);
  if (hipError_t e = hipGetLastError(); e != hipSuccess || nnz <= kSampleLongRow) return e;
  const QuantileLongOp op{a, m, nnz};
  long_rows_kernel<QuantileLongOp, true><<<dim3((unsigned)(m < kLongBlocks ? m : kLongBlocks), (unsigned)tiles), 256, 0, st>>>(op, flags + 1);
  return hipGetLastError();
}

}  // namespace gcn
