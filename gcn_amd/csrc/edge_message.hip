// edge_message.hip — message passing with a feature VECTOR per stored entry (DGL's u_op_e -> reduce; GINE, MPNN, CGConv):
//
//   forward     out[r, j] = sum / max / min over the entries e of row r of msg(e, j)        (arg[r, j] = the winning e)
//   backward x  gx[c, j]  = sum over the entries t of row c of the TRANSPOSED pattern of g[r, j] * D * (w[e, j] if mul),
//               r = trow[t], e = tperm[t]
//   backward e  ge[e, j]  = g[row(e), j] * D * (x[col[e], j] if mul)                        (one writer per element)
//
// The message, the same in every kernel: t = x[c, j] + w[e, j] (add) or x[c, j] * w[e, j] (mul), ONE fp32 operation rounded
// once; then act: none, or relu(t) = t < 0 ? +0 : t (NaN and -0.0 pass: the fused SpMM epilogue's rule).  D = t <= 0 ? 0 : 1
// under relu (torch's threshold_backward: a NaN t passes the gradient, and D selects, it does not multiply), 1 without.
// HIP's __fadd_rn / __fmul_rn are a plain + and * that the compiler may fuse with the accumulation once inlined
// (spgemm.hip), so contraction is off for everything this file defines and every operation written here is rounded once.
//
// Plan-free like aggregate.hip and multihead.hip: the caller's CSR in entry order, one 4-byte memset node and kernels (legal
// inside a stream capture), the host never reads a row length, no atomics — every output has one writer and every
// reduction a fixed order, so two calls give the same bits.  Nothing of size nnz x k is kept between forward and backward:
// the backward kernels recompute t.
//
// The walk is spmm_heads' with a second stream: a wave is SLOTS = 64 / LPS entry slots x LPS lanes x VEC columns, LPS = 16,
// 32 or 64 for k / VEC <= 16, <= 32, more; wider k tiles over blockIdx.y.  VEC = 4 (16-byte accesses) when every operand is
// 16-byte aligned and k % 4 == 0, else 1.  The wave loads 64 indices (and permutation entries) with one coalesced load each
// and hands them out with ds_bpermute (__shfl); per slot four gathers of the node row and the four loads of the matching
// w rows (streamed: row e of w beside entry e; on the transposed pattern row tperm[t], a 64-bit offset) are in flight before
// the first message is formed.  The dispatch by row length is gather_rows.h's: 8 rows a wave, rows of more than kAggChunk
// entries by chunk partials per (chunk, row, column) merged in chunk order.
// Fixed order of a sum: slot s adds the entries s, s + SLOTS, ... in ascending order (a compensated chain: add_term), the
// slots are merged by the xor butterfly LPS .. 32, chunk partials in chunk order.  An empty row writes zeros (arg -1).
// Selection (max / min) is aggregate.hip's rule applied to the message: the first entry in CSR order among equals, -0.0
// equals +0.0, a NaN beats every number and the first NaN wins; the message's bits are stored.
//
// backward e walks rows as sddmm_heads does: 8 rows a wave, rows of more than kAggChunk entries by chunks on a fixed grid of
// waves, no partials.  The wave holds g[r, :], gathers x where D or mul needs it, reads w where D needs it and stores the
// rows of ge coalesced.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "edge_message.h"
#include "gather_rows.h"
#include "long_chunks.h"
#include "spmm_kernels.h"

#pragma clang fp contract(off)

namespace gcn {
namespace {

constexpr int kNone = INT_MAX;                         // "no entry yet" (a stored entry index is below nnz <= INT_MAX)

struct EdgeArgs {
  const int *idx, *perm;                               // per entry of the walked CSR: the gathered row; the entry's row of w (null: itself)
  const float *src, *w, *own;                          // gathered [*, k]; per entry [nnz, k]; the walked row's own [rows, k] or null
  float* out;
  int* arg;
  int k, mul, relu;
};

__device__ __forceinline__ float pre_act(const EdgeArgs& a, float x, float w) { return a.mul ? x * w : x + w; }
__device__ __forceinline__ float message(const EdgeArgs& a, float x, float w) {
  const float t = pre_act(a, x, w);
  return a.relu && t < 0.f ? 0.f : t;
}
__device__ __forceinline__ bool passes(const EdgeArgs& a, float t) { return !(a.relu && t <= 0.f); }

// One step of a slot's chain of additions, compensated (Kahan): `lost` carries what the last addition rounded away into the
// next.  A slot adds up to kAggChunk / SLOTS terms one after the other, and the terms of a gradient in x under op = add are
// copies of one g[r, j] wherever the pattern repeats a (row, column) pair: a thousand equal terms round the same way at
// every step, and the plain chain drifts past 1e-5 of the sum of |terms| (measured: 1.6e-5 on a column with 1 000 such
// copies).  Compensated, a chain is good to a few ulp at any length; where every addition is exact `lost` stays 0 and the
// result is the plain chain's.  (No fast-math and no contraction here: the compiler keeps the three operations.)  A sum
// that has become +-Inf or NaN carries no compensation: Inf - Inf would turn an infinite sum into a NaN at the next step.
__device__ __forceinline__ void add_term(float& sum, float& lost, float term, bool ok) {
  const float y = term - lost;
  const float t = sum + y;
  const float c = __builtin_fabsf(t) <= 3.402823466e+38f ? (t - sum) - y : 0.f;
  lost = ok ? c : lost;
  sum = ok ? t : sum;
}

// entries [b, b + n) of one row (n <= kGatherChunk) on a wave: f(xv, wv, e, ok) per entry of the lane's slot, in ascending
// order — the gathered row and the row of w (zeros unless needw) at the lane's columns jl .. jl + VEC, the entry's index in
// w, and whether the slot's entry exists (the loads of one that does not went to the chunk's first entry, a legal address)
template <int VEC, int LPS, class F>
__device__ __forceinline__ void walk_entries(const EdgeArgs& a, bool needw, int b, int n, int lane, int jl, F f) {
  constexpr int SLOTS = 64 / LPS, BATCH = 4 * SLOTS;
  const int slot = lane / LPS;
  for (int off = 0; off < n; off += 64) {              // (n <= kAggChunk: no overflow)
    const int cnt = n - off < 64 ? n - off : 64;
    const int t = b + (lane < cnt ? off + lane : 0);   // (past the end: the first entry again)
    const int my_ix = a.idx[t];
    const int my_e = a.perm ? a.perm[t] : t;
    for (int i0 = 0; i0 < cnt; i0 += BATCH) {
      float xv[4][VEC], wv[4][VEC];
      int e[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int src = i0 + SLOTS * u + slot;         // (< 64: BATCH divides 64)
        const int ix = __shfl(my_ix, src);
        e[u] = __shfl(my_e, src);
        load_row<VEC>(a.src + (size_t)ix * a.k + jl, xv[u]);
        if (needw) {
          load_row<VEC>(a.w + (size_t)e[u] * a.k + jl, wv[u]);
        } else {
#pragma unroll
          for (int v = 0; v < VEC; ++v) wv[u][v] = 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) f(xv[u], wv[u], e[u], i0 + SLOTS * u + slot < cnt);
    }
  }
}

// ---- sums: the forward (BWD = false: idx = col, src = x) and the backward in x (BWD = true: the transposed pattern,
// idx = trow, perm = tperm, src = g, own = x) ---------------------------------------------------------------------------------
template <int VEC_, int LPS_, bool BWD>
struct EdgeSumOp : EdgeArgs {
  static constexpr int VEC = VEC_, LPS = LPS_, NS = 1;
  using Acc = float[VEC];
  using Partial = float;
  struct Lane {};
  struct Row { float own[VEC]; };
  __device__ __forceinline__ Lane lane_ctx(int, bool) const { return {}; }
  __device__ __forceinline__ void reduce(int r, int b, int n, int lane, int j, bool jok, Lane, Row& row, Acc& acc) const {
    const int jl = jok ? j : 0;                        // (lanes past k gather column 0 and add nothing)
    float lost[VEC];                                   // the compensation of the slot's chain (add_term)
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = lost[v] = 0.f;
    if constexpr (BWD) {
      load_row<VEC>(own + (size_t)r * k + jl, row.own);
      walk_entries<VEC, LPS>(*this, mul || relu, b, n, lane, jl, [&](const float (&gv)[VEC], const float (&wv)[VEC], int, bool ok) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const float gw = mul ? gv[v] * wv[v] : gv[v];
          add_term(acc[v], lost[v], passes(*this, pre_act(*this, row.own[v], wv[v])) ? gw : 0.f, ok && jok);
        }
      });
    } else {
      walk_entries<VEC, LPS>(*this, true, b, n, lane, jl, [&](const float (&xv)[VEC], const float (&wv)[VEC], int, bool ok) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) add_term(acc[v], lost[v], message(*this, xv[v], wv[v]), ok && jok);
      });
    }
#pragma unroll
    for (int o = LPS; o < 64; o <<= 1) {               // the slots hold disjoint entries of the same columns
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] += __shfl_xor(acc[v], o);
    }
  }
  __device__ __forceinline__ void store(int r, int j, const Acc& acc) const { store_row<VEC>(out + (size_t)r * k + j, acc); }
  static __device__ __forceinline__ float partial(const Acc& acc, int, int v) { return acc[v]; }
  static __device__ __forceinline__ void merge_next(float& s, float o) { s += o; }
  __device__ __forceinline__ void store_one(int r, int j, int, float v) const { out[(size_t)r * k + j] = v; }
};

// ---- max / min of the message with the entry that supplied it ----------------------------------------------------------------------
template <int VEC>
struct State {
  float v[VEC];                                        // the best message so far
  int e[VEC];                                          // its entry index, kNone before the first
};
struct Pair { float v; int e; };                       // one column of a State in the workspace

// is (av, ae) the better candidate than (bv, be)?  A total order (kNone, "no entry", below everything): usable in any
// merge order.  (aggregate.hip's rule.)
template <bool MAX>
__device__ __forceinline__ bool better(float av, int ae, float bv, int be) {
  const bool an = av != av, bn = bv != bv;
  const bool gt = MAX ? av > bv : av < bv;             // (false when either is a NaN)
  const bool eq = av == bv || (an && bn);
  return ae != kNone && (be == kNone || (an && !bn) || gt || (eq && ae < be));
}

template <int VEC_, int LPS_, bool MAX>
struct EdgeSelectOp : EdgeArgs {
  static constexpr int VEC = VEC_, LPS = LPS_, NS = 1;
  using Acc = State<VEC>;
  using Partial = Pair;
  struct Lane {};
  struct Row {};
  __device__ __forceinline__ Lane lane_ctx(int, bool) const { return {}; }
  __device__ __forceinline__ void reduce(int, int b, int n, int lane, int j, bool jok, Lane, Row&, Acc& s) const {
#pragma unroll
    for (int v = 0; v < VEC; ++v) { s.v[v] = 0.f; s.e[v] = kNone; }
    walk_entries<VEC, LPS>(*this, true, b, n, lane, jok ? j : 0, [&](const float (&xv)[VEC], const float (&wv)[VEC], int e, bool ok) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) {                  // (entries arrive in ascending order: a tie keeps the earlier one)
        const float c = message(*this, xv[v], wv[v]), best = s.v[v];
        const bool take = ok && jok && (s.e[v] == kNone || (MAX ? c > best : c < best) || (c != c && best == best));
        s.v[v] = take ? c : best;
        s.e[v] = take ? e : s.e[v];
      }
    });
#pragma unroll
    for (int o = LPS; o < 64; o <<= 1) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const float ov = __shfl_xor(s.v[v], o);
        const int oe = __shfl_xor(s.e[v], o);
        const bool take = better<MAX>(ov, oe, s.v[v], s.e[v]);
        s.v[v] = take ? ov : s.v[v];
        s.e[v] = take ? oe : s.e[v];
      }
    }
  }
  __device__ __forceinline__ void store(int r, int j, const Acc& s) const {
    const size_t at = (size_t)r * k + j;
    float val[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {                    // (element stores of arg: it has no alignment rule of its own)
      val[v] = s.e[v] == kNone ? 0.f : s.v[v];
      arg[at + v] = s.e[v] == kNone ? -1 : s.e[v];
    }
    store_row<VEC>(out + at, val);
  }
  static __device__ __forceinline__ Pair partial(const Acc& s, int, int v) { return Pair{s.v[v], s.e[v]}; }
  static __device__ __forceinline__ void merge_next(Pair& s, Pair o) {
    if (better<MAX>(o.v, o.e, s.v, s.e)) s = o;
  }
  __device__ __forceinline__ void store_one(int r, int j, int, Pair p) const {     // (kNone: the row has no entry)
    const size_t at = (size_t)r * k + j;
    out[at] = p.e == kNone ? 0.f : p.v;
    arg[at] = p.e == kNone ? -1 : p.e;
  }
};

// ---- the gradient per entry: a.idx = col, a.src = x, a.own = g, a.out = ge -----------------------------------------------------------
// entries [b, b + n) of row r (0 < n <= kGatherChunk) on a wave; the lane's columns are j .. j + VEC (jok: they exist)
template <int VEC, int LPS>
__device__ __forceinline__ void grad_entries(const EdgeArgs& a, int r, int b, int n, int lane, int j, bool jok) {
  constexpr int SLOTS = 64 / LPS, BATCH = 4 * SLOTS;
  const int slot = lane / LPS;
  const int jl = jok ? j : 0;
  const bool needx = a.mul || a.relu, needw = a.relu != 0;
  float gr[VEC];
  load_row<VEC>(a.own + (size_t)r * a.k + jl, gr);
  for (int off = 0; off < n; off += 64) {
    const int cnt = n - off < 64 ? n - off : 64;
    const int my_ix = needx ? a.idx[b + (lane < cnt ? off + lane : 0)] : 0;
    for (int i0 = 0; i0 < cnt; i0 += BATCH) {
      float xv[4][VEC], wv[4][VEC];
      int e[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + SLOTS * u + slot;
        const int ix = __shfl(my_ix, i);
        e[u] = b + (i < cnt ? off + i : 0);            // (past the end: the first entry again, a legal address)
#pragma unroll
        for (int v = 0; v < VEC; ++v) xv[u][v] = wv[u][v] = 0.f;
        if (needx) load_row<VEC>(a.src + (size_t)ix * a.k + jl, xv[u]);
        if (needw) load_row<VEC>(a.w + (size_t)e[u] * a.k + jl, wv[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float o[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const float gx = a.mul ? gr[v] * xv[u][v] : gr[v];
          o[v] = passes(a, pre_act(a, xv[u][v], wv[u][v])) ? gx : 0.f;
        }
        if (jok && i0 + SLOTS * u + slot < cnt) store_row<VEC>(a.out + (size_t)e[u] * a.k + j, o);
      }
    }
  }
}

template <int VEC, int LPS>
__global__ void __launch_bounds__(256) edge_grad_rows_kernel(EdgeArgs a, const int* __restrict__ rowptr, int m,
                                                             int* __restrict__ long_flag) {
  const int lane = threadIdx.x & 63;
  const int j = (blockIdx.y * LPS + lane % LPS) * VEC;
  const bool jok = j < a.k;
  for_wave_rows<kRowsPerWave, kGatherLong>(rowptr, m, lane, long_flag, [&](int r, int b, int n) {
    if (n > 0) grad_entries<VEC, LPS>(a, r, b, n, lane, j, jok);
  });
}

template <int VEC, int LPS>
__global__ void __launch_bounds__(256) edge_grad_long_kernel(EdgeArgs a, const int* __restrict__ rowptr, int m, int nnz, int nchunks,
                                                             const int* __restrict__ long_flag) {
  if (*long_flag == 0) return;
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = gridDim.x * 4;
  const int j = (blockIdx.y * LPS + lane % LPS) * VEC;
  const bool jok = j < a.k;
  for_long_segments<kGatherChunk, kGatherLong>(rowptr, m, nnz, nchunks, wave, nwaves, lane, [&](int, int, const Segment& sg) {
    grad_entries<VEC, LPS>(a, sg.r, sg.sb, sg.se - sg.sb, lane, j, jok);
  });
}

template <int VEC, int LPS>
hipError_t run_grad_entries(const EdgeArgs& a, const int* rowptr, int m, int nnz, void* ws, hipStream_t st) {
  int* flag = static_cast<int*>(ws);
  const long long tiles = ((long long)a.k + LPS * VEC - 1) / (LPS * VEC);
  if (tiles > 65535) return hipErrorInvalidValue;      // (the grid's y extent)
  if (hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), st); e != hipSuccess) return e;
  const long long waves = ((long long)m + kRowsPerWave - 1) / kRowsPerWave;
  edge_grad_rows_kernel<VEC, LPS><<<dim3((unsigned)((waves + 3) / 4), (unsigned)tiles), 256, 0, st>>>(a, rowptr, m, flag);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  if (nnz <= kGatherLong) return hipSuccess;           // (no row can be long)
  const int nchunks = (int)(((long long)nnz + kGatherChunk - 1) / kGatherChunk);
  const int nw = nchunks < kGatherLongWaves ? nchunks : kGatherLongWaves;
  edge_grad_long_kernel<VEC, LPS><<<dim3((unsigned)((nw + 3) / 4), (unsigned)tiles), 256, 0, st>>>(a, rowptr, m, nnz, nchunks, flag);
  return hipGetLastError();
}

// ---- the one choice of a route: VEC by alignment, LPS by k / VEC ------------------------------------------------------------------
enum class Kind { sum, max, min, grad_x, grad_e };

template <int VEC, int LPS>
hipError_t run_kind(Kind kind, const EdgeArgs& a, const int* rowptr, int rows, int nnz, void* ws, hipStream_t st) {
  switch (kind) {
    case Kind::sum: return run_gather(EdgeSumOp<VEC, LPS, false>{a}, rowptr, rows, nnz, ws, st);
    case Kind::grad_x: return run_gather(EdgeSumOp<VEC, LPS, true>{a}, rowptr, rows, nnz, ws, st);
    case Kind::max: return run_gather(EdgeSelectOp<VEC, LPS, true>{a}, rowptr, rows, nnz, ws, st);
    case Kind::min: return run_gather(EdgeSelectOp<VEC, LPS, false>{a}, rowptr, rows, nnz, ws, st);
    default: return run_grad_entries<VEC, LPS>(a, rowptr, rows, nnz, ws, st);
  }
}

template <int VEC>
hipError_t run_vec(Kind kind, const EdgeArgs& a, const int* rowptr, int rows, int nnz, void* ws, hipStream_t st) {
  const int units = a.k / VEC;
  if (units <= 16) return run_kind<VEC, 16>(kind, a, rowptr, rows, nnz, ws, st);
  if (units <= 32) return run_kind<VEC, 32>(kind, a, rowptr, rows, nnz, ws, st);
  return run_kind<VEC, 64>(kind, a, rowptr, rows, nnz, ws, st);
}

// the 16-byte form needs every gathered, streamed or stored row to start on a 16-byte boundary: the base pointers and the
// row stride k * 4; anything else takes one element per lane
hipError_t run_route(Kind kind, const EdgeArgs& a, const int* rowptr, int rows, int nnz, void* ws, hipStream_t st) {
  const bool wide = a.k % 4 == 0 && aligned16(a.src) && aligned16(a.w) && aligned16(a.own) && aligned16(a.out);
  return wide ? run_vec<4>(kind, a, rowptr, rows, nnz, ws, st) : run_vec<1>(kind, a, rowptr, rows, nnz, ws, st);
}

}  // namespace

size_t edge_aggregate_workspace_bytes(int nnz, int k) {
  return 16 + 16 * (size_t)k * (size_t)(((long long)nnz + kGatherChunk - 1) / kGatherChunk);
}

hipError_t launch_edge_aggregate(const int* rowptr, const int* col, int m, int nnz, const float* x, const float* w, int k, int op,
                                 int act, int reduce, float* out, int* arg, void* ws, hipStream_t st) {
  const EdgeArgs a{col, nullptr, x, w, nullptr, out, arg, k, op == kEdgeOpMul, act == kEdgeActRelu};
  const Kind kind = reduce == kAggMax ? Kind::max : reduce == kAggMin ? Kind::min : Kind::sum;
  return run_route(kind, a, rowptr, m, nnz, ws, st);
}

hipError_t launch_edge_aggregate_backward_x(const int* trowptr, const int* trow, const int* tperm, int n, int nnz, const float* g,
                                            const float* x, const float* w, int k, int op, int act, float* gx, void* ws,
                                            hipStream_t st) {
  const EdgeArgs a{trow, tperm, g, w, x, gx, nullptr, k, op == kEdgeOpMul, act == kEdgeActRelu};
  return run_route(Kind::grad_x, a, trowptr, n, nnz, ws, st);
}

hipError_t launch_edge_aggregate_backward_e(const int* rowptr, const int* col, int m, int nnz, const float* g, const float* x,
                                            const float* w, int k, int op, int act, float* ge, void* ws, hipStream_t st) {
  const EdgeArgs a{col, nullptr, x, w, g, ge, nullptr, k, op == kEdgeOpMul, act == kEdgeActRelu};
  return run_route(Kind::grad_e, a, rowptr, m, nnz, ws, st);
}

}  // namespace gcn
