// aggregate.hip — element-wise max / min over the stored entries of every CSR row ("neighbourhood max": GraphSAGE's pooling
// aggregator), with the entry index that supplied each value, and its backward.  Plan-free like edge_softmax.hip: the
// caller's CSR in entry order, only memset nodes and kernels (legal inside a stream capture), no atomics — every output
// has one writer and every reduction a fixed order, so results are bit-identical from call to call.
//
//   forward   out[r, j] = max (min) over the entries e of row r of x[col[e], j],  arg[r, j] = that e   (empty row: 0, -1)
//   backward  gx[c, j]  = sum of g[r, j] over the entries t of row c of the TRANSPOSED pattern with arg[r, j] == tperm[t]
//             (r = trow[t]; tperm[t] = the entry's index in the forward's CSR): a gather, one writer per gx element
//
// Both are "walk a row's entries, gather a feature row per entry, fold it into a per-feature state", so they are one set
// of kernels over an operation struct (the state is a (float, int) pair per feature: (value, entry) or (sum, unused)).
//
// The wave: 4 entry slots x 16 lanes.  The 16 lanes of a slot read 16 bytes each of one gathered feature row (fp32: 64
// columns = two whole 128-byte lines, bf16: 128 columns); the four slots take the entries e, e+1, e+2, e+3.  The wave loads
// 64 indices with one coalesced load and hands them to the slots with ds_bpermute broadcasts (__shfl); four gathers per
// slot are in flight before the first is folded.  A wider k is tiled over blockIdx.y.  The four slots are merged with two
// xor-shuffles.  Operands that are not 16-byte aligned, or k not a multiple of the vector, take the same kernels with one
// element per lane (16 columns per tile).
//
// Dispatch by row length happens in the kernels (the host never reads a row length) and is gather_rows.h's: 8 rows a
// wave, rows of more than kAggChunk entries by chunk partials (here a (value, entry) pair) merged in chunk order.
//
// Selection rule (numpy's argmax / argmin): the first entry in CSR order among equals, -0.0 == +0.0; a NaN beats every
// number and the first NaN wins; +-inf are ordinary values.  No arithmetic touches a value: the bits stored are the
// winner's bits, so bf16 and fp32 share the code and the result is exact.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "gather_rows.h"
#include "spmm_kernels.h"

namespace gcn {
namespace {

constexpr int kNone = INT_MAX;                         // "no entry yet" (a stored entry index is below nnz <= INT_MAX)

using bf16_t = unsigned short;

__device__ __forceinline__ float to_float(bf16_t v) { return __uint_as_float((unsigned)v << 16); }
// the value came from a T: the conversion back is exact and keeps every bit (NaN payloads, the sign of a zero)
__device__ __forceinline__ void put_exact(float* p, float v) { *p = v; }
__device__ __forceinline__ void put_exact(bf16_t* p, float v) { *p = (bf16_t)(__float_as_uint(v) >> 16); }
// a sum: rounded once, to nearest even
__device__ __forceinline__ void put_rounded(float* p, float v) { *p = v; }
__device__ __forceinline__ void put_rounded(bf16_t* p, float v) {
  unsigned u = __float_as_uint(v);
  if ((u & 0x7fffffffu) > 0x7f800000u) { *p = (bf16_t)((u >> 16) | 0x40u); return; }
  u += 0x7fffu + ((u >> 16) & 1u);
  *p = (bf16_t)(u >> 16);
}

// VEC consecutive elements at p as floats: one 16-byte load (fp32 x 4: gather_rows.h, bf16 x 8) or one element
using gcn::load_row;                                   // (the overloads below would hide them)
using gcn::store_row;
template <int VEC>
__device__ __forceinline__ void load_row(const bf16_t* p, float (&v)[VEC]) {
  if constexpr (VEC == 8) {
    const uint4 q = *reinterpret_cast<const uint4*>(p);
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = __uint_as_float(w[i] << 16);
      v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
  } else {
    static_assert(VEC == 1);
    v[0] = to_float(p[0]);
  }
}
template <int VEC>
__device__ __forceinline__ void load_ints(const int* p, int (&v)[VEC]) {
  if constexpr (VEC == 1) {
    v[0] = p[0];
  } else {
#pragma unroll
    for (int i = 0; i < VEC; i += 4) {
      const int4 q = *reinterpret_cast<const int4*>(p + i);
      v[i] = q.x; v[i + 1] = q.y; v[i + 2] = q.z; v[i + 3] = q.w;
    }
  }
}

// VEC consecutive elements at p (a 16-byte boundary when VEC > 1) from floats: exact (the floats came from T) or rounded
template <int VEC, bool ROUND>
__device__ __forceinline__ void store_row(bf16_t* p, const float (&v)[VEC]) {
  bf16_t h[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    if constexpr (ROUND) put_rounded(&h[i], v[i]); else put_exact(&h[i], v[i]);
  }
  if constexpr (VEC == 8) {
    *reinterpret_cast<uint4*>(p) = make_uint4(h[0] | (unsigned)h[1] << 16, h[2] | (unsigned)h[3] << 16, h[4] | (unsigned)h[5] << 16,
                                              h[6] | (unsigned)h[7] << 16);
  } else {
    static_assert(VEC == 1);
    p[0] = h[0];
  }
}
template <int VEC>
__device__ __forceinline__ void store_ints(int* p, const int (&v)[VEC]) {
  if constexpr (VEC == 1) {
    p[0] = v[0];
  } else {
#pragma unroll
    for (int i = 0; i < VEC; i += 4) *reinterpret_cast<int4*>(p + i) = make_int4(v[i], v[i + 1], v[i + 2], v[i + 3]);
  }
}

template <int VEC>
struct State {
  float v[VEC];                                        // the best value so far / the running sum
  int e[VEC];                                          // its entry index, kNone before the first / unused
};
struct Pair { float v; int e; };                       // one column of a State in the workspace

// is (av, ae) the better candidate than (bv, be)?  A total order (kNone, "no entry", below everything): usable in any
// merge order.
template <bool MAX>
__device__ __forceinline__ bool better(float av, int ae, float bv, int be) {
  const bool an = av != av, bn = bv != bv;
  const bool gt = MAX ? av > bv : av < bv;             // (false when either is a NaN)
  const bool eq = av == bv || (an && bn);
  return ae != kNone && (be == kNone || (an && !bn) || gt || (eq && ae < be));
}

// ---- the operations -----------------------------------------------------------------------------------------------------
// index(t): what entry t of the walked CSR names (loaded by one lane per entry, broadcast to the slot that takes it);
// fetch(ix, j): the gathered data of that entry at columns j .. j + VEC (always a legal address: issued before it is known
// whether the slot's entry exists); fold: into the state, entries arriving in ascending order; merge: two states of
// disjoint entry sets, any order; merge_next: a partial of LATER entries into the state of earlier ones.
template <class T, int VEC_, bool MAX>
struct SelectOp {                                      // the forward
  static constexpr int VEC = VEC_;
  using Elem = T;
  const int* col;
  const T* x;
  T* out;
  int* arg;
  int k;
  struct Index { int c; };
  struct Item { float v[VEC]; };
  __device__ Index index(int t) const { return Index{col[t]}; }
  static __device__ Index bcast(Index ix, int src) { return Index{__shfl(ix.c, src)}; }
  __device__ Item fetch(Index ix, int j) const {
    Item it;
    load_row<VEC>(x + (size_t)ix.c * k + j, it.v);
    return it;
  }
  static __device__ void init(State<VEC>& s) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) { s.v[i] = 0.f; s.e[i] = kNone; }
  }
  static __device__ void fold(State<VEC>& s, const Item& it, Index, int t, bool ok) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const float v = it.v[i], b = s.v[i];
      const bool take = ok && (s.e[i] == kNone || (MAX ? v > b : v < b) || (v != v && b == b));
      s.v[i] = take ? v : b;
      s.e[i] = take ? t : s.e[i];
    }
  }
  static __device__ void merge(State<VEC>& s, const State<VEC>& o) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const bool take = better<MAX>(o.v[i], o.e[i], s.v[i], s.e[i]);
      s.v[i] = take ? o.v[i] : s.v[i];
      s.e[i] = take ? o.e[i] : s.e[i];
    }
  }
  static __device__ void merge_next(Pair& s, Pair o) {
    if (better<MAX>(o.v, o.e, s.v, s.e)) s = o;
  }
  __device__ void store(int r, int j, const State<VEC>& s) const {    // columns j .. j + VEC of row r
    float v[VEC];
    int e[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      v[i] = s.e[i] == kNone ? 0.f : s.v[i];
      e[i] = s.e[i] == kNone ? -1 : s.e[i];
    }
    const size_t at = (size_t)r * k + j;
    store_row<VEC, false>(out + at, v);
    store_ints<VEC>(arg + at, e);
  }
  __device__ void store_one(int r, int j, int, Pair p) const {        // (kNone: the row has no entry)
    const size_t at = (size_t)r * k + j;
    put_exact(out + at, p.e == kNone ? 0.f : p.v);
    arg[at] = p.e == kNone ? -1 : p.e;
  }
};

template <class T, int VEC_>
struct ScatterOp {                                     // the backward, on the transposed pattern
  static constexpr int VEC = VEC_;
  using Elem = T;
  const int *trow, *tperm;
  const T* g;
  const int* arg;
  T* gx;
  int k;
  struct Index { int r, e; };
  struct Item { float g[VEC]; int a[VEC]; };
  __device__ Index index(int t) const { return Index{trow[t], tperm[t]}; }
  static __device__ Index bcast(Index ix, int src) { return Index{__shfl(ix.r, src), __shfl(ix.e, src)}; }
  __device__ Item fetch(Index ix, int j) const {
    Item it;
    const size_t at = (size_t)ix.r * k + j;
    load_row<VEC>(g + at, it.g);
    load_ints<VEC>(arg + at, it.a);
    return it;
  }
  static __device__ void init(State<VEC>& s) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) { s.v[i] = 0.f; s.e[i] = 0; }
  }
  static __device__ void fold(State<VEC>& s, const Item& it, Index ix, int, bool ok) {
#pragma unroll
    for (int i = 0; i < VEC; ++i)
      if (ok && it.a[i] == ix.e) s.v[i] += it.g[i];
  }
  static __device__ void merge(State<VEC>& s, const State<VEC>& o) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) s.v[i] += o.v[i];
  }
  static __device__ void merge_next(Pair& s, Pair o) { s.v += o.v; }
  __device__ void store(int c, int j, const State<VEC>& s) const { store_row<VEC, true>(gx + (size_t)c * k + j, s.v); }
  __device__ void store_one(int c, int j, int, Pair p) const { put_rounded(gx + (size_t)c * k + j, p.v); }
};

// ---- entries [b, b + n) on one wave: the lane's columns are j .. j + VEC (jok: they exist) ----------------------------------
template <class Op>
__device__ __forceinline__ void walk(const Op& op, int b, int n, int lane, int j, bool jok, State<Op::VEC>& s) {
  const int slot = lane >> 4;
  const int jl = jok ? j : 0;                          // (lanes past k gather column 0 and fold nothing)
  for (int off = 0; off < n; off += 64) {              // (n <= kAggChunk: no overflow)
    const int cnt = n - off < 64 ? n - off : 64;
    const typename Op::Index mine = op.index(b + (lane < cnt ? off + lane : 0));   // (past the end: the first entry again)
    for (int i0 = 0; i0 < cnt; i0 += 16) {
      typename Op::Index ix[4];
      typename Op::Item it[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        ix[u] = Op::bcast(mine, i0 + 4 * u + slot);
        it[u] = op.fetch(ix[u], jl);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {                    // (slot s takes entries s, s + 4, ...: ascending inside a lane)
        const int i = i0 + 4 * u + slot;
        Op::fold(s, it[u], ix[u], b + off + i, jok && i < cnt);
      }
    }
  }
}

// the four slots hold disjoint entries of the same columns: every lane ends with the merged state
template <class Op>
__device__ __forceinline__ void merge_slots(State<Op::VEC>& s) {
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {
    State<Op::VEC> t;
#pragma unroll
    for (int i = 0; i < Op::VEC; ++i) {
      t.v[i] = __shfl_xor(s.v[i], o);
      t.e[i] = __shfl_xor(s.e[i], o);
    }
    Op::merge(s, t);
  }
}

// what gather_rows.h asks of an operation: 16 lanes a slot, one state per column, nothing fixed per lane
template <class Op>
struct RowsOp : Op {
  static constexpr int LPS = 16, NS = 1;
  using Acc = State<Op::VEC>;
  using Partial = Pair;
  struct Lane {};
  struct Row {};
  __device__ Lane lane_ctx(int, bool) const { return {}; }
  __device__ void reduce(int, int b, int n, int lane, int j, bool jok, Lane, Row&, Acc& s) const {
    Op::init(s);
    walk<Op>(*this, b, n, lane, j, jok, s);
    merge_slots<Op>(s);
  }
  static __device__ Pair partial(const Acc& s, int, int v) { return Pair{s.v[v], s.e[v]}; }
};

template <class Op>
hipError_t run(const Op& op, const int* rowptr, int rows, int nnz, void* ws, hipStream_t st) {
  return run_gather(RowsOp<Op>{op}, rowptr, rows, nnz, ws, st);
}

template <class T, int VEC>
hipError_t run_select(const int* rowptr, const int* col, int m, int nnz, const T* x, int k, int op, T* out, int* arg, void* ws,
                      hipStream_t st) {
  if (op == kAggMax) return run(SelectOp<T, VEC, true>{col, x, out, arg, k}, rowptr, m, nnz, ws, st);
  return run(SelectOp<T, VEC, false>{col, x, out, arg, k}, rowptr, m, nnz, ws, st);
}

}  // namespace

size_t aggregate_workspace_bytes(int nnz, int k) {
  return 16 + 16 * (size_t)k * (size_t)(((long long)nnz + kGatherChunk - 1) / kGatherChunk);
}

// the 16-byte paths need every gathered or stored row to start on a 16-byte boundary: the base pointers and the row
// stride k * sizeof(T); anything else takes one element per lane
hipError_t launch_aggregate(const int* rowptr, const int* col, int m, int nnz, const void* x, int bf16, int k, int op, void* out,
                            int* arg, void* ws, hipStream_t st) {
  const int vec = bf16 ? 8 : 4;
  const bool wide = k % vec == 0 && aligned16(x) && aligned16(out) && aligned16(arg);
  if (bf16) {
    auto xs = static_cast<const bf16_t*>(x);
    auto os = static_cast<bf16_t*>(out);
    return wide ? run_select<bf16_t, 8>(rowptr, col, m, nnz, xs, k, op, os, arg, ws, st)
                : run_select<bf16_t, 1>(rowptr, col, m, nnz, xs, k, op, os, arg, ws, st);
  }
  auto xs = static_cast<const float*>(x);
  auto os = static_cast<float*>(out);
  return wide ? run_select<float, 4>(rowptr, col, m, nnz, xs, k, op, os, arg, ws, st)
              : run_select<float, 1>(rowptr, col, m, nnz, xs, k, op, os, arg, ws, st);
}

hipError_t launch_aggregate_backward(const int* trowptr, const int* trow, const int* tperm, int n, int nnz, const void* g, int bf16,
                                     const int* arg, int k, void* gx, void* ws, hipStream_t st) {
  const int vec = bf16 ? 8 : 4;
  const bool wide = k % vec == 0 && aligned16(g) && aligned16(gx) && aligned16(arg);
  if (bf16) {
    auto gs = static_cast<const bf16_t*>(g);
    auto os = static_cast<bf16_t*>(gx);
    return wide ? run(ScatterOp<bf16_t, 8>{trow, tperm, gs, arg, os, k}, trowptr, n, nnz, ws, st)
                : run(ScatterOp<bf16_t, 1>{trow, tperm, gs, arg, os, k}, trowptr, n, nnz, ws, st);
  }
  auto gs = static_cast<const float*>(g);
  auto os = static_cast<float*>(gx);
  return wide ? run(ScatterOp<float, 4>{trow, tperm, gs, arg, os, k}, trowptr, n, nnz, ws, st)
              : run(ScatterOp<float, 1>{trow, tperm, gs, arg, os, k}, trowptr, n, nnz, ws, st);
}

}  // namespace gcn
