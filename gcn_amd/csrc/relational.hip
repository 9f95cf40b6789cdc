// relational.hip — the aggregation of relational graph convolutions with basis decomposition (R-GCN; PyG's RGCNConv,
// DGL's RelGraphConv): every stored entry carries a relation type, and ONE gather of the neighbour's row feeds B planes.
//
//   forward    Y[r, b k + j] = sum over the entries e of row r of  w(e, b) x[col[e], j],   w(e, b) = coeff[etype[e], b] values[e]
//              (the layer's output is Y.view(m, B k) @ V.view(B k, out): one dense product for all relations)
//   typed      coeff == null, B = R: plane b takes exactly the entries of type b, weighted by values[e]
//   grad x     gx[c, j] = sum over the entries t of row c of the TRANSPOSED pattern (r = trow[t], e = tperm[t]) of
//              sum_b w(e, b) g[r, b k + j]
//   grad coeff gcoeff[t, b] = sum over the entries e of type t of  values[e] sum_j x[col[e], j] g[row[e], b k + j]
//
// Plan-free like aggregate_multi.hip and multihead.hip: the caller's CSR in entry order, one 4-byte memset node and kernels
// per pass (legal inside a stream capture), the host never reads a row length or a type, no atomics — every output has
// one writer and every sum a fixed order, so two calls give the same bits.  The dispatch by row length is gather_rows.h's:
// 8 rows a wave, rows of more than kAggChunk entries by chunk partials merged in chunk order.  Element offsets are 64-bit.
//
// A type outside [0, R) — one unsigned compare, so -1 is a mask — contributes nothing to any of the three, and coeff is
// never read for it.
//
// The forward.  A wave is SLOTS = 64 / LPS entry slots x LPS lanes x VEC columns (spmm_heads' choice: LPS = 16, 32 or 64
// for k / VEC <= 16, <= 32, more; VEC = 4 when x and out are 16-byte aligned and k % 4 == 0, else 1).  A lane keeps NB VEC
// running sums, NB in {1, 2, 4, 8} the planes of the pass: B > 8 runs as ceil(B / 8) passes of 8 planes, the last with the
// smallest NB covering what is left (planes past B are computed on plane 0's operands and not stored); every pass gathers x
// again, so B <= 8 is the shape this unit is for.  The wave loads 64 indices, types and values with one coalesced load
// each and hands them out by __shfl; a slot has kInFlight(NB) entries' gathers and coefficient loads in flight before the
// first fma.  The NB coefficients of an entry's type are the same address across a slot (a broadcast load): 16-byte loads
// when B % 4 == 0 and the table is 16-byte aligned (a pass starts at a multiple of 8), one word each otherwise.
//   w = coeff * values is rounded once; then acc[q] = fmaf(w_q, x, acc[q]).
//   Fixed order: slot s adds the entries s, s + SLOTS, ... of a run of at most kAggChunk entries in ascending order, the slots
//   are merged by the xor butterfly LPS .. 32, chunk partials in chunk order (spmm_heads' order).
//   Typed mode is a predicated fma (plane == type), not a product with 0: a non-finite row of x reached only through
//   relation t touches plane t alone.  In basis mode 0 * NaN = NaN reaches every plane, as the dense formula's would.
//
// The gradient in x is the same wave on the transposed pattern with VEC sums a lane: per entry one fma chain over b = 0 ..
// B - 1 (B at run time, four planes' gathers in flight), acc = fmaf(w(e, b), g[r, b k + j], acc); typed mode gathers
// the one plane of the entry's type (four entries in flight).  Entries ascending per slot, slots and chunks as above.
//
// The gradient in coeff walks the RELATION-MAJOR view with the same engine: a "row" is a relation (relptr [R + 1]; per entry
// in type-major stable order its row, column and CSR index), so a large relation is spread over the chip by the long-row
// path.  A wave is SLOTS x LPS lanes x VEC columns of x as above, but the columns of a wide k are walked by the lane (tile
// jt = 0, 1, ...: columns (jt LPS + lane % LPS) VEC ..), not by the grid, so a (type, plane) has one writer.  A lane keeps NB
// VEC sums; per (entry, tile) it gathers x[col] once and the NB segments of g[row], t = values * x rounded once,
// s[q][v] = fmaf(t_v, g_q[v], s[q][v]).
//   Fixed order: slot s takes the entries s, s + SLOTS, ... of a run ascending, an entry's tiles ascending; at the run's end
//   plane q's total is ((s[q][0] + s[q][1]) + s[q][2]) + s[q][3], then the xor butterfly 1, 2, .. 32 over all 64 lanes (the
//   lanes of a slot first, then the slots); chunk partials in chunk order.  Lane q then carries plane q: to the engine the
//   op looks like one of VEC = 1, LPS = 64 and k = the planes of the pass.  The entries behind relptr[R] (masked types) are
//   never walked; the chunks that hold only them find no long row and write nothing that is read.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "gather_rows.h"
#include "relational.h"
#include "spmm_kernels.h"

#pragma clang fp contract(off)

namespace gcn {
namespace {

// entries a slot keeps in flight: with 8 planes the coefficients of 4 entries would cost 32 registers more and an
// occupancy step
constexpr int in_flight(int NB) { return NB >= 8 ? 2 : 4; }

// ---- the forward ---------------------------------------------------------------------------------------------------------
struct RelArgs {
  const int *idx, *etype;
  const float *x, *coeff, *values;
  float* out;
  int k, R, B, b0;                                     // b0: the first plane of this pass
  bool cw;                                             // 16-byte coefficient loads
  size_t w;                                            // B * k, the row stride of out
};

template <int VEC_, int LPS_, int NB, bool TYPED>
struct RelForwardOp : RelArgs {
  static constexpr int VEC = VEC_, LPS = LPS_, NS = NB;
  using Acc = float[NB * VEC];
  using Partial = float;
  struct Lane {};
  struct Row {};
  __device__ __forceinline__ Lane lane_ctx(int, bool) const { return {}; }
  __device__ __forceinline__ int live() const { return B - b0 < NB ? B - b0 : NB; }

  // the pass's coefficients of one type, cp = coeff + type * B + b0 (the same address across a slot)
  __device__ __forceinline__ void load_coeff(const float* cp, int nlive, float (&c)[NB]) const {
    if constexpr (NB >= 4) {
      if (cw) {                                        // (then B % 4 == 0: every plane of the pass exists)
#pragma unroll
        for (int q = 0; q < NB; q += 4) {
          const float4 f = *reinterpret_cast<const float4*>(cp + q);
          c[q] = f.x; c[q + 1] = f.y; c[q + 2] = f.z; c[q + 3] = f.w;
        }
        return;
      }
    }
#pragma unroll
    for (int q = 0; q < NB; ++q) c[q] = cp[q < nlive ? q : 0];
  }

  __device__ __forceinline__ void reduce(int, int b, int n, int lane, int j, bool jok, Lane, Row&, Acc& acc) const {
    constexpr int SLOTS = 64 / LPS, U = in_flight(NB), BATCH = U * SLOTS;
    const int slot = lane / LPS;
    const int jl = jok ? j : 0;                        // (lanes past k gather column 0 and add nothing)
    const int nlive = live();
#pragma unroll
    for (int v = 0; v < NB * VEC; ++v) acc[v] = 0.f;
    for (int off = 0; off < n; off += 64) {            // (n <= kAggChunk: no overflow)
      const int cnt = n - off < 64 ? n - off : 64;
      const int t = b + (lane < cnt ? off + lane : 0); // (past the end: the first entry again, a legal address)
      const int my_ix = idx[t], my_ty = etype[t];
      const float my_val = values ? values[t] : 1.f;
      for (int i0 = 0; i0 < cnt; i0 += BATCH) {
        float xv[U][VEC], wq[U][NB];
        int ty[U];
        bool in[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int src = i0 + SLOTS * u + slot;       // (< 64: BATCH divides 64)
          const int ix = __shfl(my_ix, src);
          const float val = __shfl(my_val, src);
          ty[u] = __shfl(my_ty, src);
          in[u] = (unsigned)ty[u] < (unsigned)R;
          load_row<VEC>(x + (size_t)ix * k + jl, xv[u]);
          if constexpr (TYPED) {
#pragma unroll
            for (int q = 0; q < NB; ++q) wq[u][q] = val;
          } else {
            const float* cp = coeff + (size_t)(in[u] ? ty[u] : 0) * B + b0;            // (a masked entry reads type 0's and adds nothing)
            float c[NB];
            load_coeff(cp, nlive, c);
#pragma unroll
            for (int q = 0; q < NB; ++q) wq[u][q] = c[q] * val;
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {                  // (slot s takes entries s, s + SLOTS, ...: ascending inside a lane)
          const bool ok = jok && in[u] && i0 + SLOTS * u + slot < cnt;
#pragma unroll
          for (int q = 0; q < NB; ++q) {
            const bool okq = TYPED ? ok && ty[u] == b0 + q : ok;
#pragma unroll
            for (int v = 0; v < VEC; ++v)
              acc[q * VEC + v] = okq ? __builtin_fmaf(wq[u][q], xv[u][v], acc[q * VEC + v]) : acc[q * VEC + v];
          }
        }
      }
    }
#pragma unroll
    for (int o = LPS; o < 64; o <<= 1) {               // the slots hold disjoint entries of the same columns
#pragma unroll
      for (int v = 0; v < NB * VEC; ++v) acc[v] += __shfl_xor(acc[v], o);
    }
  }

  static __device__ __forceinline__ float partial(const Acc& acc, int t, int v) { return acc[t * VEC + v]; }
  static __device__ __forceinline__ void merge_next(float& s, float o) { s += o; }
  __device__ __forceinline__ void store(int r, int j, const Acc& acc) const {
    const int nlive = live();
    float* row = out + (size_t)r * w + (size_t)b0 * k + j;
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      float v[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) v[i] = acc[q * VEC + i];
      if (q < nlive) store_row<VEC>(row + (size_t)q * k, v);
    }
  }
  __device__ __forceinline__ void store_one(int r, int j, int t, float v) const {
    if (t < live()) out[(size_t)r * w + (size_t)(b0 + t) * k + j] = v;
  }
};

// ---- the gradient in x -----------------------------------------------------------------------------------------------------
struct RelBackXArgs {
  const int *trow, *tperm, *etype;
  const float *g, *coeff, *values;
  float* gx;
  int k, R, B;
  size_t w;                                            // B * k, the row stride of g
};

template <int VEC_, int LPS_, bool TYPED>
struct RelBackXOp : RelBackXArgs {
  static constexpr int VEC = VEC_, LPS = LPS_, NS = 1;
  using Acc = float[VEC];
  using Partial = float;
  struct Lane {};
  struct Row {};
  __device__ __forceinline__ Lane lane_ctx(int, bool) const { return {}; }

  __device__ __forceinline__ void reduce(int, int b, int n, int lane, int j, bool jok, Lane, Row&, Acc& acc) const {
    constexpr int SLOTS = 64 / LPS;
    const int slot = lane / LPS;
    const int jl = jok ? j : 0;
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
    for (int off = 0; off < n; off += 64) {
      const int cnt = n - off < 64 ? n - off : 64;
      const int t = b + (lane < cnt ? off + lane : 0);
      const int my_r = trow[t], my_e = tperm[t];
      const int my_ty = etype[my_e];
      const float my_val = values ? values[my_e] : 1.f;
      if constexpr (TYPED) {                           // one plane per entry: four entries in flight
        for (int i0 = 0; i0 < cnt; i0 += 4 * SLOTS) {
          float gv[4][VEC], val[4];
          bool in[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int src = i0 + SLOTS * u + slot;
            const int r = __shfl(my_r, src), ty = __shfl(my_ty, src);
            val[u] = __shfl(my_val, src);
            in[u] = (unsigned)ty < (unsigned)R;
            load_row<VEC>(g + (size_t)r * w + (size_t)(in[u] ? ty : 0) * k + jl, gv[u]);
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const bool ok = jok && in[u] && i0 + SLOTS * u + slot < cnt;
#pragma unroll
            for (int v = 0; v < VEC; ++v) acc[v] = ok ? __builtin_fmaf(val[u], gv[u][v], acc[v]) : acc[v];
          }
        }
      } else {                                         // an entry at a time per slot, four planes in flight
        for (int i0 = 0; i0 < cnt; i0 += SLOTS) {
          const int src = i0 + slot;
          const int r = __shfl(my_r, src), ty = __shfl(my_ty, src);
          const float val = __shfl(my_val, src);
          const bool in = (unsigned)ty < (unsigned)R;
          const bool ok = jok && in && src < cnt;
          const float* cp = coeff + (size_t)(in ? ty : 0) * B;
          const float* gp = g + (size_t)r * w + jl;
          for (int bb = 0; bb < B; bb += 4) {
            float gv[4][VEC], wq[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const int bq = bb + q < B ? bb + q : B - 1;
              load_row<VEC>(gp + (size_t)bq * k, gv[q]);
              wq[q] = cp[bq] * val;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {              // (b ascending)
              const bool okq = ok && bb + q < B;
#pragma unroll
              for (int v = 0; v < VEC; ++v) acc[v] = okq ? __builtin_fmaf(wq[q], gv[q][v], acc[v]) : acc[v];
            }
          }
        }
      }
    }
#pragma unroll
    for (int o = LPS; o < 64; o <<= 1) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] += __shfl_xor(acc[v], o);
    }
  }

  static __device__ __forceinline__ float partial(const Acc& acc, int, int v) { return acc[v]; }
  static __device__ __forceinline__ void merge_next(float& s, float o) { s += o; }
  __device__ __forceinline__ void store(int c, int j, const Acc& acc) const { store_row<VEC>(gx + (size_t)c * k + j, acc); }
  __device__ __forceinline__ void store_one(int c, int j, int, float v) const { gx[(size_t)c * k + j] = v; }
};

// ---- the gradient in coeff ---------------------------------------------------------------------------------------------------
struct RelCoeffArgs {
  const int *rrow, *rcol, *rperm;
  const float *g, *x, *values;
  float* gcoeff;
  int k;                                               // what the engine sees as the width: the planes of this pass
  int kx, B, b0;                                       // the columns of x; the planes of g; the first plane of this pass
  size_t w;                                            // B * kx, the row stride of g
};

template <int XV, int XL, int NB>                      // the wave's own shape over the columns of x: XV columns, XL lanes a slot
struct RelCoeffOp : RelCoeffArgs {
  static constexpr int VEC = 1, LPS = 64, NS = 1;      // to the engine: lane q carries plane q
  using Acc = float;
  using Partial = float;
  struct Lane {};
  struct Row {};
  __device__ __forceinline__ Lane lane_ctx(int, bool) const { return {}; }

  __device__ __forceinline__ void reduce(int, int b, int n, int lane, int, bool, Lane, Row&, float& mine) const {
    constexpr int SLOTS = 64 / XL;
    const int slot = lane / XL, l = lane % XL;
    float s[NB * XV];
#pragma unroll
    for (int v = 0; v < NB * XV; ++v) s[v] = 0.f;
    for (int off = 0; off < n; off += 64) {            // (n <= 0 for a chunk behind the last relation: nothing)
      const int cnt = n - off < 64 ? n - off : 64;
      const int t = b + (lane < cnt ? off + lane : 0);
      const int my_r = rrow[t], my_c = rcol[t];
      const float my_val = values ? values[rperm[t]] : 1.f;
      for (int i0 = 0; i0 < cnt; i0 += SLOTS) {
        const int src = i0 + slot;
        const int r = __shfl(my_r, src), c = __shfl(my_c, src);
        const float val = __shfl(my_val, src);
        const float* xp = x + (size_t)c * kx;
        const float* gp = g + (size_t)r * w + (size_t)b0 * kx;
        for (int j0 = 0; j0 < kx; j0 += XL * XV) {     // (tiles ascending)
          const int jj = j0 + l * XV;
          const bool ok = src < cnt && jj < kx;
          const int jl = ok ? jj : 0;
          float xv[XV], gv[NB][XV];
          load_row<XV>(xp + jl, xv);
#pragma unroll
          for (int q = 0; q < NB; ++q) load_row<XV>(gp + (size_t)(q < k ? q : 0) * kx + jl, gv[q]);
#pragma unroll
          for (int v = 0; v < XV; ++v) xv[v] = val * xv[v];
#pragma unroll
          for (int q = 0; q < NB; ++q) {
#pragma unroll
            for (int v = 0; v < XV; ++v) s[q * XV + v] = ok ? __builtin_fmaf(xv[v], gv[q][v], s[q * XV + v]) : s[q * XV + v];
          }
        }
      }
    }
    mine = 0.f;
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      float tot = s[q * XV];
#pragma unroll
      for (int v = 1; v < XV; ++v) tot += s[q * XV + v];
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) tot += __shfl_xor(tot, o);
      mine = lane == q ? tot : mine;
    }
  }

  static __device__ __forceinline__ float partial(const float& s, int, int) { return s; }
  static __device__ __forceinline__ void merge_next(float& s, float o) { s += o; }
  __device__ __forceinline__ void store(int t, int q, const float& s) const { gcoeff[(size_t)t * B + b0 + q] = s; }
  __device__ __forceinline__ void store_one(int t, int q, int, float v) const { gcoeff[(size_t)t * B + b0 + q] = v; }
};

// ---- the choices the host makes ----------------------------------------------------------------------------------------------
template <int N>
using Int = std::integral_constant<int, N>;

template <class F>
hipError_t with_planes(int nb, F f) {
  switch (nb) {
    case 1: return f(Int<1>{});
    case 2: return f(Int<2>{});
    case 4: return f(Int<4>{});
    default: return f(Int<8>{});
  }
}
template <class F>
hipError_t with_lanes(int units, F f) {                // spmm_heads' rule
  if (units <= 16) return f(Int<16>{});
  if (units <= 32) return f(Int<32>{});
  return f(Int<64>{});
}
template <class F>
hipError_t with_vec(bool wide, F f) { return wide ? f(Int<4>{}) : f(Int<1>{}); }

// the planes of a pass with `left` planes to go: 8, or the smallest of 1, 2, 4, 8 that covers them
int pass_planes(int left) { return left >= 8 ? 8 : left > 4 ? 8 : left > 2 ? 4 : left; }

}  // namespace

size_t relation_workspace_bytes(int nnz, int k, int B) {
  const size_t planes = pass_planes(B);                // (the engine keeps partials of all NB planes of a pass, stored or not)
  return 16 + 8 * planes * (size_t)k * (size_t)(((long long)nnz + kGatherChunk - 1) / kGatherChunk);
}

hipError_t launch_relation_aggregate(const int* rowptr, const int* col, const int* etype, int m, int nnz, const float* x, int k,
                                     const float* coeff, int R, int B, const float* values, float* out, void* ws, hipStream_t st) {
  const bool wide = k % 4 == 0 && aligned16(x) && aligned16(out);
  const bool cw = coeff && B % 4 == 0 && aligned16(coeff);
  for (int b0 = 0; b0 < B; b0 += kRelMaxPlanes) {
    const RelArgs a{col, etype, x, coeff, values, out, k, R, B, b0, cw, (size_t)B * k};
    const hipError_t e = with_planes(pass_planes(B - b0), [&](auto nb) {
      return with_vec(wide, [&](auto vec) {
        return with_lanes(k / vec, [&](auto lps) {
          constexpr int NB = decltype(nb)::value, VEC = decltype(vec)::value, LPS = decltype(lps)::value;
          if (coeff) return run_gather(RelForwardOp<VEC, LPS, NB, false>{a}, rowptr, m, nnz, ws, st);
          return run_gather(RelForwardOp<VEC, LPS, NB, true>{a}, rowptr, m, nnz, ws, st);
        });
      });
    });
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_relation_aggregate_backward_x(const int* trowptr, const int* trow, const int* tperm, const int* etype, int n,
                                                int nnz, const float* g, int k, const float* coeff, int R, int B,
                                                const float* values, float* gx, void* ws, hipStream_t st) {
  const RelBackXArgs a{trow, tperm, etype, g, coeff, values, gx, k, R, B, (size_t)B * k};
  const bool wide = k % 4 == 0 && aligned16(g) && aligned16(gx);
  return with_vec(wide, [&](auto vec) {
    return with_lanes(k / vec, [&](auto lps) {
      constexpr int VEC = decltype(vec)::value, LPS = decltype(lps)::value;
      if (coeff) return run_gather(RelBackXOp<VEC, LPS, false>{a}, trowptr, n, nnz, ws, st);
      return run_gather(RelBackXOp<VEC, LPS, true>{a}, trowptr, n, nnz, ws, st);
    });
  });
}

hipError_t launch_relation_aggregate_backward_coeff(const int* relptr, const int* rrow, const int* rcol, const int* rperm, int R,
                                                    int nnz, const float* g, const float* x, int k, int B, const float* values,
                                                    float* gcoeff, void* ws, hipStream_t st) {
  const bool wide = k % 4 == 0 && aligned16(g) && aligned16(x);
  for (int b0 = 0; b0 < B; b0 += kRelMaxPlanes) {
    const int nb = pass_planes(B - b0);
    const RelCoeffArgs a{rrow, rcol, rperm, g, x, values, gcoeff, B - b0 < nb ? B - b0 : nb, k, B, b0, (size_t)B * k};
    const hipError_t e = with_planes(nb, [&](auto planes) {
      return with_vec(wide, [&](auto vec) {
        return with_lanes(k / vec, [&](auto lps) {
          constexpr int NB = decltype(planes)::value, XV = decltype(vec)::value, XL = decltype(lps)::value;
          return run_gather(RelCoeffOp<XV, XL, NB>{a}, relptr, R, nnz, ws, st);
        });
      });
    });
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace gcn
