// aggregate_multi.hip — several statistics of every CSR row's neighbourhood from ONE gather per entry (PNA's aggregators,
// PyG's MultiAggregation, DGL's PNAConv), and the gradient of all of them in one walk of the transposed pattern.
//
//   forward   out[r, p k + j] = statistic p of { x[col[e], j] : e an entry of row r },  p in the caller's order, of
//             max, min (with argmax / argmin[r, j] = the entry), sum, mean, var (population), std = sqrt(var + eps)
//   backward  gx[c, j] = sum over the entries t of row c of the TRANSPOSED pattern (r = trow[t], e = tperm[t]) of
//             g_sum + g_mean / n_r + g_var 2 (x[c, j] - mean) / n_r + g_std (x[c, j] - mean) / (n_r std)
//             + g_max [argmax == e] + g_min [argmin == e],  every factor taken at [r, j]
//
// Plan-free like aggregate.hip: the caller's CSR in entry order, one 4-byte memset node and kernels (legal inside a stream
// capture), the host never reads a row length, no atomics — every output has one writer and every reduction a fixed
// order, so two calls give the same bits.  The wave and the dispatch by row length are aggregate.hip's (gather_rows.h): 4
// entry slots x 16 lanes x VEC columns, 64 indices per coalesced load handed out by __shfl, four gathers a slot in flight,
// VEC = 4 when every operand is 16-byte aligned and k % 4 == 0, else 1; 8 rows a wave, rows of more than kAggChunk entries
// by chunk partials merged in chunk order.  What is new is the state a lane keeps per column, and its rules:
//
//   S0 = sum of x                          -> sum, mean = S0 / n_r
//   K  = x[col[rowptr[r]], j], the row's FIRST entry, fetched once per row by every lane (a long row's segments too: the
//        op carries rowptr); d = x - K; S1 = sum of d, S2 = sum of d * d (fmaf)
//                                          -> var = (S2 - S1 S1 / n_r) / n_r, clamped by `var < 0 ? 0 : var` (a NaN passes)
//   (max value, entry), (min value, entry) -> select_rule.h: first among equals, a NaN wins, the winner's bits
//
// Every slot and every chunk partial of a row shifts by the same K, so merging two states is adding their sums: nothing
// like Welford's pairwise update (a division per merge, and a result that depends on how the row was split), and none of
// the cancellation of sum(x^2) - sum(x)^2 / n, whose error is relative to x^2 rather than to the spread of the row.  A row
// of one entry, or of equal entries, has d == 0 exactly and var == 0 exactly.  A non-finite entry makes S1 or S2 non-finite
// and var a NaN, as fp64 numpy's.  A long row's partial is the whole state of one column (32 bytes), so the engine's
// merge_next needs no plane index: NS = 1.
//
// The moments and the extrema are each compiled in or out (var / std requested or not, max / min requested or not): four
// kernels per VEC, not one per subset of planes.  Which planes are stored, and where, is a run-time table in the kernel
// argument.
//
// The backward's moment part is affine in x[c, j]: sum_t a[r, j] + x[c, j] sum_t b[r, j].  An element-wise prepass over
// [m, k] writes a | b side by side as [m, 2 k] (one entry's two rows are adjacent lines), and a second op on the engine
// gathers a | b (and g_max, argmax, g_min, argmin where those planes exist) per entry of the transposed pattern and
// stores sum a + x[c, j] sum b + selected.  Nothing of size nnz x k is formed.  Contraction is off: every operation
// written here is rounded once, fmaf where it says fmaf.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <initializer_list>

#include "aggregate_multi.h"
#include "gather_rows.h"
#include "select_rule.h"
#include "spmm_kernels.h"

#pragma clang fp contract(off)

namespace gcn {
namespace {

template <int VEC>
__device__ __forceinline__ void load_ints(const int* p, int (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const int4 q = *reinterpret_cast<const int4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    static_assert(VEC == 1);
    v[0] = p[0];
  }
}
template <int VEC>
__device__ __forceinline__ void store_ints(int* p, const int (&v)[VEC]) {
  if constexpr (VEC == 4) {
    *reinterpret_cast<int4*>(p) = make_int4(v[0], v[1], v[2], v[3]);
  } else {
    static_assert(VEC == 1);
    p[0] = v[0];
  }
}

// ---- the forward ---------------------------------------------------------------------------------------------------------
struct MultiArgs {
  const int *rowptr, *col;
  const float* x;
  float* out;
  int *argmax, *argmin;
  float* save_mean;
  int k;
  MultiPlanes pl;
  float eps;
};

// one column's whole state: what a lane keeps (VEC of them), and a long row's partial in the workspace
struct alignas(16) ColState {
  float s0, s1, s2;                                    // sum of x; sums of d and d * d, d = x - K
  float hi;
  int hie;                                             // (max value, entry), kNone before the first
  float lo;
  int loe;
  int pad;
};
static_assert(sizeof(ColState) == 32, "GCN_AGGREGATE_MULTI_WS_BYTES");

// the six statistics of a row of nr entries from its merged state (an empty row: zeros and -1)
__device__ __forceinline__ void finish(const ColState& c, int nr, float eps, float (&val)[kMultiStats], int& amax, int& amin) {
  const bool has = nr > 0;
  const float fn = (float)nr;
  float var = has ? (c.s2 - c.s1 * c.s1 / fn) / fn : 0.f;
  var = var < 0.f ? 0.f : var;                         // (a NaN is not < 0: it stays)
  val[kMultiMax] = c.hie == kNone ? 0.f : c.hi;
  val[kMultiMin] = c.loe == kNone ? 0.f : c.lo;
  val[kMultiSum] = has ? c.s0 : 0.f;
  val[kMultiMean] = has ? c.s0 / fn : 0.f;
  val[kMultiVar] = var;
  val[kMultiStd] = has ? sqrtf(var + eps) : 0.f;
  amax = c.hie == kNone ? -1 : c.hie;
  amin = c.loe == kNone ? -1 : c.loe;
}

template <int VEC_, bool MOM, bool SEL>
struct MultiOp : MultiArgs {
  static constexpr int VEC = VEC_, LPS = 16, NS = 1;
  struct Acc { float s0[VEC], s1[VEC], s2[VEC], hi[VEC], lo[VEC]; int hie[VEC], loe[VEC]; };
  using Partial = ColState;
  struct Lane {};
  struct Row {};
  __device__ __forceinline__ Lane lane_ctx(int, bool) const { return {}; }

  __device__ __forceinline__ void reduce(int r, int b, int n, int lane, int j, bool jok, Lane, Row&, Acc& s) const {
    const int slot = lane >> 4;
    const int jl = jok ? j : 0;                        // (lanes past k gather column 0 and keep nothing)
    float shift[VEC];                                  // K: the first entry of the ROW (b may be a later segment's start)
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      s.s0[v] = s.s1[v] = s.s2[v] = s.hi[v] = s.lo[v] = shift[v] = 0.f;
      s.hie[v] = s.loe[v] = kNone;
    }
    if (MOM && n > 0) load_row<VEC>(x + (size_t)col[rowptr[r]] * k + jl, shift);      // (n > 0: the row has a first entry)
    for (int off = 0; off < n; off += 64) {            // (n <= kAggChunk: no overflow)
      const int cnt = n - off < 64 ? n - off : 64;
      const int mine = col[b + (lane < cnt ? off + lane : 0)];                         // (past the end: the first entry again)
      for (int i0 = 0; i0 < cnt; i0 += 16) {
        float it[4][VEC];
#pragma unroll
        for (int u = 0; u < 4; ++u) load_row<VEC>(x + (size_t)__shfl(mine, i0 + 4 * u + slot) * k + jl, it[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) {                  // (slot s takes entries s, s + 4, ...: ascending inside a lane)
          const int i = i0 + 4 * u + slot;
          const bool ok = jok && i < cnt;
          const int t = b + off + i;
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            const float xv = it[u][v];
            s.s0[v] = ok ? s.s0[v] + xv : s.s0[v];
            if constexpr (MOM) {
              const float d = xv - shift[v];
              s.s1[v] = ok ? s.s1[v] + d : s.s1[v];
              s.s2[v] = ok ? fmaf(d, d, s.s2[v]) : s.s2[v];
            }
            if constexpr (SEL) {
              select_fold<true>(s.hi[v], s.hie[v], xv, t, ok);
              select_fold<false>(s.lo[v], s.loe[v], xv, t, ok);
            }
          }
        }
      }
    }
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {               // the four slots hold disjoint entries of the same columns
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        s.s0[v] += __shfl_xor(s.s0[v], o);
        if constexpr (MOM) {
          s.s1[v] += __shfl_xor(s.s1[v], o);
          s.s2[v] += __shfl_xor(s.s2[v], o);
        }
        if constexpr (SEL) {
          const float ohi = __shfl_xor(s.hi[v], o), olo = __shfl_xor(s.lo[v], o);
          const int ohie = __shfl_xor(s.hie[v], o), oloe = __shfl_xor(s.loe[v], o);
          select_merge<true>(s.hi[v], s.hie[v], ohi, ohie);
          select_merge<false>(s.lo[v], s.loe[v], olo, oloe);
        }
      }
    }
  }

  static __device__ __forceinline__ ColState partial(const Acc& s, int, int v) {
    return ColState{s.s0[v], s.s1[v], s.s2[v], s.hi[v], s.hie[v], s.lo[v], s.loe[v], 0};
  }
  // a partial of LATER entries: the same K, so the sums add; the extrema by the rule
  static __device__ __forceinline__ void merge_next(ColState& s, const ColState& o) {
    s.s0 += o.s0;
    s.s1 += o.s1;
    s.s2 += o.s2;
    select_merge<true>(s.hi, s.hie, o.hi, o.hie);
    select_merge<false>(s.lo, s.loe, o.lo, o.loe);
  }

  __device__ __forceinline__ void store(int r, int j, const Acc& s) const {            // columns j .. j + VEC of row r
    const int nr = rowptr[r + 1] - rowptr[r];
    float val[kMultiStats][VEC];
    int amax[VEC], amin[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      float one[kMultiStats];
      finish(partial(s, 0, v), nr, eps, one, amax[v], amin[v]);
#pragma unroll
      for (int q = 0; q < kMultiStats; ++q) val[q][v] = one[q];
    }
    float* row = out + (size_t)r * pl.nred * k + j;
#pragma unroll
    for (int q = 0; q < kMultiStats; ++q)
      if (pl.at[q] >= 0) store_row<VEC>(row + (size_t)pl.at[q] * k, val[q]);
    const size_t at = (size_t)r * k + j;
    if (pl.at[kMultiMax] >= 0) store_ints<VEC>(argmax + at, amax);
    if (pl.at[kMultiMin] >= 0) store_ints<VEC>(argmin + at, amin);
    if (save_mean) store_row<VEC>(save_mean + at, val[kMultiMean]);
  }
  __device__ __forceinline__ void store_one(int r, int j, int, const ColState& c) const {   // column j of a long row
    float val[kMultiStats];
    int amax, amin;
    finish(c, rowptr[r + 1] - rowptr[r], eps, val, amax, amin);
    float* row = out + (size_t)r * pl.nred * k + j;
#pragma unroll
    for (int q = 0; q < kMultiStats; ++q)
      if (pl.at[q] >= 0) row[(size_t)pl.at[q] * k] = val[q];
    const size_t at = (size_t)r * k + j;
    if (pl.at[kMultiMax] >= 0) argmax[at] = amax;
    if (pl.at[kMultiMin] >= 0) argmin[at] = amin;
    if (save_mean) save_mean[at] = val[kMultiMean];
  }
};

template <int VEC>
hipError_t run_forward(const MultiArgs& a, int m, int nnz, void* ws, hipStream_t st) {
  const bool mom = a.pl.moments(), sel = a.pl.extrema();
  if (mom && sel) return run_gather(MultiOp<VEC, true, true>{a}, a.rowptr, m, nnz, ws, st);
  if (mom) return run_gather(MultiOp<VEC, true, false>{a}, a.rowptr, m, nnz, ws, st);
  if (sel) return run_gather(MultiOp<VEC, false, true>{a}, a.rowptr, m, nnz, ws, st);
  return run_gather(MultiOp<VEC, false, false>{a}, a.rowptr, m, nnz, ws, st);
}

// ---- the backward -----------------------------------------------------------------------------------------------------------
// a[r, j] | b[r, j] of the affine part  sum_t a + x[c, j] sum_t b:  with i = 1 / n_r, cv = 2 i g_var and cs = i g_std / std,
// a = g_sum + i g_mean - (cv + cs) mean,  b = cv + cs.  An empty row has no entry to read them: zeros.
__global__ void __launch_bounds__(256) multi_prepass_kernel(const int* __restrict__ rowptr, size_t elems, int k, MultiPlanes pl,
                                                            const float* __restrict__ g, const float* __restrict__ out,
                                                            const float* __restrict__ mean, size_t mean_stride,
                                                            float* __restrict__ ab) {
  const size_t w = (size_t)pl.nred * k;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < elems; i += (size_t)gridDim.x * 256) {
    const size_t r = i / k;
    const int j = (int)(i - r * k);
    const int nr = rowptr[r + 1] - rowptr[r];
    float a = 0.f, b = 0.f;
    if (nr > 0) {
      const float inv = 1.f / (float)nr;
      const float* gr = g + r * w + j;
      if (pl.at[kMultiSum] >= 0) a += gr[(size_t)pl.at[kMultiSum] * k];
      if (pl.at[kMultiMean] >= 0) a += gr[(size_t)pl.at[kMultiMean] * k] * inv;
      if (pl.at[kMultiVar] >= 0) b += 2.f * inv * gr[(size_t)pl.at[kMultiVar] * k];
      if (pl.at[kMultiStd] >= 0) b += inv * gr[(size_t)pl.at[kMultiStd] * k] / out[r * w + (size_t)pl.at[kMultiStd] * k + j];
      if (pl.at[kMultiVar] >= 0 || pl.at[kMultiStd] >= 0) a -= b * mean[r * mean_stride + j];
    }
    ab[r * 2 * k + j] = a;
    ab[r * 2 * k + k + j] = b;
  }
}

struct BackArgs {
  const int *trow, *tperm;
  const float *ab, *g, *x;                             // [m, 2 k] or null; [m, nred k]; [n, k]
  const int *argmax, *argmin;                          // [m, k] or null
  float* gx;
  int k, gmax_at, gmin_at;                             // the columns of g where the max / min plane starts, -1 = none
  size_t w;                                            // nred * k
};

struct alignas(16) BackState { float a, b, sel, pad; };

// sum a + x sum b.  A zero sum b takes nothing of x: a row nobody lists, or planes whose gradient does not depend on x
// (sum, mean), give the same result for a non-finite x.
__device__ __forceinline__ float affine(float x, float a, float b) { return b == 0.f ? a : fmaf(x, b, a); }

template <int VEC_, bool AFF, bool SEL>
struct MultiBackOp : BackArgs {
  static constexpr int VEC = VEC_, LPS = 16, NS = 1;
  struct Acc { float a[VEC], b[VEC], sel[VEC], own[VEC]; };
  using Partial = BackState;
  struct Lane {};
  struct Row {};
  struct Item { float a[VEC], b[VEC], ghi[VEC], glo[VEC]; int ahi[VEC], alo[VEC]; };
  __device__ __forceinline__ Lane lane_ctx(int, bool) const { return {}; }

  __device__ __forceinline__ Item fetch(int r, int jl) const {
    Item it;
    if constexpr (AFF) {
      const float* p = ab + (size_t)r * 2 * k + jl;
      load_row<VEC>(p, it.a);
      load_row<VEC>(p + k, it.b);
    }
    if constexpr (SEL) {
      const size_t at = (size_t)r * k + jl;
      if (gmax_at >= 0) {
        load_row<VEC>(g + (size_t)r * w + gmax_at + jl, it.ghi);
        load_ints<VEC>(argmax + at, it.ahi);
      }
      if (gmin_at >= 0) {
        load_row<VEC>(g + (size_t)r * w + gmin_at + jl, it.glo);
        load_ints<VEC>(argmin + at, it.alo);
      }
    }
    return it;
  }

  __device__ __forceinline__ void reduce(int c, int b, int n, int lane, int j, bool jok, Lane, Row&, Acc& s) const {
    const int slot = lane >> 4;
    const int jl = jok ? j : 0;                        // (lanes past k gather column 0 and keep nothing)
#pragma unroll
    for (int v = 0; v < VEC; ++v) s.a[v] = s.b[v] = s.sel[v] = 0.f;
    load_row<VEC>(x + (size_t)c * k + jl, s.own);      // the walked row's own features, once
    for (int off = 0; off < n; off += 64) {            // (n <= kAggChunk: no overflow)
      const int cnt = n - off < 64 ? n - off : 64;
      const int t = b + (lane < cnt ? off + lane : 0); // (past the end: the first entry again)
      const int my_r = trow[t], my_e = tperm[t];
      for (int i0 = 0; i0 < cnt; i0 += 16) {
        Item it[4];
        int e[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          e[u] = __shfl(my_e, i0 + 4 * u + slot);
          it[u] = fetch(__shfl(my_r, i0 + 4 * u + slot), jl);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const bool ok = jok && i0 + 4 * u + slot < cnt;
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            if constexpr (AFF) {
              s.a[v] = ok ? s.a[v] + it[u].a[v] : s.a[v];
              s.b[v] = ok ? s.b[v] + it[u].b[v] : s.b[v];
            }
            if constexpr (SEL) {                       // (a selection, not a product: an unselected NaN stays out)
              if (gmax_at >= 0) s.sel[v] = ok && it[u].ahi[v] == e[u] ? s.sel[v] + it[u].ghi[v] : s.sel[v];
              if (gmin_at >= 0) s.sel[v] = ok && it[u].alo[v] == e[u] ? s.sel[v] + it[u].glo[v] : s.sel[v];
            }
          }
        }
      }
    }
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        if constexpr (AFF) {
          s.a[v] += __shfl_xor(s.a[v], o);
          s.b[v] += __shfl_xor(s.b[v], o);
        }
        if constexpr (SEL) s.sel[v] += __shfl_xor(s.sel[v], o);
      }
    }
  }
  static __device__ __forceinline__ BackState partial(const Acc& s, int, int v) { return BackState{s.a[v], s.b[v], s.sel[v], 0.f}; }
  static __device__ __forceinline__ void merge_next(BackState& s, const BackState& o) {
    s.a += o.a;
    s.b += o.b;
    s.sel += o.sel;
  }
  __device__ __forceinline__ void store(int c, int j, const Acc& s) const {
    float v[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] = affine(s.own[i], s.a[i], s.b[i]) + s.sel[i];
    store_row<VEC>(gx + (size_t)c * k + j, v);
  }
  __device__ __forceinline__ void store_one(int c, int j, int, const BackState& p) const {
    const size_t at = (size_t)c * k + j;
    gx[at] = affine(x[at], p.a, p.b) + p.sel;
  }
};

template <int VEC>
hipError_t run_backward(const BackArgs& a, bool aff, bool sel, const int* trowptr, int n, int nnz, void* ws, hipStream_t st) {
  if (aff && sel) return run_gather(MultiBackOp<VEC, true, true>{a}, trowptr, n, nnz, ws, st);
  if (aff) return run_gather(MultiBackOp<VEC, true, false>{a}, trowptr, n, nnz, ws, st);
  return run_gather(MultiBackOp<VEC, false, true>{a}, trowptr, n, nnz, ws, st);
}

__global__ void __launch_bounds__(256) fill_words_kernel(unsigned* __restrict__ p, size_t count, unsigned word) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) p[i] = word;
}

unsigned blocks_for(size_t elems) {                    // a grid-stride loop: enough blocks to fill the chip, no more
  const size_t want = (elems + 255) / 256;
  return (unsigned)(want < 65536 ? want : 65536);
}

bool all_aligned16(std::initializer_list<const void*> ps) {
  for (const void* p : ps)
    if (p && !aligned16(p)) return false;
  return true;
}

}  // namespace

size_t aggregate_multi_workspace_bytes(int nnz, int k) {
  return 16 + 2 * sizeof(ColState) * (size_t)k * (size_t)(((long long)nnz + kGatherChunk - 1) / kGatherChunk);
}

hipError_t launch_fill_words(void* p, size_t count, unsigned word, hipStream_t st) {
  fill_words_kernel<<<blocks_for(count), 256, 0, st>>>(static_cast<unsigned*>(p), count, word);
  return hipGetLastError();
}

hipError_t launch_aggregate_multi_empty(int m, int k, MultiPlanes pl, float* out, int* argmax, int* argmin, float* save_mean,
                                        hipStream_t st) {
  const size_t elems = (size_t)m * (size_t)k;
  if (hipError_t e = launch_fill_words(out, elems * pl.nred, 0u, st); e != hipSuccess) return e;
  if (pl.has(kMultiMax))
    if (hipError_t e = launch_fill_words(argmax, elems, 0xffffffffu, st); e != hipSuccess) return e;
  if (pl.has(kMultiMin))
    if (hipError_t e = launch_fill_words(argmin, elems, 0xffffffffu, st); e != hipSuccess) return e;
  return save_mean ? launch_fill_words(save_mean, elems, 0u, st) : hipSuccess;
}

// the 16-byte paths need every gathered or stored row to start on a 16-byte boundary: the base pointers and the row
// strides k, nred k and 2 k floats; anything else takes one element per lane
hipError_t launch_aggregate_multi(const int* rowptr, const int* col, int m, int nnz, const float* x, int k, MultiPlanes pl, float eps,
                                  float* out, int* argmax, int* argmin, float* save_mean, void* ws, hipStream_t st) {
  if (!pl.has(kMultiMax)) argmax = nullptr;
  if (!pl.has(kMultiMin)) argmin = nullptr;
  const MultiArgs a{rowptr, col, x, out, argmax, argmin, save_mean, k, pl, eps};
  const bool wide = k % 4 == 0 && all_aligned16({x, out, argmax, argmin, save_mean});
  return wide ? run_forward<4>(a, m, nnz, ws, st) : run_forward<1>(a, m, nnz, ws, st);
}

hipError_t launch_aggregate_multi_backward(const int* trowptr, const int* trow, const int* tperm, const int* rowptr, int n, int m,
                                           int nnz, const float* g, const float* x, int k, MultiPlanes pl, const float* out,
                                           const int* argmax, const int* argmin, const float* save_mean, float* ab, float* gx,
                                           void* ws, hipStream_t st) {
  const bool aff = pl.affine(), sel = pl.extrema();
  if (aff) {
    const bool own_plane = pl.has(kMultiMean);         // the mean: a plane of out, or the buffer the forward filled beside it
    const float* mean = own_plane ? out + (size_t)pl.at[kMultiMean] * k : save_mean;
    const size_t elems = (size_t)m * (size_t)k;
    multi_prepass_kernel<<<blocks_for(elems), 256, 0, st>>>(rowptr, elems, k, pl, g, out, mean,
                                                            own_plane ? (size_t)pl.nred * k : (size_t)k, ab);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  } else {
    ab = nullptr;
  }
  if (!pl.has(kMultiMax)) argmax = nullptr;
  if (!pl.has(kMultiMin)) argmin = nullptr;
  const BackArgs a{trow, tperm, ab, g, x, argmax, argmin, gx, k, pl.has(kMultiMax) ? pl.at[kMultiMax] * k : -1,
                   pl.has(kMultiMin) ? pl.at[kMultiMin] * k : -1, (size_t)pl.nred * k};
  const bool wide = k % 4 == 0 && all_aligned16({ab, g, x, argmax, argmin, gx});
  return wide ? run_backward<4>(a, aff, sel, trowptr, n, nnz, ws, st) : run_backward<1>(a, aff, sel, trowptr, n, nnz, ws, st);
}

}  // namespace gcn
