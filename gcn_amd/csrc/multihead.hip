// multihead.hip — the gather primitives of multi-head attention, H heads in one pass over the adjacency: the head-weighted
// SpMM and the per-head SDDMM.  (The per-head edge softmax family and the row sums of an [nnz, H] array are the H-head
// layout of edge_softmax.hip.)  Plan-free like edge_softmax.hip and aggregate.hip, whose kernels these follow: the caller's
// CSR in entry order, one 4-byte memset node and kernels (legal inside a stream capture), the host never reads a row
// length, no atomics — every output has one writer and every sum a fixed order, so two calls give the same bits.
//
// Layouts: node arrays [rows, k] with k = H * F, head h owns columns hF .. hF + F - 1; per-entry arrays [nnz, H], an
// entry's heads contiguous.  nnz * H < 2^31 (checked by the C ABI), so an element index of a per-entry array is an int.
//
// 1. spmm_heads ("gather a row per entry", aggregate.hip's wave): SLOTS entry slots x LPS lanes x VEC columns with
//    LPS = 16, 32 or 64 lanes for k / VEC <= 16, <= 32, more — so up to 256 columns the adjacency is walked once for all
//    heads and a gather brings the whole k-wide row; wider k tiles 256 columns over blockIdx.y.  VEC = 4 (one 16-byte load;
//    F % 4 == 0 keeps a lane's four columns in one head) or 1 (an operand that is not 16-byte aligned, or F % 4 != 0).  The
//    wave loads 64 indices (and permutation entries) with one coalesced load each and hands them out with ds_bpermute; each
//    slot has 4 gathers and their 4 one-word value loads vals[e * H + head] in flight before the first fma.  The
//    dispatch by row length is gather_rows.h's: 8 rows a wave, rows of more than kAggChunk entries by chunk partials
//    per (chunk, row, column), merged in chunk order by the wave whose chunk holds the row's first entry.
//    Fixed order: slot s adds the entries s, s + SLOTS, ... in ascending order (fma), the slots are merged by the xor
//    butterfly LPS .. 32, chunk partials in chunk order.
//
// 2. sddmm_heads: a wave takes a row at a time (8 rows a wave, long rows by chunks of kAggChunk entries on a fixed grid of
//    waves: no partials, an entry's result has one writer).  A head's F columns are U = F / VEC units; P = min(4, the
//    largest power of two dividing U) lanes share an (entry, head), lane p taking the units p, p + P, ...  With H a power
//    of two <= 16 an entry is H * P <= 64 adjacent lanes and a wave step takes 64 / (H P) entries, four steps in flight;
//    any other H puts an entry on a lane, which walks the heads one after the other (the slow route).
//    Fixed order of an (entry, head) sum, a function of F and VEC only — not of the row, the chunk, the slot or H:
//    s_p = fma chain over the units p, p + P, ... in ascending order, a unit's elements in ascending order; then
//    P = 2: s0 + s1, P = 4: (s0 + s2) + (s1 + s3).
//
// 3. gatv2_scores: the walk of 2 with another per-element op — s[e, h] = sum_j att[h, j] leaky_relu(a[row(e), hF + j] +
//    b[col[e], hF + j]): t = a + b; t = t > 0 ? t : slope * t; acc = fma(att[j], t, acc) — so the same routes and the same
//    fixed order of an (entry, head) sum as sddmm_heads; att [H, F] is read with the unit's 16-byte (or one-word) load.
//    Its backward is the walk of 1 with another per-element op, run once on the pattern and once on its transpose: with
//    t = own[r, j] + other[idx[e], j] and D = t > 0 ? 1 : slope (the slope at 0) a lane keeps
//    mask[j] += g[e, h] * D and, where asked for, act[j] += g[e, h] * (t * D); grad_own[r, j] = att[j] * mask[j], multiplied
//    once after the merge, act_sums[r, j] = act[j] (grad_att is its column sums).  Long rows keep chunk partials of both
//    sums (the second set behind the first).  Fixed order, as in 1: slot s adds the entries s, s + SLOTS, ... in ascending
//    order (fma), the slots are merged by the xor butterfly LPS .. 32, chunk partials in chunk order.  An empty row
//    writes zeros.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gather_rows.h"
#include "spmm_kernels.h"

namespace gcn {
namespace {

constexpr int kMaxFastHeads = 16;

struct HeadsSpmmArgs {
  const int *idx, *perm;
  const float *vals, *x;
  float* out;
  int H, F, k;
};

// The per-element op of the row walk.  A lane keeps NS running sums for its VEC columns of a row, sum q in acc[q VEC ..],
// and in Row what begin() fetched of the row itself; a gathered element x of an entry with value w adds
// fma(w, term(q, row, v, x), .) to sum q; store() is what the merged sums of a row become (store_one: one element, for the
// long rows).  The fma stays in the walk: an op that did the accumulation itself cost the existing kernels registers.
// spmm_heads: out[r, j] = sum of w * x[j].
struct WeightedSumOp {
  static constexpr int NS = 1;
  template <int VEC>
  struct Row {};
  template <int VEC>
  __device__ __forceinline__ void begin(const HeadsSpmmArgs&, int, int, Row<VEC>&) const {}
  template <int VEC>
  __device__ __forceinline__ float term(int, const Row<VEC>&, int, float x) const { return x; }
  template <int VEC>
  __device__ __forceinline__ void store(const HeadsSpmmArgs& a, int r, int j, const float (&acc)[VEC]) const {
    store_row<VEC>(a.out + (size_t)r * a.k + j, acc);
  }
  __device__ __forceinline__ void store_one(const HeadsSpmmArgs& a, int r, int j, int, float v) const { a.out[(size_t)r * a.k + j] = v; }
};

// the backward of gatv2_scores on one side (a.vals = g, a.x = the gathered side, a.out = grad_own): with t = own + x and
// D = t > 0 ? 1 : slope, sum 0 (mask) takes w * D and, with ACT, sum 1 (act) takes w * (t * D); grad_own = att * mask,
// act_sums = act
template <bool ACT>
struct Gatv2BackwardOp {
  static constexpr int NS = ACT ? 2 : 1;
  const float *own, *att;
  float* act_sums;
  float slope;
  template <int VEC>
  struct Row {
    float own[VEC];
  };
  template <int VEC>
  __device__ __forceinline__ void begin(const HeadsSpmmArgs& a, int r, int jl, Row<VEC>& row) const {
    load_row<VEC>(own + (size_t)r * a.k + jl, row.own);
  }
  template <int VEC>
  __device__ __forceinline__ float term(int q, const Row<VEC>& row, int v, float x) const {
    const float t = row.own[v] + x;
    const float d = t > 0.f ? 1.f : slope;
    return q == 0 ? d : t * d;
  }
  template <int VEC>
  __device__ __forceinline__ void store(const HeadsSpmmArgs& a, int r, int j, const float (&acc)[NS * VEC]) const {
    float w[VEC], gr[VEC], ac[VEC];
    load_row<VEC>(att + j, w);
#pragma unroll
    for (int v = 0; v < VEC; ++v) gr[v] = w[v] * acc[v];
    store_row<VEC>(a.out + (size_t)r * a.k + j, gr);
    if constexpr (ACT) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) ac[v] = acc[VEC + v];
      store_row<VEC>(act_sums + (size_t)r * a.k + j, ac);
    }
  }
  __device__ __forceinline__ void store_one(const HeadsSpmmArgs& a, int r, int j, int q, float v) const {
    if (q == 0) a.out[(size_t)r * a.k + j] = att[j] * v;
    else act_sums[(size_t)r * a.k + j] = v;
  }
};

// entries [b, b + n) of one row (n <= kGatherChunk) on a wave; the lane's columns are j .. j + VEC of head `head` (jok: they exist)
template <int VEC, int LPS, class Op>
__device__ __forceinline__ void spmm_walk(const HeadsSpmmArgs& a, const Op& op, int b, int n, int lane, int j, bool jok, int head,
                                          const typename Op::template Row<VEC>& row, float (&acc)[Op::NS * VEC]) {
  constexpr int SLOTS = 64 / LPS, BATCH = 4 * SLOTS;
  const int slot = lane / LPS;
  const int jl = jok ? j : 0, hl = jok ? head : 0;     // (lanes past k gather column 0 and add nothing)
  for (int off = 0; off < n; off += 64) {
    const int cnt = n - off < 64 ? n - off : 64;
    const int t = b + (lane < cnt ? off + lane : 0);   // (past the end: the first entry again, a legal address)
    const int my_ix = a.idx[t];
    const int my_ve = a.perm ? a.perm[t] : t;
    for (int i0 = 0; i0 < cnt; i0 += BATCH) {
      float xv[4][VEC], w[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int src = i0 + SLOTS * u + slot;         // (< 64: BATCH divides 64)
        const int ix = __shfl(my_ix, src), ve = __shfl(my_ve, src);
        load_row<VEC>(a.x + (size_t)ix * a.k + jl, xv[u]);
        w[u] = a.vals[ve * a.H + hl];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {                    // (slot s takes entries s, s + SLOTS, ...: ascending inside a lane)
        const bool ok = jok && i0 + SLOTS * u + slot < cnt;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
#pragma unroll
          for (int q = 0; q < Op::NS; ++q)
            acc[q * VEC + v] = ok ? __builtin_fmaf(w[u], op.term(q, row, v, xv[u][v]), acc[q * VEC + v]) : acc[q * VEC + v];
        }
      }
    }
  }
}

template <int VEC, int LPS>
__device__ __forceinline__ void merge_slots(float (&acc)[VEC]) {
#pragma unroll
  for (int o = LPS; o < 64; o <<= 1) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] += __shfl_xor(acc[v], o);
  }
}

// what gather_rows.h asks of a walk, over the args and the per-element op E: Acc stays the bare array of the walk, and the
// head of a lane's columns (the one division) is found once a kernel
template <int VEC_, int LPS_, class E>
struct HeadsRowsOp : HeadsSpmmArgs {
  static constexpr int VEC = VEC_, LPS = LPS_, NS = E::NS;
  E e;
  using Acc = float[NS * VEC];
  using Partial = float;
  using Lane = int;
  using Row = typename E::template Row<VEC>;
  __device__ __forceinline__ int lane_ctx(int j, bool jok) const { return jok ? j / F : 0; }
  __device__ __forceinline__ void reduce(int r, int b, int n, int lane, int j, bool jok, int head, Row& row, Acc& acc) const {
#pragma unroll
    for (int v = 0; v < NS * VEC; ++v) acc[v] = 0.f;
    e.begin(*this, r, jok ? j : 0, row);
    spmm_walk<VEC, LPS>(*this, e, b, n, lane, j, jok, head, row, acc);
    merge_slots<NS * VEC, LPS>(acc);
  }
  __device__ __forceinline__ void store(int r, int j, const Acc& acc) const { e.template store<VEC>(*this, r, j, acc); }
  static __device__ __forceinline__ float partial(const Acc& acc, int t, int v) { return acc[t * VEC + v]; }
  static __device__ __forceinline__ void merge_next(float& s, float o) { s += o; }
  __device__ __forceinline__ void store_one(int r, int j, int t, float v) const { e.store_one(*this, r, j, t, v); }
};

template <int VEC, int LPS, class E>
hipError_t run_spmm(const HeadsSpmmArgs& a, const E& op, const int* rowptr, int rows, int nnz, void* ws, hipStream_t st) {
  return run_gather(HeadsRowsOp<VEC, LPS, E>{a, op}, rowptr, rows, nnz, ws, st);
}

template <int VEC, class Op>
hipError_t run_spmm_vec(const HeadsSpmmArgs& a, const Op& op, const int* rowptr, int rows, int nnz, void* ws, hipStream_t st) {
  const int units = a.k / VEC;
  if (units <= 16) return run_spmm<VEC, 16>(a, op, rowptr, rows, nnz, ws, st);
  if (units <= 32) return run_spmm<VEC, 32>(a, op, rowptr, rows, nnz, ws, st);
  return run_spmm<VEC, 64>(a, op, rowptr, rows, nnz, ws, st);
}

// ---- SDDMM -----------------------------------------------------------------------------------------------------------------------
struct SddmmHeadsArgs {
  const int* col;
  const float *a, *b;
  float* out;
  int H, F, k;
  int hshift;                                          // log2 H on the fast route, -1 on the slow one
  int pshift;                                          // log2 P: P lanes share an (entry, head) on the fast route
  int nu;                                              // F / VEC units per head
};

// The per-element op of the entry walk: acc' = elem(w, a, b, acc) over a head's columns, w what weights() brings for the unit
// at node column jj.  sddmm_heads: the dot product, acc' = fma(a, b, acc).
struct DotOp {
  template <int VEC>
  __device__ __forceinline__ void weights(int, float (&w)[VEC]) const {
#pragma unroll
    for (int v = 0; v < VEC; ++v) w[v] = 0.f;
  }
  __device__ __forceinline__ float elem(float, float a, float b, float acc) const { return __builtin_fmaf(a, b, acc); }
};

// gatv2_scores: acc' = fma(att[jj], leaky_relu(a + b), acc); att [H, F] row-major, so its flat index is the node column
struct Gatv2ScoreOp {
  const float* att;
  float slope;
  template <int VEC>
  __device__ __forceinline__ void weights(int jj, float (&w)[VEC]) const {
    load_row<VEC>(att + jj, w);
  }
  __device__ __forceinline__ float elem(float w, float a, float b, float acc) const {
    float t = a + b;
    t = t > 0.f ? t : slope * t;
    return __builtin_fmaf(w, t, acc);
  }
};

// the merge of the P partial sums of an (entry, head): the butterfly's order, P = 2: s0 + s1, P = 4: (s0 + s2) + (s1 + s3)
__device__ __forceinline__ float merge_parts(float s, int pshift) {
  if (pshift == 2) s += __shfl_xor(s, 2);
  if (pshift >= 1) s += __shfl_xor(s, 1);
  return s;
}

// entries [b0, b0 + n) of row r (0 < n <= kGatherChunk) on a wave
template <int VEC, class Op>
__device__ __forceinline__ void sddmm_entries(const SddmmHeadsArgs& s, const Op& op, int r, int b0, int n, int lane) {
  const float* arow = s.a + (size_t)r * s.k;
  if (s.hshift >= 0) {                                 // fast route: H P adjacent lanes an entry, 64 / (H P) entries a step
    const int gshift = s.hshift + s.pshift;            // (H P <= 64)
    const int epw = 64 >> gshift;
    const int sub = lane >> gshift, head = (lane >> s.pshift) & (s.H - 1), part = lane & ((1 << s.pshift) - 1);
    const int upl = s.nu >> s.pshift;                  // units per lane
    for (int e0 = 0; e0 < n; e0 += 4 * epw) {          // (wave-uniform trips: the shuffles below see their partners)
      int c[4];
      bool ok[4];
      float acc[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + u * epw + sub;
        ok[u] = e < n;
        c[u] = s.col[b0 + (ok[u] ? e : 0)];
        acc[u] = 0.f;
      }
      for (int q = 0; q < upl; ++q) {
        const int jj = head * s.F + ((q << s.pshift) + part) * VEC;
        float av[VEC], wv[VEC], bv[4][VEC];
        load_row<VEC>(arow + jj, av);
        op.weights(jj, wv);
#pragma unroll
        for (int u = 0; u < 4; ++u) load_row<VEC>(s.b + (size_t)c[u] * s.k + jj, bv[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[u] = op.elem(wv[v], av[v], bv[u][v], acc[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float t = merge_parts(acc[u], s.pshift);
        if (ok[u] && part == 0) s.out[(b0 + e0 + u * epw + sub) * s.H + head] = t;
      }
    }
    return;
  }
  // slow route: a lane an entry, the heads one after the other; the same P partial sums, merged in the butterfly's order
  const int P = 1 << s.pshift;
  for (int e0 = 0; e0 < n; e0 += 64) {
    const int e = e0 + lane;
    if (e >= n) continue;
    const float* brow = s.b + (size_t)s.col[b0 + e] * s.k;
    for (int h = 0; h < s.H; ++h) {
      float ps[4] = {0.f, 0.f, 0.f, 0.f};
      for (int u = 0; u < s.nu; ++u) {
        float av[VEC], wv[VEC], bv[VEC];
        load_row<VEC>(arow + h * s.F + u * VEC, av);
        op.weights(h * s.F + u * VEC, wv);
        load_row<VEC>(brow + h * s.F + u * VEC, bv);
        float t = ps[u & (P - 1)];
#pragma unroll
        for (int v = 0; v < VEC; ++v) t = op.elem(wv[v], av[v], bv[v], t);
        ps[u & (P - 1)] = t;
      }
      const float t = P == 4 ? (ps[0] + ps[2]) + (ps[1] + ps[3]) : P == 2 ? ps[0] + ps[1] : ps[0];
      s.out[(b0 + e) * s.H + h] = t;
    }
  }
}

template <int VEC, class Op>
__global__ void __launch_bounds__(256) sddmm_heads_rows_kernel(SddmmHeadsArgs s, Op op, const int* __restrict__ rowptr, int m,
                                                               int* __restrict__ long_flag) {
  const int lane = threadIdx.x & 63;
  for_wave_rows<kRowsPerWave, kGatherLong>(rowptr, m, lane, long_flag, [&](int r, int b, int n) {
    if (n > 0) sddmm_entries<VEC>(s, op, r, b, n, lane);
  });
}

template <int VEC, class Op>
__global__ void __launch_bounds__(256) sddmm_heads_long_kernel(SddmmHeadsArgs s, Op op, const int* __restrict__ rowptr, int m, int nnz,
                                                               int nchunks, const int* __restrict__ long_flag) {
  if (*long_flag == 0) return;
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = gridDim.x * 4;
  for_long_segments<kGatherChunk, kGatherLong>(rowptr, m, nnz, nchunks, wave, nwaves, lane, [&](int c, int slot, const Segment& sg) {
    sddmm_entries<VEC>(s, op, sg.r, sg.sb, sg.se - sg.sb, lane);
  });
}

template <int VEC, class Op>
hipError_t run_sddmm(SddmmHeadsArgs s, const Op& op, const int* rowptr, int m, int nnz, void* ws, hipStream_t st) {
  s.nu = s.F / VEC;
  const int low = s.nu & -s.nu;                        // the largest power of two dividing the units of a head
  s.pshift = low >= 4 ? 2 : low >= 2 ? 1 : 0;
  int* flag = static_cast<int*>(ws);
  if (hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), st); e != hipSuccess) return e;
  const long long waves = ((long long)m + kRowsPerWave - 1) / kRowsPerWave;
  sddmm_heads_rows_kernel<VEC, Op><<<(unsigned)((waves + 3) / 4), 256, 0, st>>>(s, op, rowptr, m, flag);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  if (nnz <= kGatherLong) return hipSuccess;
  const int nchunks = (int)(((long long)nnz + kGatherChunk - 1) / kGatherChunk);
  const int nw = nchunks < kGatherLongWaves ? nchunks : kGatherLongWaves;
  sddmm_heads_long_kernel<VEC, Op><<<(unsigned)((nw + 3) / 4), 256, 0, st>>>(s, op, rowptr, m, nnz, nchunks, flag);
  return hipGetLastError();
}

// log2 H where the entry walk has its fast route (H a power of two <= kMaxFastHeads), -1 otherwise
int fast_hshift(int H) {
  if (H > kMaxFastHeads || (H & (H - 1)) != 0) return -1;
  int hshift = 0;
  while ((1 << hshift) < H) ++hshift;
  return hshift;
}

}  // namespace

size_t heads_spmm_workspace_bytes(int nnz, int k) {
  return 16 + 8 * (size_t)k * (size_t)(((long long)nnz + kGatherChunk - 1) / kGatherChunk);
}

// the 16-byte form needs every gathered or stored row to start on a 16-byte boundary (the base pointers and the row stride)
// and a lane's four columns inside one head
hipError_t launch_spmm_heads(const int* rowptr, const int* idx, const int* perm, int rows, int nnz, int H, int k, const float* vals,
                             const float* x, float* out, void* ws, hipStream_t st) {
  const HeadsSpmmArgs a{idx, perm, vals, x, out, H, k / H, k};
  const bool wide = (k / H) % 4 == 0 && aligned16(x) && aligned16(out);
  const WeightedSumOp op;
  return wide ? run_spmm_vec<4>(a, op, rowptr, rows, nnz, ws, st) : run_spmm_vec<1>(a, op, rowptr, rows, nnz, ws, st);
}

hipError_t launch_sddmm_heads(const int* rowptr, const int* col, int m, int nnz, int H, int k, const float* a, const float* b,
                              float* out, void* ws, hipStream_t st) {
  const SddmmHeadsArgs s{col, a, b, out, H, k / H, k, fast_hshift(H), 0, 0};
  const bool wide = (k / H) % 4 == 0 && aligned16(a) && aligned16(b);
  const DotOp op;
  return wide ? run_sddmm<4>(s, op, rowptr, m, nnz, ws, st) : run_sddmm<1>(s, op, rowptr, m, nnz, ws, st);
}

size_t gatv2_workspace_bytes(int nnz, int k) {
  return 16 + 2 * 8 * (size_t)k * (size_t)(((long long)nnz + kGatherChunk - 1) / kGatherChunk);
}

hipError_t launch_gatv2_scores(const int* rowptr, const int* col, int m, int nnz, int H, int k, const float* h_dst, const float* h_src,
                               const float* att, float slope, float* out, void* ws, hipStream_t st) {
  const SddmmHeadsArgs s{col, h_dst, h_src, out, H, k / H, k, fast_hshift(H), 0, 0};
  const bool wide = (k / H) % 4 == 0 && aligned16(h_dst) && aligned16(h_src) && aligned16(att);
  const Gatv2ScoreOp op{att, slope};
  return wide ? run_sddmm<4>(s, op, rowptr, m, nnz, ws, st) : run_sddmm<1>(s, op, rowptr, m, nnz, ws, st);
}

hipError_t launch_gatv2_scores_backward(const int* rowptr, const int* idx, const int* perm, int rows, int nnz, int H, int k,
                                        const float* own, const float* other, const float* att, float slope, const float* g,
                                        float* grad_own, float* act_sums, void* ws, hipStream_t st) {
  const HeadsSpmmArgs a{idx, perm, g, other, grad_own, H, k / H, k};
  const bool wide = (k / H) % 4 == 0 && aligned16(own) && aligned16(other) && aligned16(att) && aligned16(grad_own) &&
                    aligned16(act_sums);
  if (act_sums) {
    const Gatv2BackwardOp<true> op{own, att, act_sums, slope};
    return wide ? run_spmm_vec<4>(a, op, rowptr, rows, nnz, ws, st) : run_spmm_vec<1>(a, op, rowptr, rows, nnz, ws, st);
  }
  const Gatv2BackwardOp<false> op{own, att, nullptr, slope};
  return wide ? run_spmm_vec<4>(a, op, rowptr, rows, nnz, ws, st) : run_spmm_vec<1>(a, op, rowptr, rows, nnz, ws, st);
}

}  // namespace gcn
