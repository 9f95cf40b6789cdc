// multihead.hip — the attention primitives for H heads in one pass over the adjacency: the per-head edge softmax (plain
// and fused with GAT scores) and their backwards, CSR row sums of an [nnz, H] array, the head-weighted SpMM and the
// per-head SDDMM.  Plan-free like edge_softmax.hip and aggregate.hip, whose kernels these follow: the caller's CSR in entry
// order, one 4-byte memset node and kernels (legal inside a stream capture), the host never reads a row length, no
// atomics — every output has one writer and every sum a fixed order, so two calls give the same bits.
//
// Layouts: node arrays [rows, k] with k = H * F, head h owns columns hF .. hF + F - 1; per-entry arrays [nnz, H], an
// entry's heads contiguous; per-node scalars [rows, H].  nnz * H < 2^31 (checked by the C ABI), so an element index of a
// per-entry array is an int.
//
// 1. Softmax family and segment sum ("reduce a row, map its entries"; the arithmetic of edge_softmax.hip, DESIGN §4.9: two
//    passes m = max, sum of exp2((s - m) log2 e), p = e * (1 / sum); backward and segment sums carried in fp64).
//    A row's [len, H] block is one contiguous stream of len * H elements.  With H a power of two <= 16 (the fast route)
//    element i belongs to head i mod H, and because H divides 8, 64 and 256 a lane that strides by its group size stays
//    on ONE head: it reduces privately, and the lanes of a head are merged by the xor butterfly with the offsets
//    G/2 .. H (the offsets below H would mix heads and are skipped).  The dispatch of edge_softmax.hip, in elements:
//      * a wave owns 8 rows; H <= 8 and all 8 rows of at most 32 elements: 8 lanes a row, 4 elements a lane in registers;
//      * else a row at a time on 64 lanes: up to 256 and up to 1024 elements in registers (4 or 16 a lane) — read once,
//        written once; more, up to 8192 ENTRIES, streamed with 4 loads a lane in flight (one touch per reduction and one
//        for the map, the repeats hit L2).  With 8 heads the Reddit-shaped mean row of 500 entries is 4000 elements and
//        is streamed: a 64-a-lane register form takes the kernel to 256 VGPRs and scratch;
//      * a row of more than 8192 entries raises the flag; the chunk kernels (a fixed grid of 256-thread blocks over chunks
//        of 8192 entries) write one partial per (chunk, long row, head) and the finish kernel merges a row's partials —
//        every block of the row the same partials in the same order: thread t takes chunks t, t + 256, ..., then the block
//        tree, ONE rescale per chunk for the softmax — and maps its chunk.
//    Any other H (the slow route: not a power of two, or above 16) runs the same code once per head with the lanes on
//    entries and stride H: the row pointer is read once, the rows' data H times with 4 useful bytes per H * 4 fetched.
//    In flight per wave: 4 (registers: 4 or 16) independent loads per lane.
//    Fixed orders: a lane adds its elements in ascending order, then the butterfly (same bits on every lane), then for a
//    block ((w0 + w1) + w2) + w3 over its waves.
//
// 2. spmm_heads ("gather a row per entry", aggregate.hip's wave): SLOTS entry slots x LPS lanes x VEC columns with
//    LPS = 16, 32 or 64 lanes for k / VEC <= 16, <= 32, more — so up to 256 columns the adjacency is walked once for all
//    heads and a gather brings the whole k-wide row; wider k tiles 256 columns over blockIdx.y.  VEC = 4 (one 16-byte load;
//    F % 4 == 0 keeps a lane's four columns in one head) or 1 (an operand that is not 16-byte aligned, or F % 4 != 0).  The
//    wave loads 64 indices (and permutation entries) with one coalesced load each and hands them out with ds_bpermute; each
//    slot has 4 gathers and their 4 one-word value loads vals[e * H + head] in flight before the first fma.  Rows of
//    more than kAggChunk entries: chunk partials per (chunk, row, column), merged in chunk order by the wave whose chunk
//    holds the row's first entry.
//    Fixed order: slot s adds the entries s, s + SLOTS, ... in ascending order (fma), the slots are merged by the xor
//    butterfly LPS .. 32, chunk partials in chunk order.
//
// 3. sddmm_heads: a wave takes a row at a time (8 rows a wave, long rows by chunks of kAggChunk entries on a fixed grid of
//    waves: no partials, an entry's result has one writer).  A head's F columns are U = F / VEC units; P = min(4, the
//    largest power of two dividing U) lanes share an (entry, head), lane p taking the units p, p + P, ...  With H a power
//    of two <= 16 an entry is H * P <= 64 adjacent lanes and a wave step takes 64 / (H P) entries, four steps in flight;
//    any other H puts an entry on a lane, which walks the heads one after the other (the slow route).
//    Fixed order of an (entry, head) sum, a function of F and VEC only — not of the row, the chunk, the slot or H:
//    s_p = fma chain over the units p, p + P, ... in ascending order, a unit's elements in ascending order; then
//    P = 2: s0 + s1, P = 4: (s0 + s2) + (s1 + s3).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "long_chunks.h"
#include "spmm_kernels.h"

namespace gcn {
namespace {

constexpr int kRowsPerWave = 8;
constexpr int kShortCnt = 32;                          // 8 lanes x 4 elements
constexpr int kEChunk = kEdgeChunk;                    // entries per block of the softmax family's long-row kernels
constexpr int kELong = kEdgeChunk;                     // its rows longer than this are split over blocks
constexpr int kELongGrid = 2048;
constexpr int kGChunk = kAggChunk;                     // entries per chunk of the gather kernels' long-row route
constexpr int kGLong = kAggChunk;
constexpr int kGLongWaves = 8192;
constexpr int kMaxFastHeads = 16;
constexpr float kLog2e = 1.4426950408889634f;

// how the elements of a row's [len, H] block map to lanes.  Fast route: shift = log2 H, hp = H, one pass with h0 = 0 —
// element i is entry i >> shift, head i & (hp - 1).  Slow route: shift = 0, hp = 1, a pass per head h0 — element i is entry i.
struct Lay {
  int H, shift, hp, h0;
  __device__ int cnt(int n) const { return n << shift; }           // (n * H <= nnz * H < 2^31)
  __device__ int off(int i) const { return i >> shift; }
  __device__ int head(int i) const { return (i & (hp - 1)) + h0; }
};

// over the lanes of a group of G that hold the same head: offsets G/2 .. hp (every such lane ends with the same bits)
template <int G>
__device__ __forceinline__ float hmax(float v, int hp) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1)
    if (o >= hp) v = fmaxf(v, __shfl_xor(v, o, G));
  return v;
}
template <int G, class T>
__device__ __forceinline__ T hsum(T v, int hp) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1)
    if (o >= hp) v += __shfl_xor(v, o, G);
  return v;
}

__device__ __forceinline__ float exps(float x, float m) { return __builtin_amdgcn_exp2f((x - m) * kLog2e); }
__device__ __forceinline__ float safe_max(float m) { return m == -INFINITY ? 0.f : m; }
__device__ __forceinline__ float safe_inv(float s) { return s == 0.f ? 0.f : 1.0f / s; }

// ---- the operations of the softmax family (edge_softmax.hip's, with a head: element (e, h) is at e * H + h) -----------------
struct SoftmaxOp {
  static constexpr bool SOFTMAX = true, MAP = false;
  const float* s;
  float* p;
  int H;
  __device__ float ctx(int, int) const { return 0.f; }
  __device__ float2 load(int e, int h, float) const { return make_float2(s[e * H + h], 0.f); }
  __device__ void store(int e, int h, float v) const { p[e * H + h] = v; }
};

struct GatSoftmaxOp {                                  // s = leaky_relu(a_dst[row, h] + a_src[col[e], h]), never stored
  static constexpr bool SOFTMAX = true, MAP = false;
  const int* col;
  const float *a_dst, *a_src;
  float slope;
  float* p;
  int H;
  __device__ float ctx(int r, int h) const { return a_dst[(size_t)r * H + h]; }
  __device__ float2 load(int e, int h, float c) const {
    const float t = c + a_src[(size_t)col[e] * H + h];
    return make_float2(t > 0.f ? t : t * slope, 0.f);
  }
  __device__ void store(int e, int h, float v) const { p[e * H + h] = v; }
};

struct SoftmaxBwdOp {                                  // ds = p (g - sum p g)
  static constexpr bool SOFTMAX = false, MAP = true, ROWOUT = false;
  const float *p, *g;
  float* ds;
  int H;
  __device__ float ctx(int, int) const { return 0.f; }
  __device__ float2 load(int e, int h, float) const { return make_float2(p[e * H + h], g[e * H + h]); }
  static __device__ double term(float2 v) { return (double)v.x * (double)v.y; }
  __device__ float map(int e, int h, float2 v, double t, float) const {
    const float d = (float)((double)v.x * ((double)v.y - t));
    ds[e * H + h] = d;
    return d;
  }
  __device__ void rowout(int, int, float) const {}
};

struct GatSoftmaxBwdOp {                               // ds = p (g - sum p g) leaky_relu'(s_pre); grad_a_dst[r, h] = sum ds
  static constexpr bool SOFTMAX = false, MAP = true, ROWOUT = true;
  const int* col;
  const float *a_dst, *a_src, *p, *g;
  float slope;
  float *ds, *grad_a_dst;
  int H;
  __device__ float ctx(int r, int h) const { return a_dst[(size_t)r * H + h]; }
  __device__ float2 load(int e, int h, float) const { return make_float2(p[e * H + h], g[e * H + h]); }
  static __device__ double term(float2 v) { return (double)v.x * (double)v.y; }
  __device__ float map(int e, int h, float2 v, double t, float c) const {
    const float pre = c + a_src[(size_t)col[e] * H + h];
    const float d = (float)((double)v.x * ((double)v.y - t) * (double)(pre > 0.f ? 1.f : slope));   // (slope at 0, as torch)
    ds[e * H + h] = d;
    return d;
  }
  __device__ void rowout(int r, int h, float v) const { grad_a_dst[(size_t)r * H + h] = v; }
};

struct SegSumOp {                                      // out[r, h] = sum x[e, h] (x[perm[e], h] with a permutation)
  static constexpr bool SOFTMAX = false, MAP = false, ROWOUT = true;
  const float* x;
  const int* perm;
  float* out;
  int H;
  __device__ float ctx(int, int) const { return 0.f; }
  __device__ float2 load(int e, int h, float) const { return make_float2(x[(perm ? perm[e] : e) * H + h], 0.f); }
  static __device__ double term(float2 v) { return (double)v.x; }
  __device__ float map(int, int, float2, double, float) const { return 0.f; }
  __device__ void rowout(int r, int h, float v) const { out[(size_t)r * H + h] = v; }
};

template <class Op>
__device__ __forceinline__ float2 pad() { return make_float2(Op::SOFTMAX ? -INFINITY : 0.f, 0.f); }
template <class Op>
__device__ __forceinline__ double term_of(float2 v) {
  if constexpr (Op::SOFTMAX) return 0.0; else return Op::term(v);
}

// ---- a row of at most G*K elements (n entries from b) on a group of G lanes: its elements stay in registers -----------------
template <int G, int K, class Op>
__device__ __forceinline__ void row_cached(const Op& op, const Lay& L, int r, bool row_ok, int b, int n, int gl) {
  const int h = L.head(gl);                            // (G is a multiple of hp: the lane's elements gl + G i share a head)
  const float c = row_ok ? op.ctx(r, h) : 0.f;
  const int cnt = L.cnt(n);
  float2 v[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const int idx = gl + G * i;
    v[i] = idx < cnt ? op.load(b + L.off(idx), h, c) : pad<Op>();
  }
  if constexpr (Op::SOFTMAX) {
    float m = v[0].x;
#pragma unroll
    for (int i = 1; i < K; ++i) m = fmaxf(m, v[i].x);
    m = safe_max(hmax<G>(m, L.hp));
    float ex[K], s = 0.f;
#pragma unroll
    for (int i = 0; i < K; ++i) {
      ex[i] = exps(v[i].x, m);
      s += ex[i];
    }
    const float inv = safe_inv(hsum<G, float>(s, L.hp));
#pragma unroll
    for (int i = 0; i < K; ++i) {
      const int idx = gl + G * i;
      if (idx < cnt) op.store(b + L.off(idx), h, ex[i] * inv);
    }
  } else {
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < K; ++i) t += term_of<Op>(v[i]);
    t = hsum<G, double>(t, L.hp);
    double post = 0.0;
    if constexpr (Op::MAP) {
#pragma unroll
      for (int i = 0; i < K; ++i) {
        const int idx = gl + G * i;
        if (idx < cnt) post += op.map(b + L.off(idx), h, v[i], t, c);
      }
      if constexpr (Op::ROWOUT) post = hsum<G, double>(post, L.hp);
    }
    if constexpr (Op::ROWOUT)
      if (row_ok && gl < L.hp) op.rowout(r, h, (float)(Op::MAP ? post : t));   // (lanes 0 .. hp - 1 hold the heads h0 + gl)
  }
}

// ---- a row of up to kELong entries on a whole wave, streamed ---------------------------------------------------------------------
template <class F>
__device__ __forceinline__ void for_elems4(int cnt, int lane, F f) {           // four independent loads in flight
  for (int base = lane; base < cnt; base += 256) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = base + 64 * u;
      if (i < cnt) f(i);
    }
  }
}

template <class Op>
__device__ __forceinline__ void row_stream(const Op& op, const Lay& L, int r, int b, int n, int lane) {
  const int h = L.head(lane);
  const float c = op.ctx(r, h);
  const int cnt = L.cnt(n);
  if constexpr (Op::SOFTMAX) {
    float m = -INFINITY;
    for_elems4(cnt, lane, [&](int i) { m = fmaxf(m, op.load(b + L.off(i), h, c).x); });
    m = safe_max(hmax<64>(m, L.hp));
    float s = 0.f;
    for_elems4(cnt, lane, [&](int i) { s += exps(op.load(b + L.off(i), h, c).x, m); });
    const float inv = safe_inv(hsum<64, float>(s, L.hp));
    for_elems4(cnt, lane, [&](int i) { op.store(b + L.off(i), h, exps(op.load(b + L.off(i), h, c).x, m) * inv); });
  } else {
    double t = 0.0;
    for_elems4(cnt, lane, [&](int i) { t += term_of<Op>(op.load(b + L.off(i), h, c)); });
    t = hsum<64, double>(t, L.hp);
    double post = 0.0;
    if constexpr (Op::MAP) {
      for_elems4(cnt, lane, [&](int i) { post += op.map(b + L.off(i), h, op.load(b + L.off(i), h, c), t, c); });
      if constexpr (Op::ROWOUT) post = hsum<64, double>(post, L.hp);
    }
    if constexpr (Op::ROWOUT)
      if (lane < L.hp) op.rowout(r, h, (float)(Op::MAP ? post : t));
  }
}

template <class Op>
__global__ void __launch_bounds__(256) heads_rows_kernel(Op op, Lay L, int passes, const int* __restrict__ rowptr, int m,
                                                         int* __restrict__ long_flag) {
  const int lane = threadIdx.x & 63;
  const long long wave = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (wave * kRowsPerWave >= m) return;                // (whole waves leave: the shuffles below see full groups)
  const int r0 = (int)wave * kRowsPerWave;
  const int ri = r0 + lane < m ? r0 + lane : m;
  const int rp = rowptr[ri];                           // lanes 0..8: the 9 row bounds (later lanes repeat rowptr[m])
  const int len = __shfl_down(rp, 1) - rp;
  const bool all_short = L.hp <= 8 && __ballot(lane < kRowsPerWave && L.cnt(len) > kShortCnt) == 0;
  for (int pass = 0; pass < passes; ++pass) {          // (fast route: one pass; slow route: a pass per head)
    L.h0 = pass;
    if (all_short) {
      const int g = lane >> 3;
      const int b = __shfl(rp, g), e = __shfl(rp, g + 1);
      row_cached<8, kShortCnt / 8, Op>(op, L, r0 + g, r0 + g < m, b, e - b, lane & 7);
      continue;
    }
    for (int j = 0; j < kRowsPerWave && r0 + j < m; ++j) {
      const int b = __shfl(rp, j), e = __shfl(rp, j + 1);
      const int n = e - b;
      if (n > kELong) {
        if (lane == 0) *long_flag = 1;                 // (every writer writes the same word)
        continue;
      }
      const int cnt = L.cnt(n);
      if (cnt <= 256) row_cached<64, 4, Op>(op, L, r0 + j, true, b, n, lane);  // (n == 0: nothing but rowout(r, h, 0))
      else if (cnt <= 1024) row_cached<64, 16, Op>(op, L, r0 + j, true, b, n, lane);
      else row_stream<Op>(op, L, r0 + j, b, n, lane);
    }
  }
}

// ---- long rows: a 256-thread block per chunk; a thread's elements tid + 256 i share the head L.head(tid) ----------------------
// the reduction over the threads of a head; the caller's head must be (tid & (hp - 1)) + h0.  sh: [4][kMaxFastHeads]
__device__ __forceinline__ float block_hmax(float v, int hp, float* sh) {
  v = hmax<64>(v, hp);
  const int lane = threadIdx.x & 63, hl = threadIdx.x & (hp - 1);
  __syncthreads();                                     // (sh may still be read from the reduction before)
  if (lane < hp) sh[(threadIdx.x >> 6) * kMaxFastHeads + lane] = v;
  __syncthreads();
  return fmaxf(fmaxf(sh[hl], sh[kMaxFastHeads + hl]), fmaxf(sh[2 * kMaxFastHeads + hl], sh[3 * kMaxFastHeads + hl]));
}
template <class T>
__device__ __forceinline__ T block_hsum(T v, int hp, T* sh) {
  v = hsum<64, T>(v, hp);
  const int lane = threadIdx.x & 63, hl = threadIdx.x & (hp - 1);
  __syncthreads();
  if (lane < hp) sh[(threadIdx.x >> 6) * kMaxFastHeads + lane] = v;
  __syncthreads();
  return ((sh[hl] + sh[kMaxFastHeads + hl]) + sh[2 * kMaxFastHeads + hl]) + sh[3 * kMaxFastHeads + hl];
}

template <class Op>
__global__ void __launch_bounds__(256) heads_long_partial_kernel(Op op, Lay L, int passes, const int* __restrict__ rowptr, int m,
                                                                 int nnz, int nchunks, const int* __restrict__ long_flag,
                                                                 float2* __restrict__ part) {
  if (*long_flag == 0) return;
  __shared__ float sh[4 * kMaxFastHeads];
  __shared__ double shd[4 * kMaxFastHeads];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int e0 = c * kEChunk;
    const int e1 = (long long)e0 + kEChunk < nnz ? e0 + kEChunk : nnz;
    const int rh = find_row(rowptr, m, e0, lane), rt = find_row(rowptr, m, e1 - 1, lane);
    for (int slot = 0; slot < 2; ++slot) {
      Segment s;
      if (!long_segment<kELong>(rowptr, slot, rh, rt, e0, e1, s)) continue;    // (block-uniform)
      for (int pass = 0; pass < passes; ++pass) {
        L.h0 = pass;
        const int h = L.head(tid), cnt = L.cnt(s.se - s.sb);
        const float cx = op.ctx(s.r, h);
        const size_t at = (2 * (size_t)c + slot) * L.H + h;
        if constexpr (Op::SOFTMAX) {
          float mx = -INFINITY;
          for (int i = tid; i < cnt; i += 256) mx = fmaxf(mx, op.load(s.sb + L.off(i), h, cx).x);
          mx = block_hmax(mx, L.hp, sh);
          const float ms = safe_max(mx);
          float sum = 0.f;
          for (int i = tid; i < cnt; i += 256) sum += exps(op.load(s.sb + L.off(i), h, cx).x, ms);
          sum = block_hsum(sum, L.hp, sh);             // (relative to safe_max(mx))
          if (tid < L.hp) part[at] = make_float2(mx, sum);
        } else {                                       // (sums are carried in fp64: a partial is one double in the same 8 bytes)
          double t = 0.0;
          for (int i = tid; i < cnt; i += 256) t += term_of<Op>(op.load(s.sb + L.off(i), h, cx));
          t = block_hsum(t, L.hp, shd);
          if (tid < L.hp) reinterpret_cast<double*>(part)[at] = t;
        }
      }
    }
  }
}

template <class Op>
__global__ void __launch_bounds__(256) heads_long_finish_kernel(Op op, Lay L, const int* __restrict__ rowptr, int m, int nnz,
                                                                int nchunks, const int* __restrict__ long_flag,
                                                                const float2* __restrict__ part) {
  if (*long_flag == 0) return;
  __shared__ float sh[4 * kMaxFastHeads];
  __shared__ double shd[4 * kMaxFastHeads];
  const int tid = threadIdx.x, lane = tid & 63;
  const int H = L.H;
  const bool fast = L.hp == H;
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int e0 = c * kEChunk;
    const int e1 = (long long)e0 + kEChunk < nnz ? e0 + kEChunk : nnz;
    const int rh = find_row(rowptr, m, e0, lane), rt = find_row(rowptr, m, e1 - 1, lane);
    for (int slot = 0; slot < 2; ++slot) {
      Segment s;
      if (!long_segment<kELong>(rowptr, slot, rh, rt, e0, e1, s)) continue;
      // the row's partials: chunks c_first..c_last, the first in slot 1 unless the row starts on the chunk's first entry.
      // Every block of the row merges the same partials in the same order, a head at a time (all 256 threads on that
      // head: thread t takes chunks t, t + 256, ..., then the block tree); on the fast route a thread keeps the result of
      // the head its elements belong to and the map follows the last head, on the slow route each head is mapped at once.
      const int c_first = s.rb / kEChunk, c_last = (s.re - 1) / kEChunk;
      const int first_slot = s.rb > c_first * kEChunk ? 1 : 0;
      float my_ms = 0.f, my_inv = 0.f;
      double my_t = 0.0;
      for (int hh = 0; hh < H; ++hh) {
        if constexpr (Op::SOFTMAX) {
          float mx = -INFINITY;
          for (int cc = c_first + tid; cc <= c_last; cc += 256)
            mx = fmaxf(mx, part[(2 * (size_t)cc + (cc == c_first ? first_slot : 0)) * H + hh].x);
          const float ms = safe_max(block_hmax(mx, 1, sh));
          float sum = 0.f;
          for (int cc = c_first + tid; cc <= c_last; cc += 256) {
            const float2 q = part[(2 * (size_t)cc + (cc == c_first ? first_slot : 0)) * H + hh];
            sum += q.y * exps(safe_max(q.x), ms);      // one rescale per chunk (an all -inf chunk: 0 * exp(0 - ms))
          }
          const float inv = safe_inv(block_hsum(sum, 1, sh));
          if (!fast || (tid & (H - 1)) == hh) { my_ms = ms; my_inv = inv; }
        } else {
          double t = 0.0;
          for (int cc = c_first + tid; cc <= c_last; cc += 256)
            t += reinterpret_cast<const double*>(part)[(2 * (size_t)cc + (cc == c_first ? first_slot : 0)) * H + hh];
          t = block_hsum(t, 1, shd);
          if constexpr (!Op::MAP && Op::ROWOUT) {
            if (c == c_first && tid == 0) op.rowout(s.r, hh, (float)t);
          }
          if (!fast || (tid & (H - 1)) == hh) my_t = t;
        }
        if (fast && hh + 1 < H) continue;              // (block-uniform)
        if constexpr (Op::SOFTMAX || Op::MAP) {
          Lay M = L;
          M.h0 = fast ? 0 : hh;
          const int h = M.head(tid), cnt = M.cnt(s.se - s.sb);
          const float cx = op.ctx(s.r, h);
          if constexpr (Op::SOFTMAX) {
            for (int i = tid; i < cnt; i += 256)
              op.store(s.sb + M.off(i), h, exps(op.load(s.sb + M.off(i), h, cx).x, my_ms) * my_inv);
          } else {
            for (int i = tid; i < cnt; i += 256) op.map(s.sb + M.off(i), h, op.load(s.sb + M.off(i), h, cx), my_t, cx);
          }
        }
      }
    }
  }
}

struct Route { Lay L; int passes; };
Route route_of(int H) {
  const bool fast = H <= kMaxFastHeads && (H & (H - 1)) == 0;
  int shift = 0;
  while (fast && (1 << shift) < H) ++shift;
  return Route{Lay{H, shift, fast ? H : 1, 0}, fast ? 1 : H};
}

template <class Op>
hipError_t run_rows(const Op& op, const Route& rt, const int* rowptr, int m, int* flag, hipStream_t st) {
  const long long waves = ((long long)m + kRowsPerWave - 1) / kRowsPerWave;
  heads_rows_kernel<Op><<<(unsigned)((waves + 3) / 4), 256, 0, st>>>(op, rt.L, rt.passes, rowptr, m, flag);
  return hipGetLastError();
}

template <class Op>
hipError_t run_long(const Op& op, const Route& rt, const int* rowptr, int m, int nnz, int* flag, float2* part, hipStream_t st) {
  if (nnz <= kELong) return hipSuccess;                // (no row can be long)
  const int nchunks = (int)(((long long)nnz + kEChunk - 1) / kEChunk);
  const int grid = nchunks < kELongGrid ? nchunks : kELongGrid;
  heads_long_partial_kernel<Op><<<grid, 256, 0, st>>>(op, rt.L, rt.passes, rowptr, m, nnz, nchunks, flag, part);
  heads_long_finish_kernel<Op><<<grid, 256, 0, st>>>(op, rt.L, rowptr, m, nnz, nchunks, flag, part);
  return hipGetLastError();
}

template <class Op>
hipError_t run_edge(const Op& op, int H, const int* rowptr, int m, int nnz, void* ws, hipStream_t st) {
  const Route rt = route_of(H);
  int* flag = static_cast<int*>(ws);
  float2* part = reinterpret_cast<float2*>(static_cast<char*>(ws) + 16);
  if (hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), st); e != hipSuccess) return e;
  if (hipError_t e = run_rows(op, rt, rowptr, m, flag, st); e != hipSuccess) return e;
  return run_long(op, rt, rowptr, m, nnz, flag, part, st);
}

// ================================================================================================================================
// the gather kernels
template <int VEC>
__device__ __forceinline__ void load_row(const float* p, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    static_assert(VEC == 1);
    v[0] = p[0];
  }
}
template <int VEC>
__device__ __forceinline__ void store_row(float* p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    static_assert(VEC == 1);
    p[0] = v[0];
  }
}

struct HeadsSpmmArgs {
  const int *idx, *perm;
  const float *vals, *x;
  float* out;
  int H, F, k;
};

// entries [b, b + n) of one row (n <= kGChunk) on a wave; the lane's columns are j .. j + VEC of head `head` (jok: they exist)
template <int VEC, int LPS>
__device__ __forceinline__ void spmm_walk(const HeadsSpmmArgs& a, int b, int n, int lane, int j, bool jok, int head, float (&acc)[VEC]) {
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
        for (int v = 0; v < VEC; ++v) acc[v] = ok ? __builtin_fmaf(w[u], xv[u][v], acc[v]) : acc[v];
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

template <int VEC, int LPS>
__global__ void __launch_bounds__(256) spmm_heads_rows_kernel(HeadsSpmmArgs a, const int* __restrict__ rowptr, int rows,
                                                              int* __restrict__ long_flag) {
  const int lane = threadIdx.x & 63;
  const long long wave = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (wave * kRowsPerWave >= rows) return;
  const int r0 = (int)wave * kRowsPerWave;
  const int ri = r0 + lane < rows ? r0 + lane : rows;
  const int rp = rowptr[ri];
  const int j = (blockIdx.y * LPS + (lane % LPS)) * VEC;
  const bool jok = j < a.k;
  const int head = jok ? j / a.F : 0;
  for (int q = 0; q < kRowsPerWave && r0 + q < rows; ++q) {
    const int b = __shfl(rp, q), e = __shfl(rp, q + 1);
    const int n = e - b;
    if (n > kGLong) {
      if (lane == 0) *long_flag = 1;
      continue;
    }
    float acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
    spmm_walk<VEC, LPS>(a, b, n, lane, j, jok, head, acc);
    merge_slots<VEC, LPS>(acc);
    if (lane < LPS && jok) store_row<VEC>(a.out + (size_t)(r0 + q) * a.k + j, acc);
  }
}

template <int VEC, int LPS>
__global__ void __launch_bounds__(256) spmm_heads_long_partial_kernel(HeadsSpmmArgs a, const int* __restrict__ rowptr, int rows, int nnz,
                                                                      int nchunks, const int* __restrict__ long_flag,
                                                                      float* __restrict__ part) {
  if (*long_flag == 0) return;
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = gridDim.x * 4;
  const int j = (blockIdx.y * LPS + (lane % LPS)) * VEC;
  const bool jok = j < a.k;
  const int head = jok ? j / a.F : 0;
  for (int c = wave; c < nchunks; c += nwaves) {
    const int e0 = c * kGChunk;
    const int e1 = (long long)e0 + kGChunk < nnz ? e0 + kGChunk : nnz;
    const int rh = find_row(rowptr, rows, e0, lane), rt = find_row(rowptr, rows, e1 - 1, lane);
    for (int slot = 0; slot < 2; ++slot) {
      Segment sg;
      if (!long_segment<kGLong>(rowptr, slot, rh, rt, e0, e1, sg)) continue;   // (wave-uniform)
      float acc[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] = 0.f;
      spmm_walk<VEC, LPS>(a, sg.sb, sg.se - sg.sb, lane, j, jok, head, acc);
      merge_slots<VEC, LPS>(acc);
      if (lane < LPS && jok) {
        float* p = part + (2 * (size_t)c + slot) * a.k + j;
#pragma unroll
        for (int v = 0; v < VEC; ++v) p[v] = acc[v];
      }
    }
  }
}

template <int VEC, int LPS>
__global__ void __launch_bounds__(256) spmm_heads_long_finish_kernel(HeadsSpmmArgs a, const int* __restrict__ rowptr, int rows, int nnz,
                                                                     int nchunks, const int* __restrict__ long_flag,
                                                                     const float* __restrict__ part) {
  if (*long_flag == 0) return;
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = gridDim.x * 4;
  const int j0 = blockIdx.y * LPS * VEC;
  const int j1 = j0 + LPS * VEC < a.k ? j0 + LPS * VEC : a.k;
  for (int c = wave; c < nchunks; c += nwaves) {
    const int e0 = c * kGChunk;
    const int e1 = (long long)e0 + kGChunk < nnz ? e0 + kGChunk : nnz;
    const int rh = find_row(rowptr, rows, e0, lane), rt = find_row(rowptr, rows, e1 - 1, lane);
    for (int slot = 0; slot < 2; ++slot) {
      Segment sg;
      if (!long_segment<kGLong>(rowptr, slot, rh, rt, e0, e1, sg)) continue;
      // one writer per row: the wave whose chunk holds the row's first entry merges the partials, in chunk order
      const int c_first = sg.rb / kGChunk, c_last = (sg.re - 1) / kGChunk;
      if (c != c_first) continue;
      const int first_slot = sg.rb > c_first * kGChunk ? 1 : 0;
      for (int j = j0 + lane; j < j1; j += 64) {
        float acc = part[(2 * (size_t)c_first + first_slot) * a.k + j];
        for (int cc = c_first + 1; cc <= c_last; ++cc) acc += part[2 * (size_t)cc * a.k + j];
        a.out[(size_t)sg.r * a.k + j] = acc;
      }
    }
  }
}

template <int VEC, int LPS>
hipError_t run_spmm(const HeadsSpmmArgs& a, const int* rowptr, int rows, int nnz, void* ws, hipStream_t st) {
  int* flag = static_cast<int*>(ws);
  float* part = reinterpret_cast<float*>(static_cast<char*>(ws) + 16);
  const long long tiles = ((long long)a.k + LPS * VEC - 1) / (LPS * VEC);
  if (tiles > 65535) return hipErrorInvalidValue;
  if (hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), st); e != hipSuccess) return e;
  const long long waves = ((long long)rows + kRowsPerWave - 1) / kRowsPerWave;
  spmm_heads_rows_kernel<VEC, LPS><<<dim3((unsigned)((waves + 3) / 4), (unsigned)tiles), 256, 0, st>>>(a, rowptr, rows, flag);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  if (nnz <= kGLong) return hipSuccess;
  const int nchunks = (int)(((long long)nnz + kGChunk - 1) / kGChunk);
  const int nw = nchunks < kGLongWaves ? nchunks : kGLongWaves;
  const dim3 grid((unsigned)((nw + 3) / 4), (unsigned)tiles);
  spmm_heads_long_partial_kernel<VEC, LPS><<<grid, 256, 0, st>>>(a, rowptr, rows, nnz, nchunks, flag, part);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  spmm_heads_long_finish_kernel<VEC, LPS><<<grid, 256, 0, st>>>(a, rowptr, rows, nnz, nchunks, flag, part);
  return hipGetLastError();
}

template <int VEC>
hipError_t run_spmm_vec(const HeadsSpmmArgs& a, const int* rowptr, int rows, int nnz, void* ws, hipStream_t st) {
  const int units = a.k / VEC;
  if (units <= 16) return run_spmm<VEC, 16>(a, rowptr, rows, nnz, ws, st);
  if (units <= 32) return run_spmm<VEC, 32>(a, rowptr, rows, nnz, ws, st);
  return run_spmm<VEC, 64>(a, rowptr, rows, nnz, ws, st);
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

// the merge of the P partial sums of an (entry, head): the butterfly's order, P = 2: s0 + s1, P = 4: (s0 + s2) + (s1 + s3)
__device__ __forceinline__ float merge_parts(float s, int pshift) {
  if (pshift == 2) s += __shfl_xor(s, 2);
  if (pshift >= 1) s += __shfl_xor(s, 1);
  return s;
}

// entries [b0, b0 + n) of row r (0 < n <= kGChunk) on a wave
template <int VEC>
__device__ __forceinline__ void sddmm_entries(const SddmmHeadsArgs& s, int r, int b0, int n, int lane) {
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
        float av[VEC], bv[4][VEC];
        load_row<VEC>(arow + jj, av);
#pragma unroll
        for (int u = 0; u < 4; ++u) load_row<VEC>(s.b + (size_t)c[u] * s.k + jj, bv[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
          for (int v = 0; v < VEC; ++v) acc[u] = __builtin_fmaf(av[v], bv[u][v], acc[u]);
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
        float av[VEC], bv[VEC];
        load_row<VEC>(arow + h * s.F + u * VEC, av);
        load_row<VEC>(brow + h * s.F + u * VEC, bv);
        float t = ps[u & (P - 1)];
#pragma unroll
        for (int v = 0; v < VEC; ++v) t = __builtin_fmaf(av[v], bv[v], t);
        ps[u & (P - 1)] = t;
      }
      const float t = P == 4 ? (ps[0] + ps[2]) + (ps[1] + ps[3]) : P == 2 ? ps[0] + ps[1] : ps[0];
      s.out[(b0 + e) * s.H + h] = t;
    }
  }
}

template <int VEC>
__global__ void __launch_bounds__(256) sddmm_heads_rows_kernel(SddmmHeadsArgs s, const int* __restrict__ rowptr, int m,
                                                               int* __restrict__ long_flag) {
  const int lane = threadIdx.x & 63;
  const long long wave = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (wave * kRowsPerWave >= m) return;
  const int r0 = (int)wave * kRowsPerWave;
  const int ri = r0 + lane < m ? r0 + lane : m;
  const int rp = rowptr[ri];
  for (int q = 0; q < kRowsPerWave && r0 + q < m; ++q) {
    const int b = __shfl(rp, q), e = __shfl(rp, q + 1);
    const int n = e - b;
    if (n > kGLong) {
      if (lane == 0) *long_flag = 1;
      continue;
    }
    if (n > 0) sddmm_entries<VEC>(s, r0 + q, b, n, lane);
  }
}

template <int VEC>
__global__ void __launch_bounds__(256) sddmm_heads_long_kernel(SddmmHeadsArgs s, const int* __restrict__ rowptr, int m, int nnz,
                                                               int nchunks, const int* __restrict__ long_flag) {
  if (*long_flag == 0) return;
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = gridDim.x * 4;
  for (int c = wave; c < nchunks; c += nwaves) {
    const int e0 = c * kGChunk;
    const int e1 = (long long)e0 + kGChunk < nnz ? e0 + kGChunk : nnz;
    const int rh = find_row(rowptr, m, e0, lane), rt = find_row(rowptr, m, e1 - 1, lane);
    for (int slot = 0; slot < 2; ++slot) {
      Segment sg;
      if (!long_segment<kGLong>(rowptr, slot, rh, rt, e0, e1, sg)) continue;
      sddmm_entries<VEC>(s, sg.r, sg.sb, sg.se - sg.sb, lane);
    }
  }
}

template <int VEC>
hipError_t run_sddmm(SddmmHeadsArgs s, const int* rowptr, int m, int nnz, void* ws, hipStream_t st) {
  s.nu = s.F / VEC;
  const int low = s.nu & -s.nu;                        // the largest power of two dividing the units of a head
  s.pshift = low >= 4 ? 2 : low >= 2 ? 1 : 0;
  int* flag = static_cast<int*>(ws);
  if (hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), st); e != hipSuccess) return e;
  const long long waves = ((long long)m + kRowsPerWave - 1) / kRowsPerWave;
  sddmm_heads_rows_kernel<VEC><<<(unsigned)((waves + 3) / 4), 256, 0, st>>>(s, rowptr, m, flag);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  if (nnz <= kGLong) return hipSuccess;
  const int nchunks = (int)(((long long)nnz + kGChunk - 1) / kGChunk);
  const int nw = nchunks < kGLongWaves ? nchunks : kGLongWaves;
  sddmm_heads_long_kernel<VEC><<<(unsigned)((nw + 3) / 4), 256, 0, st>>>(s, rowptr, m, nnz, nchunks, flag);
  return hipGetLastError();
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

size_t heads_edge_workspace_bytes(int nnz, int H) {
  return 16 + 16 * (size_t)H * (size_t)(((long long)nnz + kEChunk - 1) / kEChunk);
}
size_t heads_spmm_workspace_bytes(int nnz, int k) {
  return 16 + 8 * (size_t)k * (size_t)(((long long)nnz + kGChunk - 1) / kGChunk);
}

hipError_t launch_edge_softmax_heads(const int* rowptr, int m, int nnz, int H, const float* s, float* p, void* ws, hipStream_t st) {
  return run_edge(SoftmaxOp{s, p, H}, H, rowptr, m, nnz, ws, st);
}

hipError_t launch_edge_softmax_heads_backward(const int* rowptr, int m, int nnz, int H, const float* p, const float* g, float* ds,
                                              void* ws, hipStream_t st) {
  return run_edge(SoftmaxBwdOp{p, g, ds, H}, H, rowptr, m, nnz, ws, st);
}

hipError_t launch_gat_edge_softmax_heads(const int* rowptr, const int* col, int m, int nnz, int H, const float* a_dst,
                                         const float* a_src, float slope, float* p, void* ws, hipStream_t st) {
  return run_edge(GatSoftmaxOp{col, a_dst, a_src, slope, p, H}, H, rowptr, m, nnz, ws, st);
}

hipError_t launch_gat_edge_softmax_heads_backward(const int* rowptr, const int* col, int m, int nnz, int H, const float* a_dst,
                                                  const float* a_src, float slope, const float* p, const float* g, float* ds,
                                                  float* grad_a_dst, void* ws, hipStream_t st) {
  if (hipError_t e = run_edge(GatSoftmaxBwdOp{col, a_dst, a_src, p, g, slope, ds, grad_a_dst, H}, H, rowptr, m, nnz, ws, st);
      e != hipSuccess)
    return e;
  // grad_a_dst of the long rows: the row kernel left them out, and their ds is complete only now — the long-row half of a
  // segment sum over ds (the flag still says whether there is such a row)
  int* flag = static_cast<int*>(ws);
  float2* part = reinterpret_cast<float2*>(static_cast<char*>(ws) + 16);
  return run_long(SegSumOp{ds, nullptr, grad_a_dst, H}, route_of(H), rowptr, m, nnz, flag, part, st);
}

hipError_t launch_segment_sum_heads(const int* rowptr, int rows, int nnz, int H, const float* x, const int* perm, float* out,
                                    void* ws, hipStream_t st) {
  return run_edge(SegSumOp{x, perm, out, H}, H, rowptr, rows, nnz, ws, st);
}

// the 16-byte form needs every gathered or stored row to start on a 16-byte boundary (the base pointers and the row stride)
// and a lane's four columns inside one head
hipError_t launch_spmm_heads(const int* rowptr, const int* idx, const int* perm, int rows, int nnz, int H, int k, const float* vals,
                             const float* x, float* out, void* ws, hipStream_t st) {
  const HeadsSpmmArgs a{idx, perm, vals, x, out, H, k / H, k};
  const bool wide = (k / H) % 4 == 0 && aligned16(x) && aligned16(out);
  return wide ? run_spmm_vec<4>(a, rowptr, rows, nnz, ws, st) : run_spmm_vec<1>(a, rowptr, rows, nnz, ws, st);
}

hipError_t launch_sddmm_heads(const int* rowptr, const int* col, int m, int nnz, int H, int k, const float* a, const float* b,
                              float* out, void* ws, hipStream_t st) {
  const bool fast = H <= kMaxFastHeads && (H & (H - 1)) == 0;
  int hshift = -1;
  if (fast)
    for (hshift = 0; (1 << hshift) < H; ++hshift) {}
  const SddmmHeadsArgs s{col, a, b, out, H, k / H, k, hshift, 0, 0};
  const bool wide = (k / H) % 4 == 0 && aligned16(a) && aligned16(b);
  return wide ? run_sddmm<4>(s, rowptr, m, nnz, ws, st) : run_sddmm<1>(s, rowptr, m, nnz, ws, st);
}

}  // namespace gcn
