// edge_softmax.hip — softmax over the stored entries of every CSR row ("edge softmax"), its backward, the fused GAT score
// form of both, and plain CSR row sums of a per-entry array — for one head ([nnz] arrays) and for H heads in one pass over
// the adjacency ([nnz, H] arrays, an entry's heads contiguous; per-node scalars [rows, H]; nnz * H < 2^31, checked by the
// C ABI, so an element index of a per-entry array is an int).  Everything works on the caller's CSR in entry order, takes
// no plan, only enqueues (one 4-byte memset node and kernels: legal inside a stream capture) and uses no atomics: every
// output has one writer and every sum a fixed order, so results are bit-identical from call to call.
//
// All five operations are "reduce a row, then map its entries with the result", and the host knows nothing about the row
// lengths (reading them would synchronise).  So ONE row kernel adapts per wave, and two chunk kernels take what a wave
// cannot.  A row's [len, H] block is one contiguous stream of len * H elements; the dispatch, in elements:
//   * a wave owns 8 consecutive rows.  If H <= 8 and all 8 have at most 32 elements, 8 lanes take each row (4 elements per
//     lane in registers; Cora-shaped rows of 1-5 entries, and millions of empty rows cost one rowptr load per 8 rows);
//   * otherwise the wave takes its rows one after the other with all 64 lanes: up to 1024 elements stay in registers
//     between the reduction and the map (4 or 16 per lane), so such a row is read once and written once;
//   * more, up to 8192 ENTRIES, are streamed with 4 loads a lane in flight: one touch per reduction and one for the map
//     (the repeats hit L2).  With 8 heads the Reddit-shaped mean row of 500 entries is 4000 elements and is streamed: a
//     64-a-lane register form takes the kernel to 256 VGPRs and scratch;
//   * a row of more than kLongRow entries is left alone and a flag in the workspace is raised.  The chunk kernels
//     (a fixed grid of 256-thread blocks walking chunks of kChunk = 8192 entries, returning at once while the flag is
//     down) find the at most two long rows that meet a chunk (the rows of its first and last entry: a 64-ary search of
//     rowptr per wave), write one partial per (chunk, long row, head) to the workspace, and a second kernel merges a row's
//     partials — every block of the row the same partials in the same order: thread t takes chunks t, t + 256, ..., then
//     the block tree, ONE rescale per chunk for the softmax — and maps its chunk.  A row holding a whole 100 M-entry
//     matrix is spread over the chip.
//
// Heads: ONE copy of all this, templated on a layout that says how a row's elements map to lanes.
//   * OneLay (H = 1, all of it compile-time constants: element i is entry i, head 0): the single-head kernels.
//   * HeadsLay, fast route (H a power of two <= 16): element i belongs to head i mod H, and because H divides 8, 64 and
//     256 a lane that strides by its group size stays on ONE head: it reduces privately, and the lanes of a head are merged
//     by the xor butterfly with the offsets G/2 .. H (the offsets below H would mix heads and are skipped).
//   * HeadsLay, slow route (any other H): the same code once per head with the lanes on entries and stride H: the row
//     pointer is read once, the rows' data H times with 4 useful bytes per H * 4 fetched.
// The single-head form is the heads code with H = 1, shift = 0, hp = 1 folded in by the compiler, not a second text.
// Fixed orders: a lane adds its elements in ascending order, then the butterfly (same bits on every lane), then for a
// block ((w0 + w1) + w2) + w3 over its waves.
//
// Softmax arithmetic: two passes, not an online rescaled sum — m = max, then sum of exp2((s - m) * log2 e)
// — because a rescale is one more rounded factor per step of the running maximum, and the short and medium rows that
// are nearly all of the work sit in registers for both passes anyway.  Long rows merge per-chunk (max, sum) pairs with
// ONE rescale each (the global maximum of the partials first, then the sum).  p = e * (1 / sum).
// The backward's row sums (sum p g, sum ds) and the segment sum are carried in fp64: ds = p (g - t) cancels, so an fp32 t
// would leave grad_a_dst = sum ds with an error the size of eps * sum p|g| however small sum |ds| is; fp64 adds are free
// in a kernel that waits for memory.
// Deliberately unlike torch.softmax: a row whose entries are all -inf gets zeros (not NaN), so a fully masked row is
// usable; an entry of -inf beside a finite one gets 0; a NaN makes its own row NaN and no other.
#include <hip/hip_runtime.h>

#include <cmath>

#include "long_chunks.h"
#include "spmm_kernels.h"

namespace gcn {
namespace {

constexpr int kRowsPerWave = 8;
constexpr int kShortCnt = 32;                          // 8 lanes x 4 elements
constexpr int kChunk = kEdgeChunk;                     // entries per block of the long-row kernels
constexpr int kLongRow = kEdgeChunk;                   // rows longer than this are split over blocks (>= kChunk: long_segment)
constexpr int kLongGrid = 2048;                        // blocks of the long-row kernels (they loop over the chunks)
constexpr int kMaxFastHeads = 16;
constexpr float kLog2e = 1.4426950408889634f;

// how the elements of a row's [len, H] block map to lanes.  Fast route: shift = log2 H, hp = H, one pass with h0 = 0 —
// element i is entry i >> shift, head i & (hp - 1).  Slow route: shift = 0, hp = 1, a pass per head h0 — element i is entry i.
struct HeadsLay {
  static constexpr int kMaxHp = kMaxFastHeads;
  int H, shift, hp, h0;
  __device__ int cnt(int n) const { return n << shift; }           // (n * H <= nnz * H < 2^31)
  __device__ int off(int i) const { return i >> shift; }
  __device__ int head(int i) const { return (i & (hp - 1)) + h0; }
  __device__ void pass(int p) { h0 = p; }
  __device__ static int passes(int n) { return n; }
};

// one head: the same with every member a constant, so the head arithmetic folds away (One: what its operations keep in
// place of int H)
struct One {
  __host__ __device__ constexpr operator int() const { return 1; }
};
struct OneLay {
  static constexpr int kMaxHp = 1;
  static constexpr One H{};
  static constexpr int hp = 1;
  __device__ static int cnt(int n) { return n; }
  __device__ static int off(int i) { return i; }
  __device__ static int head(int) { return 0; }
  __device__ static void pass(int) {}
  __device__ static int passes(int) { return 1; }
};

// over the lanes of a group of G that hold the same head: offsets G/2 .. hp (a butterfly: every such lane ends with the
// same bits)
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

// exp(x - m) through v_exp_f32; -inf gives 0
__device__ __forceinline__ float exps(float x, float m) { return __builtin_amdgcn_exp2f((x - m) * kLog2e); }
// (the maximum of an all -inf row is -inf: subtracting it would make NaN of every entry)
__device__ __forceinline__ float safe_max(float m) { return m == -INFINITY ? 0.f : m; }
__device__ __forceinline__ float safe_inv(float s) { return s == 0.f ? 0.f : 1.0f / s; }

// ---- the operations (HT: int, or One on the one-head layout; element (e, h) is at e * H + h) ------------------------------
// load(e, h, c): what element (e, h) contributes (c = ctx(r, h), a per-row value).  SOFTMAX ops reduce .x by (max, sum of
// exp) and store(e, h, p); the others reduce term(v) by a sum, then, with MAP, map(e, h, v, t, c) writes the element's result
// and returns it to be summed again for rowout(r, h, .) (ROWOUT; without MAP rowout gets the first sum).
template <class HT>
struct SoftmaxOp {
  static constexpr bool SOFTMAX = true, MAP = false;
  const float* s;
  float* p;
  HT H;
  __device__ float ctx(int, int) const { return 0.f; }
  __device__ float2 load(int e, int h, float) const { return make_float2(s[e * H + h], 0.f); }
  __device__ void store(int e, int h, float v) const { p[e * H + h] = v; }
};

template <class HT>
struct GatSoftmaxOp {                                  // s = leaky_relu(a_dst[row, h] + a_src[col[e], h]), never stored
  static constexpr bool SOFTMAX = true, MAP = false;
  const int* col;
  const float *a_dst, *a_src;
  float slope;
  float* p;
  HT H;
  __device__ float ctx(int r, int h) const { return a_dst[(size_t)r * H + h]; }
  __device__ float2 load(int e, int h, float c) const {
    const float t = c + a_src[(size_t)col[e] * H + h];
    return make_float2(t > 0.f ? t : t * slope, 0.f);
  }
  __device__ void store(int e, int h, float v) const { p[e * H + h] = v; }
};

template <class HT>
struct SoftmaxBwdOp {                                  // ds = p (g - sum p g)
  static constexpr bool SOFTMAX = false, MAP = true, ROWOUT = false;
  const float *p, *g;
  float* ds;
  HT H;
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

template <class HT>
struct GatSoftmaxBwdOp {                               // ds = p (g - sum p g) leaky_relu'(s_pre); grad_a_dst[r, h] = sum ds
  static constexpr bool SOFTMAX = false, MAP = true, ROWOUT = true;
  const int* col;
  const float *a_dst, *a_src, *p, *g;
  float slope;
  float *ds, *grad_a_dst;
  HT H;
  __device__ float ctx(int r, int h) const { return a_dst[(size_t)r * H + h]; }
  __device__ float2 load(int e, int h, float) const { return make_float2(p[e * H + h], g[e * H + h]); }
  static __device__ double term(float2 v) { return (double)v.x * (double)v.y; }
  __device__ float map(int e, int h, float2 v, double t, float c) const {
    const float pre = c + a_src[(size_t)col[e] * H + h];
    const float d = (float)((double)v.x * ((double)v.y - t) * (double)(pre > 0.f ? 1.f : slope));   // (slope at 0, as torch's leaky_relu)
    ds[e * H + h] = d;
    return d;
  }
  __device__ void rowout(int r, int h, float v) const { grad_a_dst[(size_t)r * H + h] = v; }
};

template <class HT>
struct SegSumOp {                                      // out[r, h] = sum x[e, h] (x[perm[e], h] with a permutation)
  static constexpr bool SOFTMAX = false, MAP = false, ROWOUT = true;
  const float* x;
  const int* perm;
  float* out;
  HT H;
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

// ---- a row of at most G*K elements (n entries from b) on a group of G lanes (gl = lane in the group): its elements stay in
// registers ----------------------------------------------------------------------------------------------------------------
template <int G, int K, class Op, class Lay>
__device__ __forceinline__ void row_cached(const Op& op, const Lay& L, int r, bool row_ok, int b, int n, int gl) {
  const int h = L.head(gl);                            // (G is a multiple of hp: the lane's elements gl + G i share a head)
  const float c = row_ok ? op.ctx(r, h) : 0.f;
  const int cnt = L.cnt(n);
  float2 v[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const int idx = gl + G * i;                        // (offsets from b: b + off is formed only inside the row, so never past INT_MAX)
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

// ---- a row of up to kLongRow entries on a whole wave, streamed: one touch per reduction, one for the map ----------------
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

template <class Op, class Lay>
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

template <class Op, class Lay>
__global__ void __launch_bounds__(256) edge_rows_kernel(Op op, Lay L, int passes, const int* __restrict__ rowptr, int m,
                                                        int* __restrict__ long_flag) {
  const int lane = threadIdx.x & 63;
  const long long wave = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (wave * kRowsPerWave >= m) return;                // (whole waves leave: the shuffles below see full groups)
  const int r0 = (int)wave * kRowsPerWave;
  const int ri = r0 + lane < m ? r0 + lane : m;
  const int rp = rowptr[ri];                           // lanes 0..8: the 9 row bounds (later lanes repeat rowptr[m])
  const int len = __shfl_down(rp, 1) - rp;
  const bool all_short = L.hp <= 8 && __ballot(lane < kRowsPerWave && L.cnt(len) > kShortCnt) == 0;
  for (int pass = 0; pass < Lay::passes(passes); ++pass) {   // (one head and the fast route: one pass; slow route: a pass per head)
    L.pass(pass);
    if (all_short) {
      const int g = lane >> 3;
      const int b = __shfl(rp, g), e = __shfl(rp, g + 1);
      row_cached<8, kShortCnt / 8, Op>(op, L, r0 + g, r0 + g < m, b, e - b, lane & 7);
      continue;
    }
    for (int j = 0; j < kRowsPerWave && r0 + j < m; ++j) {
      const int b = __shfl(rp, j), e = __shfl(rp, j + 1);
      const int n = e - b;
      if (n > kLongRow) {
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

// ---- long rows (find_row, Segment and long_segment: long_chunks.h): a 256-thread block per chunk; a thread's elements
// tid + 256 i share the head L.head(tid) -------------------------------------------------------------------------------------
// the reduction over the threads of a head; the caller's head must be (tid & (hp - 1)) + h0.  sh: [4][MAXHP]
template <int MAXHP>
__device__ __forceinline__ float block_hmax(float v, int hp, float* sh) {
  v = hmax<64>(v, hp);
  const int lane = threadIdx.x & 63, hl = threadIdx.x & (hp - 1);
  __syncthreads();                                     // (sh may still be read from the reduction before)
  if (lane < hp) sh[(threadIdx.x >> 6) * MAXHP + lane] = v;
  __syncthreads();
  return fmaxf(fmaxf(sh[hl], sh[MAXHP + hl]), fmaxf(sh[2 * MAXHP + hl], sh[3 * MAXHP + hl]));
}
template <int MAXHP, class T>
__device__ __forceinline__ T block_hsum(T v, int hp, T* sh) {
  v = hsum<64, T>(v, hp);
  const int lane = threadIdx.x & 63, hl = threadIdx.x & (hp - 1);
  __syncthreads();
  if (lane < hp) sh[(threadIdx.x >> 6) * MAXHP + lane] = v;
  __syncthreads();
  return ((sh[hl] + sh[MAXHP + hl]) + sh[2 * MAXHP + hl]) + sh[3 * MAXHP + hl];
}

template <class Op, class Lay>
__global__ void __launch_bounds__(256) edge_long_partial_kernel(Op op, Lay L, int passes, const int* __restrict__ rowptr, int m,
                                                                int nnz, int nchunks, const int* __restrict__ long_flag,
                                                                float2* __restrict__ part) {
  if (*long_flag == 0) return;
  constexpr int MH = Lay::kMaxHp;
  __shared__ float sh[4 * MH];
  __shared__ double shd[4 * MH];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int e0 = c * kChunk;
    const int e1 = (long long)e0 + kChunk < nnz ? e0 + kChunk : nnz;
    const int rh = find_row(rowptr, m, e0, lane), rt = find_row(rowptr, m, e1 - 1, lane);
    for (int slot = 0; slot < 2; ++slot) {
      Segment s;
      if (!long_segment<kLongRow>(rowptr, slot, rh, rt, e0, e1, s)) continue;  // (block-uniform)
      for (int pass = 0; pass < Lay::passes(passes); ++pass) {
        L.pass(pass);
        const int h = L.head(tid), cnt = L.cnt(s.se - s.sb);
        const float cx = op.ctx(s.r, h);
        const size_t at = (2 * (size_t)c + slot) * L.H + h;
        if constexpr (Op::SOFTMAX) {
          float mx = -INFINITY;
          for (int i = tid; i < cnt; i += 256) mx = fmaxf(mx, op.load(s.sb + L.off(i), h, cx).x);
          mx = block_hmax<MH>(mx, L.hp, sh);
          const float ms = safe_max(mx);
          float sum = 0.f;
          for (int i = tid; i < cnt; i += 256) sum += exps(op.load(s.sb + L.off(i), h, cx).x, ms);
          sum = block_hsum<MH>(sum, L.hp, sh);         // (relative to safe_max(mx))
          if (tid < L.hp) part[at] = make_float2(mx, sum);
        } else {                                       // (sums are carried in fp64: a partial is one double in the same 8 bytes)
          double t = 0.0;
          for (int i = tid; i < cnt; i += 256) t += term_of<Op>(op.load(s.sb + L.off(i), h, cx));
          t = block_hsum<MH>(t, L.hp, shd);
          if (tid < L.hp) reinterpret_cast<double*>(part)[at] = t;
        }
      }
    }
  }
}

template <class Op, class Lay>
__global__ void __launch_bounds__(256) edge_long_finish_kernel(Op op, Lay L, const int* __restrict__ rowptr, int m, int nnz,
                                                               int nchunks, const int* __restrict__ long_flag,
                                                               const float2* __restrict__ part) {
  if (*long_flag == 0) return;
  constexpr int MH = Lay::kMaxHp;
  __shared__ float sh[4 * MH];
  __shared__ double shd[4 * MH];
  const int tid = threadIdx.x, lane = tid & 63;
  const int H = L.H;
  const bool fast = L.hp == H;
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int e0 = c * kChunk;
    const int e1 = (long long)e0 + kChunk < nnz ? e0 + kChunk : nnz;
    const int rh = find_row(rowptr, m, e0, lane), rt = find_row(rowptr, m, e1 - 1, lane);
    for (int slot = 0; slot < 2; ++slot) {
      Segment s;
      if (!long_segment<kLongRow>(rowptr, slot, rh, rt, e0, e1, s)) continue;
      // the row's partials: chunks c_first..c_last, the first in slot 1 unless the row starts on the chunk's first entry.
      // Every block of the row merges the same partials in the same order, a head at a time (all 256 threads on that
      // head: thread t takes chunks t, t + 256, ..., then the block tree); on the fast route a thread keeps the result of
      // the head its elements belong to and the map follows the last head, on the slow route each head is mapped at once.
      const int c_first = s.rb / kChunk, c_last = (s.re - 1) / kChunk;
      const int first_slot = s.rb > c_first * kChunk ? 1 : 0;
      float my_ms = 0.f, my_inv = 0.f;
      double my_t = 0.0;
      for (int hh = 0; hh < H; ++hh) {
        if constexpr (Op::SOFTMAX) {
          float mx = -INFINITY;
          for (int cc = c_first + tid; cc <= c_last; cc += 256)
            mx = fmaxf(mx, part[(2 * (size_t)cc + (cc == c_first ? first_slot : 0)) * H + hh].x);
          const float ms = safe_max(block_hmax<MH>(mx, 1, sh));
          float sum = 0.f;
          for (int cc = c_first + tid; cc <= c_last; cc += 256) {
            const float2 q = part[(2 * (size_t)cc + (cc == c_first ? first_slot : 0)) * H + hh];
            sum += q.y * exps(safe_max(q.x), ms);      // one rescale per chunk (an all -inf chunk: 0 * exp(0 - ms))
          }
          const float inv = safe_inv(block_hsum<MH>(sum, 1, sh));
          if (!fast || (tid & (H - 1)) == hh) { my_ms = ms; my_inv = inv; }
        } else {
          double t = 0.0;
          for (int cc = c_first + tid; cc <= c_last; cc += 256)
            t += reinterpret_cast<const double*>(part)[(2 * (size_t)cc + (cc == c_first ? first_slot : 0)) * H + hh];
          t = block_hsum<MH>(t, 1, shd);
          if constexpr (!Op::MAP && Op::ROWOUT) {
            if (c == c_first && tid == 0) op.rowout(s.r, hh, (float)t);
          }
          if (!fast || (tid & (H - 1)) == hh) my_t = t;
        }
        if (fast && hh + 1 < H) continue;              // (block-uniform)
        if constexpr (Op::SOFTMAX || Op::MAP) {
          Lay M = L;
          M.pass(fast ? 0 : hh);
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

// the layout of a call and its passes over the rows: one head is its own layout, a power of two up to 16 the fast route
template <class Lay>
struct Route { Lay L; int passes; };
Route<HeadsLay> route_of(int H) {
  const bool fast = H <= kMaxFastHeads && (H & (H - 1)) == 0;
  int shift = 0;
  while (fast && (1 << shift) < H) ++shift;
  return {HeadsLay{H, shift, fast ? H : 1, 0}, fast ? 1 : H};
}
// f(route, heads): heads is what the operation of that route keeps as its H
template <class F>
hipError_t with_route(int H, F f) {
  if (H == 1) return f(Route<OneLay>{{}, 1}, One{});
  return f(route_of(H), H);
}

template <class Op, class Lay>
hipError_t run_rows(const Op& op, const Route<Lay>& rt, const int* rowptr, int m, int* flag, hipStream_t st) {
  const long long waves = ((long long)m + kRowsPerWave - 1) / kRowsPerWave;
  edge_rows_kernel<Op, Lay><<<(unsigned)((waves + 3) / 4), 256, 0, st>>>(op, rt.L, rt.passes, rowptr, m, flag);
  return hipGetLastError();
}

template <class Op, class Lay>
hipError_t run_long(const Op& op, const Route<Lay>& rt, const int* rowptr, int m, int nnz, void* ws, hipStream_t st) {
  if (nnz <= kLongRow) return hipSuccess;              // (no row can be long)
  int* flag = static_cast<int*>(ws);
  float2* part = reinterpret_cast<float2*>(static_cast<char*>(ws) + 16);
  const int nchunks = (int)(((long long)nnz + kChunk - 1) / kChunk);
  const int grid = nchunks < kLongGrid ? nchunks : kLongGrid;
  edge_long_partial_kernel<Op, Lay><<<grid, 256, 0, st>>>(op, rt.L, rt.passes, rowptr, m, nnz, nchunks, flag, part);
  edge_long_finish_kernel<Op, Lay><<<grid, 256, 0, st>>>(op, rt.L, rowptr, m, nnz, nchunks, flag, part);
  return hipGetLastError();
}

template <class Op, class Lay>
hipError_t run(const Op& op, const Route<Lay>& rt, const int* rowptr, int m, int nnz, void* ws, hipStream_t st) {
  int* flag = static_cast<int*>(ws);
  if (hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), st); e != hipSuccess) return e;
  if (hipError_t e = run_rows(op, rt, rowptr, m, flag, st); e != hipSuccess) return e;
  return run_long(op, rt, rowptr, m, nnz, ws, st);
}

}  // namespace

size_t edge_workspace_bytes(int nnz, int H) {
  return 16 + 16 * (size_t)H * (size_t)(((long long)nnz + kChunk - 1) / kChunk);
}

hipError_t launch_edge_softmax_heads(const int* rowptr, int m, int nnz, int H, const float* s, float* p, void* ws, hipStream_t st) {
  return with_route(H, [&](auto rt, auto heads) {
    return run(SoftmaxOp<decltype(heads)>{s, p, heads}, rt, rowptr, m, nnz, ws, st);
  });
}

hipError_t launch_edge_softmax_heads_backward(const int* rowptr, int m, int nnz, int H, const float* p, const float* g, float* ds,
                                              void* ws, hipStream_t st) {
  return with_route(H, [&](auto rt, auto heads) {
    return run(SoftmaxBwdOp<decltype(heads)>{p, g, ds, heads}, rt, rowptr, m, nnz, ws, st);
  });
}

hipError_t launch_gat_edge_softmax_heads(const int* rowptr, const int* col, int m, int nnz, int H, const float* a_dst,
                                         const float* a_src, float slope, float* p, void* ws, hipStream_t st) {
  return with_route(H, [&](auto rt, auto heads) {
    return run(GatSoftmaxOp<decltype(heads)>{col, a_dst, a_src, slope, p, heads}, rt, rowptr, m, nnz, ws, st);
  });
}

hipError_t launch_gat_edge_softmax_heads_backward(const int* rowptr, const int* col, int m, int nnz, int H, const float* a_dst,
                                                  const float* a_src, float slope, const float* p, const float* g, float* ds,
                                                  float* grad_a_dst, void* ws, hipStream_t st) {
  return with_route(H, [&](auto rt, auto heads) {
    using HT = decltype(heads);
    if (hipError_t e = run(GatSoftmaxBwdOp<HT>{col, a_dst, a_src, p, g, slope, ds, grad_a_dst, heads}, rt, rowptr, m, nnz, ws, st);
        e != hipSuccess)
      return e;
    // grad_a_dst of the long rows: the row kernel left them out, and their ds is complete only now — the long-row half of
    // a segment sum over ds (the flag still says whether there is such a row)
    return run_long(SegSumOp<HT>{ds, nullptr, grad_a_dst, heads}, rt, rowptr, m, nnz, ws, st);
  });
}

hipError_t launch_segment_sum_heads(const int* rowptr, int rows, int nnz, int H, const float* x, const int* perm, float* out,
                                    void* ws, hipStream_t st) {
  return with_route(H, [&](auto rt, auto heads) {
    return run(SegSumOp<decltype(heads)>{x, perm, out, heads}, rt, rowptr, rows, nnz, ws, st);
  });
}

// one head: the [nnz] arrays are the [nnz, 1] arrays
hipError_t launch_edge_softmax(const int* rowptr, int m, int nnz, const float* s, float* p, void* ws, hipStream_t st) {
  return launch_edge_softmax_heads(rowptr, m, nnz, 1, s, p, ws, st);
}

hipError_t launch_edge_softmax_backward(const int* rowptr, int m, int nnz, const float* p, const float* g, float* ds, void* ws,
                                        hipStream_t st) {
  return launch_edge_softmax_heads_backward(rowptr, m, nnz, 1, p, g, ds, ws, st);
}

hipError_t launch_gat_edge_softmax(const int* rowptr, const int* col, int m, int nnz, const float* a_dst, const float* a_src,
                                   float slope, float* p, void* ws, hipStream_t st) {
  return launch_gat_edge_softmax_heads(rowptr, col, m, nnz, 1, a_dst, a_src, slope, p, ws, st);
}

hipError_t launch_gat_edge_softmax_backward(const int* rowptr, const int* col, int m, int nnz, const float* a_dst,
                                            const float* a_src, float slope, const float* p, const float* g, float* ds,
                                            float* grad_a_dst, void* ws, hipStream_t st) {
  return launch_gat_edge_softmax_heads_backward(rowptr, col, m, nnz, 1, a_dst, a_src, slope, p, g, ds, grad_a_dst, ws, st);
}

hipError_t launch_segment_sum(const int* rowptr, int m, int nnz, const float* x, const int* perm, float* out, void* ws,
                              hipStream_t st) {
  return launch_segment_sum_heads(rowptr, m, nnz, 1, x, perm, out, ws, st);
}

}  // namespace gcn
