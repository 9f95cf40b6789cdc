// edge_softmax.hip — softmax over the stored entries of every CSR row ("edge softmax"), its backward, the fused GAT score
// form of both, and plain CSR row sums of a per-entry array.  Everything works on the caller's CSR in entry order, takes
// no plan, only enqueues (one 4-byte memset node and kernels: legal inside a stream capture) and uses no atomics: every
// output has one writer and every sum a fixed order, so results are bit-identical from call to call.
//
// All five operations are "reduce a row, then map its entries with the result", and the host knows nothing about the row
// lengths (reading them would synchronise).  So ONE row kernel adapts per wave, and two chunk kernels take what a wave
// cannot:
//   * a wave owns 8 consecutive rows.  If all 8 have at most 32 entries, 8 lanes take each row (4 entries per lane in
//     registers; Cora-shaped rows of 1-5 entries, and millions of empty rows cost one rowptr load per 8 rows);
//   * otherwise the wave takes its rows one after the other with all 64 lanes: up to 1024 entries stay in registers
//     between the reduction and the map (4 or 16 per lane), so such a row is read once and written once;
//   * 1025..8192 entries are streamed: one touch per reduction and one for the map (the repeats hit L2: <= 32 KB a row);
//   * a row of more than kLongRow entries is left alone and a flag in the workspace is raised.  The chunk kernels
//     (a fixed grid walking chunks of kChunk = 8192 entries, returning at once while the flag is down) find the at most
//     two long rows that meet a chunk (the rows of its first and last entry: a 64-ary search of rowptr per wave), write
//     one partial per (chunk, row) to the workspace, and a second kernel merges a row's partials — every block the same
//     partials in the same order — and maps its chunk.  A row holding a whole 100 M-entry matrix is spread over the chip.
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
constexpr int kShortRow = 32;                          // 8 lanes x 4 entries
constexpr int kChunk = kEdgeChunk;                     // entries per block of the long-row kernels
constexpr int kLongRow = kEdgeChunk;                   // rows longer than this are split over blocks (>= kChunk: see below)
constexpr int kLongGrid = 2048;                        // blocks of the long-row kernels (they loop over the chunks)
constexpr float kLog2e = 1.4426950408889634f;

template <int G>
__device__ __forceinline__ float gmax(float v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, G));
  return v;
}
// (a butterfly: every lane of the group ends with the same bits)
template <int G, class T>
__device__ __forceinline__ T gsum(T v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, G);
  return v;
}

// exp(x - m) through v_exp_f32; -inf gives 0
__device__ __forceinline__ float exps(float x, float m) { return __builtin_amdgcn_exp2f((x - m) * kLog2e); }
// (the maximum of an all -inf row is -inf: subtracting it would make NaN of every entry)
__device__ __forceinline__ float safe_max(float m) { return m == -INFINITY ? 0.f : m; }
__device__ __forceinline__ float safe_inv(float s) { return s == 0.f ? 0.f : 1.0f / s; }

// ---- the operations ---------------------------------------------------------------------------------------------------
// load(e, c): what entry e contributes (c = ctx(r), a per-row value).  SOFTMAX ops reduce .x by (max, sum of exp) and
// store(e, p); the others reduce term(v) by a sum, then, with MAP, map(e, v, t, c) writes the entry's result and returns it
// to be summed again for rowout(r, .) (ROWOUT; without MAP rowout gets the first sum).
struct SoftmaxOp {
  static constexpr bool SOFTMAX = true;
  const float* s;
  float* p;
  __device__ float ctx(int) const { return 0.f; }
  __device__ float2 load(int e, float) const { return make_float2(s[e], 0.f); }
  __device__ void store(int e, float v) const { p[e] = v; }
};

struct GatSoftmaxOp {                                  // s[e] = leaky_relu(a_dst[row] + a_src[col[e]]), never stored
  static constexpr bool SOFTMAX = true;
  const int* col;
  const float *a_dst, *a_src;
  float slope;
  float* p;
  __device__ float ctx(int r) const { return a_dst[r]; }
  __device__ float2 load(int e, float c) const {
    const float t = c + a_src[col[e]];
    return make_float2(t > 0.f ? t : t * slope, 0.f);
  }
  __device__ void store(int e, float v) const { p[e] = v; }
};

struct SoftmaxBwdOp {                                  // ds = p (g - sum p g)
  static constexpr bool SOFTMAX = false, MAP = true, ROWOUT = false;
  const float *p, *g;
  float* ds;
  __device__ float ctx(int) const { return 0.f; }
  __device__ float2 load(int e, float) const { return make_float2(p[e], g[e]); }
  static __device__ double term(float2 v) { return (double)v.x * (double)v.y; }
  __device__ float map(int e, float2 v, double t, float) const {
    const float d = (float)((double)v.x * ((double)v.y - t));
    ds[e] = d;
    return d;
  }
  __device__ void rowout(int, float) const {}
};

struct GatSoftmaxBwdOp {                               // ds = p (g - sum p g) leaky_relu'(s_pre); grad_a_dst[r] = sum ds
  static constexpr bool SOFTMAX = false, MAP = true, ROWOUT = true;
  const int* col;
  const float *a_dst, *a_src, *p, *g;
  float slope;
  float *ds, *grad_a_dst;
  __device__ float ctx(int r) const { return a_dst[r]; }
  __device__ float2 load(int e, float) const { return make_float2(p[e], g[e]); }
  static __device__ double term(float2 v) { return (double)v.x * (double)v.y; }
  __device__ float map(int e, float2 v, double t, float c) const {
    const float pre = c + a_src[col[e]];
    const float d = (float)((double)v.x * ((double)v.y - t) * (double)(pre > 0.f ? 1.f : slope));   // (slope at 0, as torch's leaky_relu)
    ds[e] = d;
    return d;
  }
  __device__ void rowout(int r, float v) const { grad_a_dst[r] = v; }
};

struct SegSumOp {                                      // out[r] = sum x[e] (x[perm[e]] with a permutation)
  static constexpr bool SOFTMAX = false, MAP = false, ROWOUT = true;
  const float* x;
  const int* perm;
  float* out;
  __device__ float ctx(int) const { return 0.f; }
  __device__ float2 load(int e, float) const { return make_float2(x[perm ? perm[e] : e], 0.f); }
  static __device__ double term(float2 v) { return (double)v.x; }
  __device__ float map(int, float2, double, float) const { return 0.f; }
  __device__ void rowout(int r, float v) const { out[r] = v; }
};

template <class Op>
__device__ __forceinline__ float2 pad() { return make_float2(Op::SOFTMAX ? -INFINITY : 0.f, 0.f); }
template <class Op>
__device__ __forceinline__ double term_of(float2 v) {
  if constexpr (Op::SOFTMAX) return 0.0; else return Op::term(v);
}

// ---- a row of at most G*K entries [b, e) on a group of G lanes (gl = lane in the group): entries stay in registers ----
template <int G, int K, class Op>
__device__ __forceinline__ void row_cached(const Op& op, int r, bool row_ok, int b, int e, int gl) {
  const float c = row_ok ? op.ctx(r) : 0.f;
  float2 v[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const int off = gl + G * i;                        // (offsets from b: b + off is formed only below e, so never past INT_MAX)
    v[i] = off < e - b ? op.load(b + off, c) : pad<Op>();
  }
  if constexpr (Op::SOFTMAX) {
    float m = v[0].x;
#pragma unroll
    for (int i = 1; i < K; ++i) m = fmaxf(m, v[i].x);
    m = safe_max(gmax<G>(m));
    float ex[K], s = 0.f;
#pragma unroll
    for (int i = 0; i < K; ++i) {
      ex[i] = exps(v[i].x, m);
      s += ex[i];
    }
    const float inv = safe_inv(gsum<G, float>(s));
#pragma unroll
    for (int i = 0; i < K; ++i) {
      const int off = gl + G * i;
      if (off < e - b) op.store(b + off, ex[i] * inv);
    }
  } else {
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < K; ++i) t += term_of<Op>(v[i]);
    t = gsum<G, double>(t);
    double post = 0.0;
    if constexpr (Op::MAP) {
#pragma unroll
      for (int i = 0; i < K; ++i) {
        const int off = gl + G * i;
        if (off < e - b) post += op.map(b + off, v[i], t, c);
      }
      if constexpr (Op::ROWOUT) post = gsum<G, double>(post);
    }
    if constexpr (Op::ROWOUT)
      if (row_ok && gl == 0) op.rowout(r, (float)(Op::MAP ? post : t));
  }
}

// ---- a row of up to kLongRow entries on a whole wave, streamed: one touch per reduction, one for the map ----------------
template <class Op, class F>
__device__ __forceinline__ void for_entries4(int b, int e, int lane, F f) {   // four independent loads in flight
  const int n = e - b;                                 // (rows here have at most kLongRow entries: offsets cannot overflow)
  for (int base = lane; base < n; base += 256) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int off = base + 64 * u;
      if (off < n) f(b + off);
    }
  }
}

template <class Op>
__device__ __forceinline__ void row_stream(const Op& op, int r, int b, int e, int lane) {
  const float c = op.ctx(r);
  if constexpr (Op::SOFTMAX) {
    float m = -INFINITY;
    for_entries4<Op>(b, e, lane, [&](int idx) { m = fmaxf(m, op.load(idx, c).x); });
    m = safe_max(gmax<64>(m));
    float s = 0.f;
    for_entries4<Op>(b, e, lane, [&](int idx) { s += exps(op.load(idx, c).x, m); });
    const float inv = safe_inv(gsum<64, float>(s));
    for_entries4<Op>(b, e, lane, [&](int idx) { op.store(idx, exps(op.load(idx, c).x, m) * inv); });
  } else {
    double t = 0.0;
    for_entries4<Op>(b, e, lane, [&](int idx) { t += term_of<Op>(op.load(idx, c)); });
    t = gsum<64, double>(t);
    double post = 0.0;
    if constexpr (Op::MAP) {
      for_entries4<Op>(b, e, lane, [&](int idx) { post += op.map(idx, op.load(idx, c), t, c); });
      if constexpr (Op::ROWOUT) post = gsum<64, double>(post);
    }
    if constexpr (Op::ROWOUT)
      if (lane == 0) op.rowout(r, (float)(Op::MAP ? post : t));
  }
}

template <class Op>
__global__ void __launch_bounds__(256) edge_rows_kernel(Op op, const int* __restrict__ rowptr, int m, int* __restrict__ long_flag) {
  const int lane = threadIdx.x & 63;
  const long long wave = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
  if (wave * kRowsPerWave >= m) return;                // (whole waves leave: the shuffles below see full groups)
  const int r0 = (int)wave * kRowsPerWave;
  const int ri = r0 + lane < m ? r0 + lane : m;
  const int rp = rowptr[ri];                           // lanes 0..8: the 9 row bounds (later lanes repeat rowptr[m])
  const int len = __shfl_down(rp, 1) - rp;
  const bool all_short = __ballot(lane < kRowsPerWave && len > kShortRow) == 0;
  if (all_short) {
    const int g = lane >> 3;
    const int b = __shfl(rp, g), e = __shfl(rp, g + 1);
    row_cached<8, kShortRow / 8, Op>(op, r0 + g, r0 + g < m, b, e, lane & 7);
    return;
  }
  for (int j = 0; j < kRowsPerWave && r0 + j < m; ++j) {
    const int b = __shfl(rp, j), e = __shfl(rp, j + 1);
    const int n = e - b;
    if (n <= 256) row_cached<64, 4, Op>(op, r0 + j, true, b, e, lane);          // (n == 0: nothing but rowout(r, 0))
    else if (n <= 1024) row_cached<64, 16, Op>(op, r0 + j, true, b, e, lane);
    else if (n <= kLongRow) row_stream<Op>(op, r0 + j, b, e, lane);
    else if (lane == 0) *long_flag = 1;                // (every writer writes the same word)
  }
}

// ---- long rows (find_row, Segment and long_segment: long_chunks.h) --------------------------------------------------------
__device__ __forceinline__ float block_max(float v, float* sh) {
  v = gmax<64>(v);
  __syncthreads();                                     // (sh may still be read from the reduction before)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}
template <class T>
__device__ __forceinline__ T block_sum(T v, T* sh) {
  v = gsum<64, T>(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

template <class Op>
__global__ void __launch_bounds__(256) edge_long_partial_kernel(Op op, const int* __restrict__ rowptr, int m, int nnz, int nchunks,
                                                                const int* __restrict__ long_flag, float2* __restrict__ part) {
  if (*long_flag == 0) return;
  __shared__ float sh[4];
  __shared__ double shd[4];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int e0 = c * kChunk;
    const int e1 = (long long)e0 + kChunk < nnz ? e0 + kChunk : nnz;
    const int rh = find_row(rowptr, m, e0, lane), rt = find_row(rowptr, m, e1 - 1, lane);
    for (int slot = 0; slot < 2; ++slot) {
      Segment s;
      if (!long_segment<kLongRow>(rowptr, slot, rh, rt, e0, e1, s)) continue;  // (block-uniform)
      const float cx = op.ctx(s.r);
      if constexpr (Op::SOFTMAX) {
        float mx = -INFINITY;
        for (int off = tid; off < s.se - s.sb; off += 256) mx = fmaxf(mx, op.load(s.sb + off, cx).x);
        mx = block_max(mx, sh);
        const float ms = safe_max(mx);
        float sum = 0.f;
        for (int off = tid; off < s.se - s.sb; off += 256) sum += exps(op.load(s.sb + off, cx).x, ms);
        sum = block_sum(sum, sh);                      // (relative to safe_max(mx))
        if (tid == 0) part[2 * (size_t)c + slot] = make_float2(mx, sum);
      } else {                                         // (sums are carried in fp64: a partial is one double in the same 8 bytes)
        double t = 0.0;
        for (int off = tid; off < s.se - s.sb; off += 256) t += term_of<Op>(op.load(s.sb + off, cx));
        t = block_sum(t, shd);
        if (tid == 0) reinterpret_cast<double*>(part)[2 * (size_t)c + slot] = t;
      }
    }
  }
}

template <class Op>
__global__ void __launch_bounds__(256) edge_long_finish_kernel(Op op, const int* __restrict__ rowptr, int m, int nnz, int nchunks,
                                                               const int* __restrict__ long_flag, const float2* __restrict__ part) {
  if (*long_flag == 0) return;
  __shared__ float sh[4];
  __shared__ double shd[4];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int e0 = c * kChunk;
    const int e1 = (long long)e0 + kChunk < nnz ? e0 + kChunk : nnz;
    const int rh = find_row(rowptr, m, e0, lane), rt = find_row(rowptr, m, e1 - 1, lane);
    for (int slot = 0; slot < 2; ++slot) {
      Segment s;
      if (!long_segment<kLongRow>(rowptr, slot, rh, rt, e0, e1, s)) continue;
      // the row's partials: chunks c_first..c_last, the first in slot 1 unless the row starts on the chunk's first entry.
      // Every block of the row merges the same partials in the same order: thread t takes t, t + 256, ..., then the block tree.
      const int c_first = s.rb / kChunk, c_last = (s.re - 1) / kChunk;
      const int first_slot = s.rb > c_first * kChunk ? 1 : 0;
      const float cx = op.ctx(s.r);
      if constexpr (Op::SOFTMAX) {
        float mx = -INFINITY;
        for (int cc = c_first + tid; cc <= c_last; cc += 256)
          mx = fmaxf(mx, part[2 * (size_t)cc + (cc == c_first ? first_slot : 0)].x);
        const float ms = safe_max(block_max(mx, sh));
        float sum = 0.f;
        for (int cc = c_first + tid; cc <= c_last; cc += 256) {
          const float2 q = part[2 * (size_t)cc + (cc == c_first ? first_slot : 0)];
          sum += q.y * exps(safe_max(q.x), ms);        // one rescale per chunk (an all -inf chunk: 0 * exp(0 - ms))
        }
        const float inv = safe_inv(block_sum(sum, sh));
        for (int off = tid; off < s.se - s.sb; off += 256) op.store(s.sb + off, exps(op.load(s.sb + off, cx).x, ms) * inv);
      } else {
        double t = 0.0;
        for (int cc = c_first + tid; cc <= c_last; cc += 256)
          t += reinterpret_cast<const double*>(part)[2 * (size_t)cc + (cc == c_first ? first_slot : 0)];
        t = block_sum(t, shd);
        if constexpr (Op::MAP) {
          for (int off = tid; off < s.se - s.sb; off += 256) op.map(s.sb + off, op.load(s.sb + off, cx), t, cx);
        } else if constexpr (Op::ROWOUT) {
          if (c == c_first && tid == 0) op.rowout(s.r, (float)t);
        }
      }
    }
  }
}

template <class Op>
hipError_t run_rows(const Op& op, const int* rowptr, int m, int* flag, hipStream_t st) {
  const long long waves = ((long long)m + kRowsPerWave - 1) / kRowsPerWave;
  edge_rows_kernel<Op><<<(unsigned)((waves + 3) / 4), 256, 0, st>>>(op, rowptr, m, flag);
  return hipGetLastError();
}

template <class Op>
hipError_t run_long(const Op& op, const int* rowptr, int m, int nnz, int* flag, float2* part, hipStream_t st) {
  if (nnz <= kLongRow) return hipSuccess;              // (no row can be long)
  const int nchunks = (int)(((long long)nnz + kChunk - 1) / kChunk);
  const int grid = nchunks < kLongGrid ? nchunks : kLongGrid;
  edge_long_partial_kernel<Op><<<grid, 256, 0, st>>>(op, rowptr, m, nnz, nchunks, flag, part);
  edge_long_finish_kernel<Op><<<grid, 256, 0, st>>>(op, rowptr, m, nnz, nchunks, flag, part);
  return hipGetLastError();
}

template <class Op>
hipError_t run(const Op& op, const int* rowptr, int m, int nnz, void* ws, hipStream_t st) {
  int* flag = static_cast<int*>(ws);
  float2* part = reinterpret_cast<float2*>(static_cast<char*>(ws) + 16);
  if (hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), st); e != hipSuccess) return e;
  if (hipError_t e = run_rows(op, rowptr, m, flag, st); e != hipSuccess) return e;
  return run_long(op, rowptr, m, nnz, flag, part, st);
}

}  // namespace

size_t edge_workspace_bytes(int nnz) { return 16 + 16 * (size_t)(((long long)nnz + kChunk - 1) / kChunk); }

hipError_t launch_edge_softmax(const int* rowptr, int m, int nnz, const float* s, float* p, void* ws, hipStream_t st) {
  return run(SoftmaxOp{s, p}, rowptr, m, nnz, ws, st);
}

hipError_t launch_edge_softmax_backward(const int* rowptr, int m, int nnz, const float* p, const float* g, float* ds, void* ws,
                                        hipStream_t st) {
  return run(SoftmaxBwdOp{p, g, ds}, rowptr, m, nnz, ws, st);
}

hipError_t launch_gat_edge_softmax(const int* rowptr, const int* col, int m, int nnz, const float* a_dst, const float* a_src,
                                   float slope, float* p, void* ws, hipStream_t st) {
  return run(GatSoftmaxOp{col, a_dst, a_src, slope, p}, rowptr, m, nnz, ws, st);
}

hipError_t launch_gat_edge_softmax_backward(const int* rowptr, const int* col, int m, int nnz, const float* a_dst,
                                            const float* a_src, float slope, const float* p, const float* g, float* ds,
                                            float* grad_a_dst, void* ws, hipStream_t st) {
  int* flag = static_cast<int*>(ws);
  float2* part = reinterpret_cast<float2*>(static_cast<char*>(ws) + 16);
  if (hipError_t e = run(GatSoftmaxBwdOp{col, a_dst, a_src, p, g, slope, ds, grad_a_dst}, rowptr, m, nnz, ws, st); e != hipSuccess)
    return e;
  // grad_a_dst of the long rows: the row kernel left them out, and their ds is complete only now — the long-row half of a
  // segment sum over ds (the flag still says whether there is such a row)
  return run_long(SegSumOp{ds, nullptr, grad_a_dst}, rowptr, m, nnz, flag, part, st);
}

hipError_t launch_segment_sum(const int* rowptr, int m, int nnz, const float* x, const int* perm, float* out, void* ws,
                              hipStream_t st) {
  return run(SegSumOp{x, perm, out}, rowptr, m, nnz, ws, st);
}

}  // namespace gcn
