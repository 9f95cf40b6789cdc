// segment_mm.hip — the gathered, segmented matrix product on the matrix cores:
//
//   forward      y[i, :]  = scale[i] * ( x[xi(i), :] @ op(W[t(i)]) )          t(i): segptr[t] <= i < segptr[t + 1]
//   weight grad  dW[t]    = sum over the rows i of segment t of  scale[i] * x[xi(i), :]^T (x) g[gi(i), :]
//
// fp32 throughout, on v_mfma_f32_32x32x2_f32 (exact fp32: an fma chain over ascending k, the instruction of
// spmm_panel_dense_mfma_kernel, whose fragment layout is used here).  Three kernels and no host read:
//
//  * segmm_prefix_kernel (one workgroup) makes the segment bounds monotone — e[s] = the running maximum of segptr clamped to
//    [0, N], so a decreasing pointer is an empty segment and the segments never overlap — puts the rows in front of
//    segptr[0] and behind segptr[T] into two pseudo-segments (their tiles store zeros), and scans the tiles and the chunks per
//    segment into the workspace.
//  * segmm_forward_kernel: a workgroup of 4 waves owns 64 rows of ONE segment x 64 output columns, each wave one 32 x 32
//    block.  The grid is ceil(N / 64) + T + 2 in x (an upper bound on the tiles: a segment wastes less than one tile), and a
//    workgroup finds its (segment, tile) by a binary search of the tile prefix; the surplus exits.  K runs in chunks of 32:
//    the gathered A rows [64][32] and the slab of W[t] ([32][64], or [64][32] of the transposed form) go through registers
//    into LDS, and the global loads of chunk c + 1 are issued before the MFMAs of chunk c.
//  * segmm_wgrad_kernel: the rows are the contraction.  A workgroup owns (chunk of 512 rows of one segment, 64 of K, 64 of O),
//    stages 32 gathered rows of x (scaled) and of g per step, and writes its [64, 64] block of the chunk's partial — or of
//    dW[t] itself when the segment is one chunk.  segmm_wgrad_reduce_kernel adds a longer segment's partials in chunk order
//    and zeroes an empty segment's dW.
//
// LDS layouts.  The fragment reads are A[l % 32][2 j + l / 32] and B[2 j + l / 32][l % 32] (l the lane).  A tile stored
// k-major ([k][64 columns], the forward's W slab and both operands of the weight gradient) has a row stride of 96 floats:
// lanes 0-31 read 32 consecutive words, lanes 32-63 the same 32 columns one row on, 96 = 32 (mod 64) words away, so the 64
// lanes hit 64 different banks.  A tile stored row-major in k ([row][32 of k], the gathered A rows and the transposed W
// slab, whose global rows run along k) has a stride of 33: odd, so 32 rows at one k are 32 different banks.
// Zero padding: rows past the segment's end, k >= K and columns >= O are zeros in LDS on BOTH operands; a padded row or
// column only feeds outputs that are never stored, and in the k tail 0 * 0 = 0, so no 0 * Inf reaches a stored value.
// A non-finite row of x therefore reaches its own rows of y only, a non-finite W[t] segment t only.
// Loads are 16 bytes where the pointer is 16-byte aligned and the row stride a multiple of 4 floats, else
// 4 bytes with the same values.  Row offsets are 64-bit.  No atomics; every output element has one writer.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "segment_mm.h"

namespace gcn {

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int kKC = 32;                                // k of one staged chunk (forward); rows of one step (weight gradient)
constexpr int kSA = kKC + 1;                           // stride of a tile that is row-major in k
constexpr int kSB = 96;                                // stride of a k-major tile of 64 columns

__host__ __device__ inline int seg_ws_ints(int T) { return 3 * T + 7; }
__host__ __device__ inline size_t seg_ws_head_bytes(int T) { return ((size_t)seg_ws_ints(T) * 4 + 15) / 16 * 16; }

// inclusive scan of one value per thread of a 256-thread workgroup (maximum or sum); s: 4 ints of LDS
template <bool MAX>
__device__ inline int block_scan(int v, int* s, int tid) {
  const int lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d, 64);
    if (lane >= d) v = MAX ? max(v, o) : v + o;
  }
  if (lane == 63) s[w] = v;
  __syncthreads();
  for (int u = 0; u < w; ++u) v = MAX ? max(v, s[u]) : v + s[u];
  __syncthreads();
  return v;
}

// ws ints: e [T + 3] (e[0] = 0, e[1 + s] = the monotone segptr[s], e[T + 2] = N: T + 2 pseudo-segments, the first and the
// last the uncovered rows), tp [T + 3] (tiles of kSegTM rows in front of pseudo-segment p; tp[T + 2] = all), cp [T + 1] (chunks
// of kSegChunk rows in front of segment t; cp[T] = all)
__global__ void __launch_bounds__(256) segmm_prefix_kernel(const int* __restrict__ segptr, int N, int T, int* __restrict__ ws) {
  __shared__ int s[4];
  __shared__ int carry[2];
  int* e = ws;
  int* tp = ws + (T + 3);
  int* cp = ws + 2 * (T + 3);
  const int tid = threadIdx.x;
  int top = 0;
  for (int base = 0; base <= T; base += 256) {
    const int i = base + tid;
    int v = i <= T ? min(max(segptr[i], 0), N) : 0;
    v = max(block_scan<true>(v, s, tid), top);
    if (i <= T) e[1 + i] = v;
    if (tid == 255) carry[0] = v;
    __syncthreads();
    top = carry[0];
  }
  if (tid == 0) {
    e[0] = 0;
    e[T + 2] = N;
  }
  __syncthreads();
  const int P = T + 2;
  int tiles = 0, chunks = 0;
  for (int base = 0; base < P; base += 256) {
    const int p = base + tid;
    const int len = p < P ? e[p + 1] - e[p] : 0;
    const int nt = (len + kSegTM - 1) / kSegTM;
    const int nc = p >= 1 && p <= T ? (len + kSegChunk - 1) / kSegChunk : 0;
    const int it = block_scan<false>(nt, s, tid) + tiles, ic = block_scan<false>(nc, s, tid) + chunks;
    if (p < P) {
      tp[p] = it - nt;
      if (p >= 1) cp[p - 1] = ic - nc;                 // (p = T + 1, the rows behind: cp[T], every chunk)
    }
    if (tid == 255) {
      carry[0] = it;
      carry[1] = ic;
    }
    __syncthreads();
    tiles = carry[0];
    chunks = carry[1];
  }
  if (tid == 0) tp[P] = tiles;
}

// four consecutive floats from p, of which `have` exist (<= 0: none; p may be null: a row of zeros); vec: one 16-byte load
// (the caller's rule: p is 16-byte aligned and have is a multiple of 4)
__device__ inline float4 load_quad(const float* p, int have, bool vec) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (p && have > 0) {
    if (vec) {
      v = *reinterpret_cast<const float4*>(p);
    } else {
      v.x = p[0];
      if (have > 1) v.y = p[1];
      if (have > 2) v.z = p[2];
      if (have > 3) v.w = p[3];
    }
  }
  return v;
}

__device__ inline void store_quad_elems(float* p, const float4& v) {
  p[0] = v.x;
  p[1] = v.y;
  p[2] = v.z;
  p[3] = v.w;
}

// the largest p in [0, count) with prefix[p] <= b, given prefix[0] <= b < prefix[count]
__device__ inline int find_owner(const int* __restrict__ prefix, int count, int b) {
  int lo = 0, hi = count;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

// C/D layout of the 32 x 32 forms: column = lane % 32, row = (reg % 4) + 8 (reg / 4) + 4 (lane / 32)
__device__ inline int frag_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

template <bool TRANS>
__global__ void __launch_bounds__(256)
segmm_forward_kernel(const float* __restrict__ x, int x_rows, const int* __restrict__ x_index, const float* __restrict__ scale,
                     const float* __restrict__ W, float* __restrict__ y, const int* __restrict__ ws, int T, int K, int O,
                     int vec_a, int vec_b) {
  __shared__ float As[kSegTM * kSA];
  __shared__ __attribute__((aligned(16))) float Bs[TRANS ? kSegTN * kSA : kKC * kSB];
  const int* e = ws;
  const int* tp = ws + (T + 3);
  const int P = T + 2;
  const int b = blockIdx.x;
  if (b >= tp[P]) return;                               // the surplus of the grid's upper bound
  const int p = find_owner(tp, P, b);
  const int row0 = e[p] + (b - tp[p]) * kSegTM, row_end = e[p + 1];
  const int col0 = blockIdx.y * kSegTN;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (p == 0 || p == P - 1) {                           // rows no segment covers: zeros
    for (int s = tid; s < kSegTM * kSegTN; s += 256) {
      const int r = row0 + s / kSegTN, c = col0 + s % kSegTN;
      if (r < row_end && c < O) y[(size_t)r * O + c] = 0.f;
    }
    return;
  }
  const float* Wt = W + (size_t)(p - 1) * K * O;

  // what this thread stages: two quads of A (rows tid / 8 and + 32, k offset 4 (tid % 8)) and two quads of the W slab
  const int ar = tid >> 3, ak = (tid & 7) * 4;
  const float* arow[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int i = row0 + ar + 32 * u;
    arow[u] = nullptr;
    if (i < row_end) {
      const int src = x_index ? x_index[i] : i;
      if ((unsigned)src < (unsigned)x_rows) arow[u] = x + (size_t)src * K;
    }
  }
  const int bk = tid >> 4, bc = (tid & 15) * 4;         // plain W: slab rows tid / 16 and + 16, columns 4 (tid % 16) ..
  float4 ra[2], rb[2];
  auto load_chunk = [&](int k0) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      ra[u] = load_quad(arow[u] ? arow[u] + k0 + ak : nullptr, K - (k0 + ak), vec_a);
      if (TRANS) {                                      // W[t] is [O, K]: the slab's rows are output columns, read along k
        const int c = col0 + ar + 32 * u;
        rb[u] = load_quad(c < O ? Wt + (size_t)c * K + k0 + ak : nullptr, K - (k0 + ak), vec_b);
      } else {
        const int k = k0 + bk + 16 * u;
        rb[u] = load_quad(k < K ? Wt + (size_t)k * O + col0 + bc : nullptr, O - (col0 + bc), vec_b);
      }
    }
  };
  const int ib = w & 1, nb = w >> 1;
  const bool active = row0 + ib * 32 < row_end && col0 + nb * 32 < O;       // (a wave without stored outputs only stages)
  const float* ap = As + (ib * 32 + (lane & 31)) * kSA + (lane >> 5);
  const float* bp = TRANS ? Bs + (nb * 32 + (lane & 31)) * kSA + (lane >> 5) : Bs + (lane >> 5) * kSB + nb * 32 + (lane & 31);
  f32x16 acc = {0};
  load_chunk(0);
  for (int k0 = 0; k0 < K; k0 += kKC) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      store_quad_elems(As + (ar + 32 * u) * kSA + ak, ra[u]);
      if (TRANS) store_quad_elems(Bs + (ar + 32 * u) * kSA + ak, rb[u]);
      else *reinterpret_cast<float4*>(Bs + (bk + 16 * u) * kSB + bc) = rb[u];
    }
    __syncthreads();
    if (k0 + kKC < K) load_chunk(k0 + kKC);             // in flight under the MFMAs below
    if (active) {
#pragma unroll
      for (int j = 0; j < kKC / 2; ++j)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * j], TRANS ? bp[2 * j] : bp[2 * j * kSB], acc, 0, 0, 0);
    }
    __syncthreads();
  }
  if (!active) return;
  const int c = col0 + nb * 32 + (lane & 31);
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int i = row0 + ib * 32 + frag_row(reg, lane);
    if (i < row_end && c < O) y[(size_t)i * O + c] = scale ? scale[i] * acc[reg] : acc[reg];
  }
}

__global__ void __launch_bounds__(256)
segmm_wgrad_kernel(const float* __restrict__ x, int x_rows, const int* __restrict__ x_index, const float* __restrict__ g,
                   int g_rows, const int* __restrict__ g_index, const float* __restrict__ scale, float* __restrict__ dW,
                   const int* __restrict__ ws, float* __restrict__ partial, int T, int K, int O, int vec_x, int vec_g) {
  __shared__ __attribute__((aligned(16))) float Xs[kKC * kSB];
  __shared__ __attribute__((aligned(16))) float Gs[kKC * kSB];
  const int* e = ws;
  const int* cp = ws + 2 * (T + 3);
  const int b = blockIdx.x;
  if (b >= cp[T]) return;
  const int t = find_owner(cp, T, b);
  const int r0 = e[1 + t] + (b - cp[t]) * kSegChunk, r_end = min(r0 + kSegChunk, e[2 + t]);
  const size_t KO = (size_t)K * O;
  float* dst = cp[t + 1] - cp[t] == 1 ? dW + (size_t)t * KO : partial + (size_t)b * KO;
  const int k0 = blockIdx.y * kSegTN, o0 = blockIdx.z * kSegTN;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int sr = tid >> 4, sq = (tid & 15) * 4;         // staged: rows tid / 16 and + 16 of the step, columns 4 (tid % 16) ..
  float4 rx[2], rg[2];
  auto load_step = [&](int rs) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = rs + sr + 16 * u;
      const float* xp = nullptr;
      const float* gp = nullptr;
      float sc = 1.f;
      if (i < r_end) {
        const int sx = x_index ? x_index[i] : i, sg = g_index ? g_index[i] : i;
        if ((unsigned)sx < (unsigned)x_rows) xp = x + (size_t)sx * K + k0 + sq;
        if ((unsigned)sg < (unsigned)g_rows) gp = g + (size_t)sg * O + o0 + sq;
        if (scale) sc = scale[i];
      }
      rx[u] = load_quad(xp, K - (k0 + sq), vec_x);
      rg[u] = load_quad(gp, O - (o0 + sq), vec_g);
      if (scale && xp) {
        rx[u].x *= sc;
        rx[u].y *= sc;
        rx[u].z *= sc;
        rx[u].w *= sc;
      }
    }
  };
  const int ib = w & 1, nb = w >> 1;
  const bool active = k0 + ib * 32 < K && o0 + nb * 32 < O;
  const float* ap = Xs + (lane >> 5) * kSB + ib * 32 + (lane & 31);
  const float* bp = Gs + (lane >> 5) * kSB + nb * 32 + (lane & 31);
  f32x16 acc = {0};
  load_step(r0);
  for (int rs = r0; rs < r_end; rs += kKC) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      *reinterpret_cast<float4*>(Xs + (sr + 16 * u) * kSB + sq) = rx[u];
      *reinterpret_cast<float4*>(Gs + (sr + 16 * u) * kSB + sq) = rg[u];
    }
    __syncthreads();
    if (rs + kKC < r_end) load_step(rs + kKC);
    if (active) {
#pragma unroll
      for (int j = 0; j < kKC / 2; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * j * kSB], bp[2 * j * kSB], acc, 0, 0, 0);
    }
    __syncthreads();
  }
  if (!active) return;
  const int c = o0 + nb * 32 + (lane & 31);
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int k = k0 + ib * 32 + frag_row(reg, lane);
    if (k < K && c < O) dst[(size_t)k * O + c] = acc[reg];
  }
}

// dW[t] of every segment that is not exactly one chunk: its partials added in chunk order; no chunk, zeros
__global__ void __launch_bounds__(256)
segmm_wgrad_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dW, const int* __restrict__ ws, int T, int KO) {
  const int* cp = ws + 2 * (T + 3);
  const int el = blockIdx.x * 256 + threadIdx.x;
  if (el >= KO) return;
  for (int t = blockIdx.y; t < T; t += gridDim.y) {
    const int c0 = cp[t], c1 = cp[t + 1];
    if (c1 - c0 == 1) continue;
    float s = 0.f;
    for (int c = c0; c < c1; ++c) s += partial[(size_t)c * KO + el];
    dW[(size_t)t * KO + el] = s;
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

size_t segment_mm_workspace_bytes(int N, int T, int K, int O) {
  const size_t chunks = (size_t)((N + kSegChunk - 1) / kSegChunk) + (size_t)T;
  return seg_ws_head_bytes(T) + chunks * (size_t)K * (size_t)O * sizeof(float);
}

hipError_t launch_segment_mm(const float* x, int x_rows, const int* x_index, const float* scale, const int* segptr,
                             const float* W, int transpose_w, int N, int T, int K, int O, float* y, void* ws, hipStream_t st) {
  int* wi = static_cast<int*>(ws);
  segmm_prefix_kernel<<<dim3(1), dim3(256), 0, st>>>(segptr, N, T, wi);
  const dim3 grid((unsigned)((N + kSegTM - 1) / kSegTM + T + 2), (unsigned)((O + kSegTN - 1) / kSegTN));
  const int vec_a = aligned16(x) && K % 4 == 0;
  if (transpose_w)
    segmm_forward_kernel<true><<<grid, dim3(256), 0, st>>>(x, x_rows, x_index, scale, W, y, wi, T, K, O, vec_a,
                                                            aligned16(W) && K % 4 == 0);
  else
    segmm_forward_kernel<false><<<grid, dim3(256), 0, st>>>(x, x_rows, x_index, scale, W, y, wi, T, K, O, vec_a,
                                                             aligned16(W) && O % 4 == 0);
  return hipGetLastError();
}

hipError_t launch_segment_mm_wgrad(const float* x, int x_rows, const int* x_index, const float* g, int g_rows,
                                   const int* g_index, const float* scale, const int* segptr, int N, int T, int K, int O,
                                   float* dW, void* ws, hipStream_t st) {
  int* wi = static_cast<int*>(ws);
  float* partial = reinterpret_cast<float*>(static_cast<char*>(ws) + seg_ws_head_bytes(T));
  segmm_prefix_kernel<<<dim3(1), dim3(256), 0, st>>>(segptr, N, T, wi);
  const dim3 grid((unsigned)((N + kSegChunk - 1) / kSegChunk + T), (unsigned)((K + kSegTN - 1) / kSegTN),
                  (unsigned)((O + kSegTN - 1) / kSegTN));
  segmm_wgrad_kernel<<<grid, dim3(256), 0, st>>>(x, x_rows, x_index, g, g_rows, g_index, scale, dW, wi, partial, T, K, O,
                                                 aligned16(x) && K % 4 == 0, aligned16(g) && O % 4 == 0);
  const int KO = K * O;
  segmm_wgrad_reduce_kernel<<<dim3((unsigned)((KO + 255) / 256), (unsigned)(T < 4096 ? T : 4096)), dim3(256), 0, st>>>(
      partial, dW, wi, T, KO);
  return hipGetLastError();
}

}  // namespace gcn
