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
//    slot has 4 gathers and their 4 one-word value loads vals[e * H + head] in flight before the first fma.  Rows of
//    more than kAggChunk entries: chunk partials per (chunk, row, column), merged in chunk order by the wave whose chunk
//    holds the row's first entry.
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
#include <hip/hip_runtime.h>

#include <cstdint>

#include "long_chunks.h"
#include "spmm_kernels.h"

namespace gcn {
namespace {

constexpr int kRowsPerWave = 8;
constexpr int kGChunk = kAggChunk;                     // entries per chunk of the long-row route
constexpr int kGLong = kAggChunk;                      // rows longer than this are split over waves
constexpr int kGLongWaves = 8192;
constexpr int kMaxFastHeads = 16;

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
  for_long_segments<kGChunk, kGLong>(rowptr, rows, nnz, nchunks, wave, nwaves, lane, [&](int c, int slot, const Segment& sg) {
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
  });
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
  for_long_segments<kGChunk, kGLong>(rowptr, rows, nnz, nchunks, wave, nwaves, lane, [&](int c, int slot, const Segment& sg) {
    // one writer per row: the wave whose chunk holds the row's first entry merges the partials, in chunk order
    const int c_first = sg.rb / kGChunk, c_last = (sg.re - 1) / kGChunk;
    if (c != c_first) return;
    const int first_slot = sg.rb > c_first * kGChunk ? 1 : 0;
    for (int j = j0 + lane; j < j1; j += 64) {
      float acc = part[(2 * (size_t)c_first + first_slot) * a.k + j];
      for (int cc = c_first + 1; cc <= c_last; ++cc) acc += part[2 * (size_t)cc * a.k + j];
      a.out[(size_t)sg.r * a.k + j] = acc;
    }
  });
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
  for_long_segments<kGChunk, kGLong>(rowptr, m, nnz, nchunks, wave, nwaves, lane, [&](int c, int slot, const Segment& sg) {
    sddmm_entries<VEC>(s, sg.r, sg.sb, sg.se - sg.sb, lane);
  });
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

size_t heads_spmm_workspace_bytes(int nnz, int k) {
  return 16 + 8 * (size_t)k * (size_t)(((long long)nnz + kGChunk - 1) / kGChunk);
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
