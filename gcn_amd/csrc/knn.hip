// knn.hip — brute-force k nearest neighbours: for every fp32 query row the k candidate rows of smallest squared Euclidean
// distance, with the q x n distance matrix never written to memory (the contract is in include/gcn_spmm.h, gcn_knn_f32;
// tests/knn_ref.py is the numpy twin).
//
// DISTANCE.  One fp32 accumulator per pair, starting at 0, columns in ascending order: diff = x_ic - y_jc, acc = fmaf(diff,
// diff, acc).  A thread keeps a 4 x 4 block of a 64 x 64 distance tile in registers while the feature columns stream through
// LDS in chunks of 32, so the per-pair column order costs nothing and the value is a pure function of the two rows: it does
// not depend on the tile, the split or the launch shape, d2(a, a) is exactly 0 and d2(a, b) has the bits of d2(b, a).
// Columns past d and rows past the operand are staged as zeros: fmaf(0, 0, acc) returns acc.
//
// ORDER.  A candidate's key is (fp32 bits of d2) << 32 | j, NaN of either sign mapped to the bits 0x7fc00000: non-negative
// floats order as unsigned integers, NaN ranks behind +inf, and equal distances order by index.  Keys are unique, so the k
// smallest are a unique set and no step below depends on the order in which keys arrive.
//
// SELECTION.  A wave owns 16 of the workgroup's 64 queries (its threads hold exactly their distance blocks), so selection
// needs no workgroup barrier.  Every query has a buffer of k + 64 keys in LDS, a counter and a threshold: the k-th smallest
// key seen so far, all ones until a compaction has seen k.  After a tile a thread appends the keys below the threshold (the
// position comes from an LDS integer counter).  A buffer holding more than k keys is compacted by its wave before the next
// tile, which may append 64: every key is ranked by counting the smaller ones (ranks are a permutation of 0 .. count - 1),
// the keys of rank < k move to their rank, and the threshold drops to the key of rank k - 1.  The same step sorts the final k.
//
// SPLITS.  The candidate tiles are cut into `splits` contiguous ranges; workgroup (query block, part) writes its k smallest
// keys and, on request, its part of the row sum to the workspace, and knn_merge_kernel, a wave per query, selects the k
// smallest of the splits * k keys with the same buffer step and adds the partial sums in part order.
//
// ROW SUM.  sum_j sqrt((double) d2_ij) over all n candidates: a thread adds its 4 distances of a row in column order, the 16
// threads of the row are added by a fixed shuffle tree, and the tile's sum is added to the running fp64 sum of the row.  The
// order depends on nothing but `splits` (a part's tiles are added first, then the parts).
//
// Every global access is a 4- or 8-byte one at its natural alignment: operands need 4-byte alignment and any row stride >= d.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "spmm_kernels.h"

namespace gcn {
namespace {

typedef unsigned long long u64;

constexpr int kChunk = 32;                             // feature columns staged at a time
constexpr int kLd = kKnnTileQ + 4;                     // floats per staged column: 16-byte aligned rows, 4 banks of skew
constexpr int kStage = kChunk * kLd;                   // floats of one staged tile
constexpr u64 kEmpty = ~0ull;                          // no candidate: index -1, distance +inf
static_assert(kKnnTileQ == 64 && kKnnTileC == 64 && kKnnKMax <= 64, "the 16 x 16 thread grid and the two-keys-per-lane compaction");

struct KnnArgs {
  const float* x;
  const float* y;
  long long ldx, ldy;
  int q, n, d, k, self_offset, splits;
  u64* part_keys;                                      // [q][splits][k]
  double* part_sum;                                    // [q][splits]
  int* out_idx;
  float* out_dist2;
  double* out_sum;
};

// a wave's steps on LDS are ordered by keeping the compiler from moving the accesses (spgemm.hip's unit_sync)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ u64 make_key(float d2, long long j) {
  unsigned bits = __float_as_uint(d2);
  if (d2 != d2) bits = 0x7fc00000u;
  return ((u64)bits << 32) | (u64)(unsigned)j;
}

// One wave: the cnt (<= k + 64 <= 128) unique keys of buf are reduced to the min(cnt, k) smallest, ascending.  Returns the
// new count.  cnt is wave-uniform.
__device__ __forceinline__ int compact(u64* buf, int cnt, int k, int lane) {
  const u64 k0 = lane < cnt ? buf[lane] : kEmpty;
  const u64 k1 = lane + 64 < cnt ? buf[lane + 64] : kEmpty;
  int r0 = 0, r1 = 0;
  for (int j = 0; j < cnt; ++j) {
    const u64 v = buf[j];
    r0 += v < k0;
    r1 += v < k1;
  }
  wave_sync();
  if (lane < cnt && r0 < k) buf[r0] = k0;
  if (lane + 64 < cnt && r1 < k) buf[r1] = k1;
  wave_sync();
  return cnt < k ? cnt : k;
}

template <bool WANT_SUM>
__global__ void __launch_bounds__(256) knn_tile_kernel(KnnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int cap = a.k + kKnnTileC;
  float* xs = reinterpret_cast<float*>(smem);          // [2][kChunk][kLd]: column-major tiles, two buffers
  float* ys = xs + 2 * kStage;
  u64* keys = reinterpret_cast<u64*>(ys + 2 * kStage); // [64][cap]
  u64* thr = keys + (size_t)kKnnTileQ * cap;           // [64]
  int* cnt = reinterpret_cast<int*>(thr + kKnnTileQ);  // [64]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ty = tid >> 4, tx = tid & 15;
  const int part = (int)(blockIdx.x % (unsigned)a.splits);
  const long long q0 = (long long)(blockIdx.x / (unsigned)a.splits) * kKnnTileQ;
  const long long tiles = ((long long)a.n + kKnnTileC - 1) / kKnnTileC;
  const long long t_begin = (long long)part * tiles / a.splits, t_end = ((long long)part + 1) * tiles / a.splits;
  const int nch = (a.d + kChunk - 1) / kChunk;

  if (tid < kKnnTileQ) {
    thr[tid] = kEmpty;
    cnt[tid] = 0;
  }

  float px[8], py[8];
  auto gload = [&](long long tile, int ch) {
    const int c0 = ch * kChunk;
    const long long j0 = tile * kKnnTileC;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int e = tid + 256 * i, r = e >> 5, col = c0 + (e & 31);
      px[i] = (q0 + r < a.q && col < a.d) ? a.x[(size_t)(q0 + r) * (size_t)a.ldx + col] : 0.0f;
      py[i] = (j0 + r < a.n && col < a.d) ? a.y[(size_t)(j0 + r) * (size_t)a.ldy + col] : 0.0f;
    }
  };
  auto lstore = [&](int b) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int e = tid + 256 * i, r = e >> 5, c = e & 31;
      xs[b * kStage + c * kLd + r] = px[i];
      ys[b * kStage + c * kLd + r] = py[i];
    }
  };

  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
  double rowsum[4] = {0.0, 0.0, 0.0, 0.0};             // (meaningful in the threads with tx == 0)

  long long tile = t_begin;
  int ch = 0, b = 0;
  if (tile < t_end) {
    gload(tile, 0);
    lstore(0);
  }
  __syncthreads();
  while (tile < t_end) {
    long long ntile = tile;
    int nc = ch + 1;
    if (nc == nch) {
      nc = 0;
      ++ntile;
    }
    const bool more = ntile < t_end;
    if (more) gload(ntile, nc);
    {
      const int c0 = ch * kChunk;
      const int cw = a.d - c0 < kChunk ? a.d - c0 : kChunk;
      const float* xb = xs + b * kStage + ty * 4;
      const float* yb = ys + b * kStage + tx * 4;
#pragma unroll 4
      for (int c = 0; c < cw; ++c) {
        const float4 xv = *reinterpret_cast<const float4*>(xb + c * kLd);
        const float4 yv = *reinterpret_cast<const float4*>(yb + c * kLd);
        const float xa[4] = {xv.x, xv.y, xv.z, xv.w}, ya[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float diff = xa[i] - ya[j];
            acc[i][j] = __builtin_fmaf(diff, diff, acc[i][j]);
          }
      }
    }
    if (more) lstore(b ^ 1);
    if (nc == 0) {                                     // the tile is complete: its keys, its part of the sums, a fresh block
      const long long j0 = tile * kKnnTileC + tx * 4;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int qi = ty * 4 + i;
        const long long row = q0 + qi;
        if (row < a.q) {
          const u64 t = thr[qi];
          const long long self = a.self_offset >= 0 ? (long long)a.self_offset + row : -1;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const long long cj = j0 + j;
            if (cj < a.n && cj != self) {
              const u64 key = make_key(acc[i][j], cj);
              if (key < t) keys[(size_t)qi * cap + atomicAdd(&cnt[qi], 1)] = key;
            }
          }
        }
        if constexpr (WANT_SUM) {
          double s = 0.0;
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (j0 + j < a.n) s += sqrt((double)acc[i][j]);
          for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
          rowsum[i] += s;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
      }
      wave_sync();
      for (int s = 0; s < 16; ++s) {
        const int qi = wave * 16 + s;
        const int c = cnt[qi];                         // (wave-uniform)
        if (c > a.k) {
          u64* buf = keys + (size_t)qi * cap;
          compact(buf, c, a.k, lane);
          if (lane == 0) {
            cnt[qi] = a.k;
            thr[qi] = buf[a.k - 1];
          }
        }
      }
      wave_sync();
    }
    __syncthreads();
    tile = ntile;
    ch = nc;
    b ^= 1;
  }

  // the part's k smallest, ascending, padded with kEmpty
  for (int s = 0; s < 16; ++s) {
    const int qi = wave * 16 + s;
    const long long row = q0 + qi;
    if (row >= a.q) break;                             // (wave-uniform)
    u64* buf = keys + (size_t)qi * cap;
    const int c = compact(buf, cnt[qi], a.k, lane);
    if (lane < a.k) a.part_keys[((size_t)row * a.splits + part) * a.k + lane] = lane < c ? buf[lane] : kEmpty;
  }
  if (WANT_SUM && tx == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long long row = q0 + ty * 4 + i;
      if (row < a.q) a.part_sum[(size_t)row * a.splits + part] = rowsum[i];
    }
  }
}

// a wave per query: the k smallest of its splits * k part keys, ascending; the partial sums added in part order
__global__ void __launch_bounds__(256) knn_merge_kernel(KnnArgs a) {
  __shared__ u64 bufs[4][kKnnKMax + 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long row = (long long)blockIdx.x * 4 + wave;
  if (row >= a.q) return;                              // (no workgroup barrier below)
  u64* buf = bufs[wave];
  const size_t total = (size_t)a.splits * a.k;
  const u64* src = a.part_keys + (size_t)row * total;
  int cnt = 0;
  u64 thr = kEmpty;
  for (size_t b0 = 0; b0 < total; b0 += 64) {
    const u64 key = b0 + lane < total ? src[b0 + lane] : kEmpty;
    const bool pass = key < thr;
    const u64 mask = __ballot(pass);
    if (pass) buf[cnt + __popcll(mask & ((1ull << lane) - 1))] = key;
    cnt += __popcll(mask);
    wave_sync();
    if (cnt > a.k) {
      cnt = compact(buf, cnt, a.k, lane);
      thr = buf[a.k - 1];
    }
  }
  cnt = compact(buf, cnt, a.k, lane);
  if (lane < a.k) {
    const u64 key = lane < cnt ? buf[lane] : kEmpty;
    const size_t o = (size_t)row * a.k + lane;
    a.out_idx[o] = key == kEmpty ? -1 : (int)(unsigned)(key & 0xffffffffull);
    if (a.out_dist2) a.out_dist2[o] = key == kEmpty ? __uint_as_float(0x7f800000u) : __uint_as_float((unsigned)(key >> 32));
  }
  if (a.out_sum && lane == 0) {
    double s = 0.0;
    for (int p = 0; p < a.splits; ++p) s += a.part_sum[(size_t)row * a.splits + p];
    a.out_sum[row] = s;
  }
}

size_t tile_lds_bytes(int k) {
  return (size_t)4 * kStage * 4 + (size_t)kKnnTileQ * (k + kKnnTileC) * 8 + kKnnTileQ * 8 + kKnnTileQ * 4;
}

}  // namespace

int knn_effective_splits(int q, int n, int splits, int cus) {
  const long long tiles = ((long long)n + kKnnTileC - 1) / kKnnTileC;
  long long s = splits > 0 ? splits : knn_auto_splits(q, n, cus);
  if (s > tiles) s = tiles;
  return s < 1 ? 1 : (int)s;
}

size_t knn_workspace_bytes(int q, int k, int eff_splits) {
  return 16 + ((size_t)q * (size_t)eff_splits * ((size_t)k + 1) * 8 + 15) / 16 * 16;
}

hipError_t launch_knn(const float* x, long long ldx, const float* y, long long ldy, int q, int n, int d, int k, int self_offset,
                      int eff_splits, int* out_idx, float* out_dist2, double* out_sum, void* ws, hipStream_t st) {
  KnnArgs a{x, y, ldx, ldy, q, n, d, k, self_offset, eff_splits, nullptr, nullptr, out_idx, out_dist2, out_sum};
  a.part_keys = reinterpret_cast<u64*>(ws);
  if (out_sum) a.part_sum = reinterpret_cast<double*>(a.part_keys + (size_t)q * eff_splits * k);
  static bool raised[64];                              // (dynamic LDS above 64 KiB has to be asked for, once per device)
  int dev = 0;
  if (hipError_t err = hipGetDevice(&dev); err != hipSuccess) return err;
  if (dev < 0 || dev >= 64 || !raised[dev]) {
    for (const void* f : {reinterpret_cast<const void*>(&knn_tile_kernel<false>), reinterpret_cast<const void*>(&knn_tile_kernel<true>)})
      if (hipError_t err = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tile_lds_bytes(kKnnKMax));
          err != hipSuccess)
        return err;
    if (dev >= 0 && dev < 64) raised[dev] = true;
  }
  const long long qblocks = ((long long)q + kKnnTileQ - 1) / kKnnTileQ;
  if (out_sum)
    knn_tile_kernel<true><<<(unsigned)(qblocks * eff_splits), 256, tile_lds_bytes(k), st>>>(a);
  else
    knn_tile_kernel<false><<<(unsigned)(qblocks * eff_splits), 256, tile_lds_bytes(k), st>>>(a);
  if (hipError_t err = hipGetLastError(); err != hipSuccess) return err;
  knn_merge_kernel<<<(unsigned)(((long long)q + 3) / 4), 256, 0, st>>>(a);
  return hipGetLastError();
}

}  // namespace gcn
