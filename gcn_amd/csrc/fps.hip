// fps.hip — farthest point sampling of a batch of point clouds stored back to back (the contract is in include/gcn_spmm.h,
// gcn_fps_f32).
//
// DISTANCE AND ORDER.  d2(p, pick) is knn.hip's chain: one fp32 accumulator, columns ascending, diff = x_pc - x_wc, acc =
// fmaf(diff, diff, acc); a NaN result counts as 0.  A row keeps dmin, the smallest d2 to the picks so far, and the next pick
// is the unpicked row of largest dmin, the smaller index on equal dmin.  dmin is never negative and never NaN, so its bits
// order as an unsigned integer and the candidate key is (bits of dmin) << 32 | ~index, reduced with a 64-bit max; a picked row
// (and a thread's slot past the cloud) carries dmin = -1 and the key 0, which no candidate has.
//
// ONE WORKGROUP PER CLOUD.  The picks are a serial chain, so all the speed is in the step from one pick to the next: one
// distance and one min per held point, a wave-wide max by shuffles, then every wave writes its best key (and, on the register
// route, that row's coordinates) to the LDS slot [parity][wave].  After ONE __syncthreads() every thread reduces the <= 16
// slots itself and holds the winner: its index, its dmin and its coordinates.  The next pick writes the slots of the other
// parity: a wave can only reach the slots of this parity again after the next barrier, which every reader of this pick has
// then passed.  Nothing but the 4-byte result leaves the chip between two picks.
//
// ROUTES.  A cloud of n_b points goes, by n_b alone and with identical results:
//   resident, 256 threads,  n_b <= min(1024, L): a thread holds P = 1, 2 or 4 points;
//   resident, 1024 threads, n_b <= L = fps_resident_points(d): P = 2, 4 or 8 (a 16-wave barrier is dearer, so small clouds
//     stay with four waves);
//   streamed, 1024 threads, any n_b: dmin lives in the workspace (a row is only ever touched by the same thread), the
//     coordinates are re-read from global memory at every pick.
// On the resident routes the coordinates sit in registers for d <= 4 (D = 3 serves d <= 3 with zero columns: fmaf(0, 0, acc)
// is acc) and in LDS, column-major, for wider rows (D = 0); dmin is in registers in both.  The host cannot see the segment
// sizes, so each route is one launch over all segments and a workgroup whose cloud belongs to another route leaves at once;
// a launch that n or L rule out as a whole is not made.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "spmm_kernels.h"

namespace gcn {
namespace {

typedef unsigned long long u64;

constexpr int kSmallThreads = 256, kLargeThreads = 1024;
constexpr int kSmallPoints = 4 * kSmallThreads;        // the most points the four-wave workgroup holds
constexpr int kMaxWaves = kLargeThreads / 64;
constexpr int kRegCols = 4;                            // columns a register-route slot carries
static_assert(kFpsResidentMax == 8 * kLargeThreads && kFpsLdsFloats * 4 + 4096 <= 160 * 1024, "P <= 8; 160 KiB of LDS per workgroup");

struct FpsArgs {
  const float* x;
  long long ldx;
  int n, d;
  const int* seg_ptr;
  const int* out_ptr;
  const int* start;
  int* out_idx;
  float* out_dist2;
  float* dmin;                                         // [n], the streamed route only
  int limit;                                           // fps_resident_points(d)
};

struct Cloud {
  int lo, nb, out_lo, m, s;                            // first row, rows, first output, picks, local start row
};

__device__ __forceinline__ int clamp_i(long long v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); }

// every figure of a cloud is clamped here: nothing below indexes by unchecked device data
__device__ __forceinline__ Cloud cloud_of(const FpsArgs& a, int b) {
  Cloud c;
  c.lo = clamp_i(a.seg_ptr[b], 0, a.n);
  const int hi = clamp_i(a.seg_ptr[b + 1], 0, a.n);
  c.nb = hi > c.lo ? hi - c.lo : 0;
  c.out_lo = clamp_i(a.out_ptr[b], 0, a.n);
  const int out_hi = clamp_i(a.out_ptr[b + 1], 0, a.n);
  c.m = out_hi > c.out_lo ? out_hi - c.out_lo : 0;
  if (c.m > c.nb) c.m = c.nb;
  c.s = (a.start && c.nb > 0) ? clamp_i((long long)a.start[b] - c.lo, 0, c.nb - 1) : 0;
  return c;
}

__device__ __forceinline__ u64 fps_key(float dmin, int i) {
  return dmin < 0.0f ? 0ull : ((u64)__float_as_uint(dmin) << 32) | (u64)(~(unsigned)i);
}

__device__ __forceinline__ u64 wave_max(u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const u64 o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

// the new dmin of a row that held v: the NaN rule, the min, and -1 once the row is the pick itself
__device__ __forceinline__ float fps_update(float v, float d2, bool is_pick) {
  d2 = d2 != d2 ? 0.0f : d2;
  v = d2 < v ? d2 : v;                                  // (v = -1 stays: d2 >= 0)
  return is_pick ? -1.0f : v;
}

__device__ __forceinline__ void fps_store(const FpsArgs& a, const Cloud& c, int t, int widx, float wd) {
  a.out_idx[(size_t)c.out_lo + t] = c.lo + widx;
  if (a.out_dist2) a.out_dist2[(size_t)c.out_lo + t] = wd;
}

// The slots of one parity -> the winner.  Every thread does this for itself; the reads are broadcasts.
template <int WAVES>
__device__ __forceinline__ u64 reduce_slots(const u64* slot_key, int par, int* wave_of) {
  u64 g = 0;
  int gw = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const u64 key = slot_key[par * kMaxWaves + w];
    if (key > g) {
      g = key;
      gw = w;
    }
  }
  *wave_of = gw;
  return g;
}

// One cloud of at most P * THREADS points.  D > 0: the coordinates of a thread's points are registers, d <= D.  D == 0: they
// are xs[column][point] in LDS, any d.
template <int D, int THREADS, int P>
__device__ __forceinline__ void fps_resident(const FpsArgs& a, const Cloud& c, float* xs, u64* slot_key, float* slot_c) {
  constexpr int WAVES = THREADS / 64;
  constexpr int DR = D > 0 ? D : 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* xb = a.x + (size_t)c.lo * (size_t)a.ldx;
  float px[P][DR], dm[P], w[DR];
  int at[P];                                           // (D == 0) the point's place in a column, kept inside the cloud
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int i = p * THREADS + tid;
    const bool in = i < c.nb;
    dm[p] = in ? __uint_as_float(0x7f800000u) : -1.0f;
    at[p] = in ? i : c.nb - 1;
#pragma unroll
    for (int k = 0; k < DR; ++k) {                     // (unconditional loads from inside the cloud: no branches here)
      const float v = D > 0 ? xb[(size_t)at[p] * (size_t)a.ldx + (k < a.d ? k : 0)] : 0.0f;
      px[p][k] = k < a.d ? v : 0.0f;
    }
  }
  if constexpr (D == 0) {
    for (long long e = tid; e < (long long)c.nb * a.d; e += THREADS) {
      const int i = (int)(e / a.d), k = (int)(e % a.d);
      xs[(size_t)k * c.nb + i] = xb[(size_t)i * (size_t)a.ldx + k];
    }
    __syncthreads();
  }
  int widx = c.s;
  float wd = __uint_as_float(0x7f800000u);
#pragma unroll
  for (int k = 0; k < DR; ++k) w[k] = (D > 0 && k < a.d) ? xb[(size_t)widx * (size_t)a.ldx + k] : 0.0f;

  int par = 0;
  for (int t = 0;; ++t) {
    if (tid == 0) fps_store(a, c, t, widx, wd);
    if (t + 1 >= c.m) break;
    float acc[P];
#pragma unroll
    for (int p = 0; p < P; ++p) acc[p] = 0.0f;
    if constexpr (D == 0) {
      for (int k = 0; k < a.d; ++k) {
        const float* col = xs + (size_t)k * c.nb;
        const float wk = col[widx];
#pragma unroll
        for (int p = 0; p < P; ++p) {
          const float diff = col[at[p]] - wk;
          acc[p] = __builtin_fmaf(diff, diff, acc[p]);
        }
      }
    }
    u64 best = 0;
    int bp = 0;                                        // which of the thread's points holds `best`
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int i = p * THREADS + tid;
      if constexpr (D > 0) {
#pragma unroll
        for (int k = 0; k < D; ++k) {
          const float diff = px[p][k] - w[k];
          acc[p] = __builtin_fmaf(diff, diff, acc[p]);
        }
      }
      dm[p] = fps_update(dm[p], acc[p], i == widx);
      const u64 key = fps_key(dm[p], i);
      bp = key > best ? p : bp;
      best = key > best ? key : best;
    }
    const u64 wbest = wave_max(best);
    if (lane == 0) slot_key[par * kMaxWaves + wave] = wbest;
    if constexpr (D > 0) {
      if (best == wbest && wbest != 0) {               // (keys are unique: one lane of the wave)
#pragma unroll
        for (int p = 0; p < P; ++p)
          if (bp == p) {
#pragma unroll
            for (int k = 0; k < D; ++k) slot_c[(par * kMaxWaves + wave) * kRegCols + k] = px[p][k];
          }
      }
    }
    __syncthreads();
    int gw;
    const u64 g = reduce_slots<WAVES>(slot_key, par, &gw);
    if (g == 0) break;                                 // (no candidate left; m <= n_b keeps this from happening)
    widx = (int)(~(unsigned)(g & 0xffffffffull));
    wd = __uint_as_float((unsigned)(g >> 32));
    if constexpr (D > 0) {
#pragma unroll
      for (int k = 0; k < D; ++k) w[k] = slot_c[(par * kMaxWaves + gw) * kRegCols + k];
    }
    par ^= 1;
  }
}

template <int D, int THREADS>
__global__ void __launch_bounds__(THREADS) fps_resident_kernel(FpsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float xs[];
  __shared__ u64 slot_key[2 * kMaxWaves];
  __shared__ float slot_c[2 * kMaxWaves * kRegCols];
  static_assert(D <= kRegCols, "a slot carries kRegCols coordinates");
  const Cloud c = cloud_of(a, (int)blockIdx.x);
  const int small_top = a.limit < kSmallPoints ? a.limit : kSmallPoints;
  if (c.m == 0) return;                                // (all returns are the whole workgroup's)
  if (THREADS == kSmallThreads ? c.nb > small_top : (c.nb <= small_top || c.nb > a.limit)) return;
  constexpr int P0 = THREADS == kSmallThreads ? 1 : 2;
  if (c.nb <= P0 * THREADS)
    fps_resident<D, THREADS, P0>(a, c, xs, slot_key, slot_c);
  else if (c.nb <= 2 * P0 * THREADS)
    fps_resident<D, THREADS, 2 * P0>(a, c, xs, slot_key, slot_c);
  else
    fps_resident<D, THREADS, 4 * P0>(a, c, xs, slot_key, slot_c);
}

// Any cloud: the workgroup strides over its rows at every pick.  dmin[row] is read and written by one thread only (rows
// tid, tid + 1024, ...), so the workspace needs no fence; at the first pick it is taken as +inf instead of being read.
__global__ void __launch_bounds__(kLargeThreads) fps_streamed_kernel(FpsArgs a) {
  __shared__ u64 slot_key[2 * kMaxWaves];
  const Cloud c = cloud_of(a, (int)blockIdx.x);
  if (c.m == 0 || c.nb <= a.limit) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* xb = a.x + (size_t)c.lo * (size_t)a.ldx;
  float* dm = a.dmin + c.lo;
  int widx = c.s;
  float wd = __uint_as_float(0x7f800000u);
  int par = 0;
  for (int t = 0;; ++t) {
    if (tid == 0) fps_store(a, c, t, widx, wd);
    if (t + 1 >= c.m) break;
    const float* wr = xb + (size_t)__builtin_amdgcn_readfirstlane(widx) * (size_t)a.ldx;
    u64 best = 0;
    for (int i = tid; i < c.nb; i += kLargeThreads) {
      float v = t == 0 ? __uint_as_float(0x7f800000u) : dm[i];
      if (v >= 0.0f) {
        const float* xr = xb + (size_t)i * (size_t)a.ldx;
        float acc = 0.0f;
        for (int k = 0; k < a.d; ++k) {
          const float diff = xr[k] - wr[k];
          acc = __builtin_fmaf(diff, diff, acc);
        }
        v = fps_update(v, acc, i == widx);
        dm[i] = v;
        const u64 key = fps_key(v, i);
        best = key > best ? key : best;
      }
    }
    const u64 wbest = wave_max(best);
    if (lane == 0) slot_key[par * kMaxWaves + wave] = wbest;
    __syncthreads();
    int gw;
    const u64 g = reduce_slots<kMaxWaves>(slot_key, par, &gw);
    if (g == 0) break;
    widx = (int)(~(unsigned)(g & 0xffffffffull));
    wd = __uint_as_float((unsigned)(g >> 32));
    par ^= 1;
  }
}

template <int D>
hipError_t launch_resident(const FpsArgs& a, int segments, bool large, hipStream_t st) {
  const int small_top = a.limit < kSmallPoints ? a.limit : kSmallPoints;
  const size_t lds = D == 0 ? (size_t)a.d * (large ? a.limit : small_top) * 4 : 0;
  if constexpr (D == 0) {                              // (dynamic LDS above 64 KiB has to be asked for, once per device)
    static bool raised[64];
    int dev = 0;
    if (hipError_t err = hipGetDevice(&dev); err != hipSuccess) return err;
    if (dev < 0 || dev >= 64 || !raised[dev]) {
      for (const void* f : {reinterpret_cast<const void*>(&fps_resident_kernel<0, kSmallThreads>),
                            reinterpret_cast<const void*>(&fps_resident_kernel<0, kLargeThreads>)})
        if (hipError_t err = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kFpsLdsFloats * 4); err != hipSuccess)
          return err;
      if (dev >= 0 && dev < 64) raised[dev] = true;
    }
  }
  if (large)
    fps_resident_kernel<D, kLargeThreads><<<(unsigned)segments, kLargeThreads, lds, st>>>(a);
  else
    fps_resident_kernel<D, kSmallThreads><<<(unsigned)segments, kSmallThreads, lds, st>>>(a);
  return hipGetLastError();
}

}  // namespace

int fps_resident_points(int d) {
  if (d < 1) return 0;
  const int fit = kFpsLdsFloats / d;                   // rows of d floats in the LDS budget; registers serve d <= 4
  return fit < kFpsResidentMax ? fit : kFpsResidentMax;
}

size_t fps_workspace_bytes(int n, int d) {
  return 16 + (n > fps_resident_points(d) ? ((size_t)n * 4 + 15) / 16 * 16 : 0);
}

hipError_t launch_fps(const float* x, long long ldx, int n, int d, const int* seg_ptr, const int* out_ptr, const int* start,
                      int segments, int* out_idx, float* out_dist2, void* ws, hipStream_t st) {
  FpsArgs a{x, ldx, n, d, seg_ptr, out_ptr, start, out_idx, out_dist2, reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + 16),
            fps_resident_points(d)};
  const int small_top = a.limit < kSmallPoints ? a.limit : kSmallPoints;
  for (int large = 0; large < 2; ++large) {
    if (large ? !(n > small_top && a.limit > small_top) : small_top < 1) continue;
    const hipError_t err = d <= 3 ? launch_resident<3>(a, segments, large, st)
                                  : (d == 4 ? launch_resident<4>(a, segments, large, st) : launch_resident<0>(a, segments, large, st));
    if (err != hipSuccess) return err;
  }
  if (n > a.limit) {
    fps_streamed_kernel<<<(unsigned)segments, kLargeThreads, 0, st>>>(a);
    return hipGetLastError();
  }
  return hipSuccess;
}

}  // namespace gcn
