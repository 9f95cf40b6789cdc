// spmm_group_bf16.hip — bf16 feature operands (fp32 accumulation everywhere): the bf16 instantiations of the group walk,
// the bf16 re-lay of B in the group kernels' slice layout, the slice reduction with a bf16 result, and the three
// element-wise passes of the fallback (widen B, narrow C) and of dropout on bf16 tensors.
//
// The walk is group_walk (group_walk.h) with the row format RowBf16: the SAME code as the fp32 kernels of spmm_group.hip —
// stream, chunk metadata, cut lists, XCD-ordered chunk assignment, segment order of the tiles, non-temporal stream rule
// (one launch rule, launch_spmm_group).  What differs is what one lane gathers: 16 bytes are 8 bf16 columns, so a 16-lane
// engine covers 128 columns per tile pass (fp32: 64) — half the bytes behind every non-zero and, at k = 128, one walk over
// the stream instead of two.  Partial rows go to the fp32 slab Cv / P (32 bytes per lane: two non-temporal 16-byte
// stores), so the slice reduction and the cut-row pieces are unchanged.  Value-free pass: the table is
// bf16(u_col[c] * B[c, :]) (one RNE rounding: relative error <= 2^-9 per entry), the reduction scales by u_row.
// Weighted pass (values that do not factor): the table is B itself (exact), one fp32 value per entry beside the stream.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include "spmm_kernels.h"
#include "group_walk.h"

namespace gcn {

namespace {

__device__ __forceinline__ float bf2f(unsigned short h) { return __uint_as_float((unsigned)h << 16); }
__device__ __forceinline__ unsigned short f2bf(float f) { return __bfloat16_as_ushort(__float2bfloat16(f)); }   // RNE

}  // namespace

// Bh: bf16 table, rows ldh bf16 apart; k % 8 == 0; LDS ring of 32 KiB per block
template <bool BIG>
__global__ void __launch_bounds__(256)
spmm_group_bf16_kernel(const unsigned short* __restrict__ stream, const int2* __restrict__ chunk_meta,
                       const unsigned short* __restrict__ Bh, float* __restrict__ Cv, float* __restrict__ P,
                       int nchunks, int T, int k, int seg_blocks, int ldh, int stream_nt, int blocks_per_tile) {
  group_walk<RowBf16, false, true, BIG>(stream, nullptr, chunk_meta, Bh, Cv, P, nchunks, T, k, seg_blocks, ldh, stream_nt, blocks_per_tile, nullptr);
}

// values beside the stream (no ring, as the fp32 weighted walk); Bh is the unscaled table
template <bool BIG>
__global__ void __launch_bounds__(256)
spmm_group_bf16_weighted_kernel(const unsigned short* __restrict__ stream, const float* __restrict__ vals,
                                const int2* __restrict__ chunk_meta, const unsigned short* __restrict__ Bh,
                                float* __restrict__ Cv, float* __restrict__ P, int nchunks, int T, int k, int seg_blocks,
                                int ldh, int stream_nt, int blocks_per_tile) {
  group_walk<RowBf16, true, false, BIG>(stream, vals, chunk_meta, Bh, Cv, P, nchunks, T, k, seg_blocks, ldh, stream_nt, blocks_per_tile, nullptr);
}

namespace {

template <bool BIG>
hipError_t launch_group_bf16_walk_t(const GroupArgs& a, int ldh, const GroupGrid& g, hipStream_t s) {
  const int2* meta = reinterpret_cast<const int2*>(a.chunk_meta);
  const unsigned short* Bh = static_cast<const unsigned short*>(a.Bp);
  if (a.vals)
    spmm_group_bf16_weighted_kernel<BIG><<<dim3(g.nblocks), dim3(256), 0, s>>>(a.stream, a.vals, meta, Bh, a.Cv, a.P, a.nchunks, a.T, a.k, g.seg_blocks, ldh, g.stream_nt, g.blocks_per_tile);
  else
    spmm_group_bf16_kernel<BIG><<<dim3(g.nblocks), dim3(256), 0, s>>>(a.stream, meta, Bh, a.Cv, a.P, a.nchunks, a.T, a.k, g.seg_blocks, ldh, g.stream_nt, g.blocks_per_tile);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_group_walk_bf16(const GroupArgs& a, int ld, const GroupGrid& g, bool big, hipStream_t s) {
  return big ? launch_group_bf16_walk_t<true>(a, ld, g, s) : launch_group_bf16_walk_t<false>(a, ld, g, s);
}


// ---- bf16 table in the group layout: dst[(c / w)*(w+1) + c % w, :] = bf16(rowscale[c] * src[c, :]) or the bits of src[c, :]
__global__ void __launch_bounds__(256)
relay_bf16_sliced_kernel(unsigned short* __restrict__ dst, const unsigned short* __restrict__ src, const float* __restrict__ rowscale,
                         int n, int k, int ld, int S, int w, int src_vec) {
  const int ld8 = ld >> 3;                                       // 16-byte pieces per destination row
  const long long total = (long long)S * (w + 1) * ld8;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const long long R = i / ld8;
    const int x = (int)(i - R * ld8) * 8;
    const int s = (int)(R / (w + 1)), j = (int)(R - (long long)s * (w + 1));
    const long long c = (long long)s * w + j;
    unsigned short h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (j < w && c < n && x < k) {
      const unsigned short* p = src + c * k + x;
      if (src_vec) {
        const uint4 t = *reinterpret_cast<const uint4*>(p);
        const unsigned t4[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) { h[2 * q] = (unsigned short)(t4[q] & 0xFFFFu); h[2 * q + 1] = (unsigned short)(t4[q] >> 16); }
      } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) if (x + q < k) h[q] = p[q];
      }
      if (rowscale) {                                            // scaled in fp32, rounded once (RNE)
        const float u = rowscale[c];
#pragma unroll
        for (int q = 0; q < 8; ++q) h[q] = f2bf(u * bf2f(h[q]));
      }
    }
    uint4 v;
    v.x = h[0] | ((unsigned)h[1] << 16); v.y = h[2] | ((unsigned)h[3] << 16);
    v.z = h[4] | ((unsigned)h[5] << 16); v.w = h[6] | ((unsigned)h[7] << 16);
    *reinterpret_cast<uint4*>(dst + R * ld + x) = v;
  }
}

hipError_t launch_relay_bf16_sliced(unsigned short* dst, const unsigned short* src, const float* rowscale, int n, int k, int ld,
                                    int S, int w, hipStream_t s) {
  if (n <= 0 || k <= 0) return hipSuccess;
  if (ld % 8 != 0 || ld < k || ((uintptr_t)dst & 15) != 0) return hipErrorInvalidValue;
  const int src_vec = ((k & 7) == 0 && ((uintptr_t)src & 15) == 0) ? 1 : 0;
  long long nb = ((long long)S * (w + 1) * (ld / 8) + 255) / 256;
  if (nb > 65536) nb = 65536;
  relay_bf16_sliced_kernel<<<(int)nb, 256, 0, s>>>(dst, src, rowscale, n, k, ld, S, w, src_vec);
  return hipGetLastError();
}

// ---- slice reduction with a bf16 result (launch_slice_reduce, slicing.hip): the S partial rows in slice order, then the cut-row
// pieces in chunk order (as slice_reduce_wide_kernel), row factor, bias, ReLU, the dropout mask of element r*k + x, one RNE rounding
template <bool DROP>
__global__ void __launch_bounds__(256)
slice_reduce_bf16_kernel(const float* __restrict__ Cv, unsigned short* __restrict__ C, const float* __restrict__ bias, int relu,
                         int m, int S, int k, const float* __restrict__ rowscale, DropoutSpec drop, CutLists cuts, int vec_out) {
  const int k4 = k >> 2;
  const long long total = (long long)m * k4;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const size_t slab = (size_t)m * (size_t)k;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const long long r = i / k4;
    const int x = (int)(i - r * k4) * 4;
    const size_t off = (size_t)r * (size_t)k + (size_t)x;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = 0; s < S; ++s) {
      const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(Cv + (size_t)s * slab + off));
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    if (cuts.ptr) {
      for (int q = cuts.ptr[r]; q < cuts.ptr[r + 1]; ++q) {
        const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(cuts.P + (size_t)(2 * cuts.chunk[q]) * (size_t)k + x));
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
      }
    }
    if (rowscale) { const float rs = rowscale[r]; acc.x *= rs; acc.y *= rs; acc.z *= rs; acc.w *= rs; }
    if (bias) { acc.x += bias[x]; acc.y += bias[x + 1]; acc.z += bias[x + 2]; acc.w += bias[x + 3]; }
    if (relu) { acc.x = relu_keep_nan(acc.x); acc.y = relu_keep_nan(acc.y); acc.z = relu_keep_nan(acc.z); acc.w = relu_keep_nan(acc.w); }
    if constexpr (DROP) acc = dropout_apply4(drop, (unsigned long long)off, acc);
    const unsigned short h0 = f2bf(acc.x), h1 = f2bf(acc.y), h2 = f2bf(acc.z), h3 = f2bf(acc.w);
    if (vec_out) {
      uint2 o;
      o.x = h0 | ((unsigned)h1 << 16); o.y = h2 | ((unsigned)h3 << 16);
      *reinterpret_cast<uint2*>(C + off) = o;
    } else {
      C[off] = h0; C[off + 1] = h1; C[off + 2] = h2; C[off + 3] = h3;
    }
  }
}

hipError_t enqueue_slice_reduce_bf16(const SliceReduce& r, int nblocks, int vec_out, hipStream_t st) {
  unsigned short* const C = static_cast<unsigned short*>(r.C);
  if (r.drop.on()) slice_reduce_bf16_kernel<true><<<nblocks, 256, 0, st>>>(r.Cv, C, r.bias, r.relu, r.m, r.S, r.k, r.rowscale, r.drop, r.cuts, vec_out);
  else             slice_reduce_bf16_kernel<false><<<nblocks, 256, 0, st>>>(r.Cv, C, r.bias, r.relu, r.m, r.S, r.k, r.rowscale, r.drop, r.cuts, vec_out);
  return hipGetLastError();
}

// ---- element-wise passes: the fallback's widen / narrow, and dropout of a bf16 tensor (the mask of element i, as fp32)
__global__ void __launch_bounds__(256)
bf16_to_f32_kernel(float* __restrict__ dst, const unsigned short* __restrict__ src, long long count) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) dst[i] = bf2f(src[i]);
}

__global__ void __launch_bounds__(256)
f32_to_bf16_kernel(unsigned short* __restrict__ dst, const float* __restrict__ src, long long count) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) dst[i] = f2bf(src[i]);
}

__global__ void __launch_bounds__(256)
dropout_bf16_kernel(unsigned short* dst, const unsigned short* src, long long count, DropoutSpec drop) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride)
    dst[i] = f2bf(dropout_apply(drop, (unsigned long long)i, bf2f(src[i])));
}

static int elementwise_blocks(long long count) {
  long long nb = (count + 255) / 256;
  return (int)(nb > 65536 ? 65536 : (nb < 1 ? 1 : nb));
}

hipError_t launch_bf16_to_f32(float* dst, const unsigned short* src, long long count, hipStream_t st) {
  if (count <= 0) return hipSuccess;
  bf16_to_f32_kernel<<<elementwise_blocks(count), 256, 0, st>>>(dst, src, count);
  return hipGetLastError();
}

hipError_t launch_f32_to_bf16(unsigned short* dst, const float* src, long long count, hipStream_t st) {
  if (count <= 0) return hipSuccess;
  f32_to_bf16_kernel<<<elementwise_blocks(count), 256, 0, st>>>(dst, src, count);
  return hipGetLastError();
}

hipError_t launch_dropout_bf16(unsigned short* dst, const unsigned short* src, long long count, const DropoutSpec& drop,
                               hipStream_t st) {
  if (count <= 0) return hipSuccess;
  dropout_bf16_kernel<<<elementwise_blocks(count), 256, 0, st>>>(dst, src, count, drop);
  return hipGetLastError();
}

}  // namespace gcn
