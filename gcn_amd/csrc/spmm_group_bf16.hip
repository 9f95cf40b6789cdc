// spmm_group_bf16.hip — bf16 feature operands (fp32 accumulation everywhere): the group walk on a bf16 table, the bf16
// re-lay of B in the group kernels' slice layout, the slice reduction with a bf16 result, and the three element-wise
// passes of the fallback (widen B, narrow C) and of dropout on bf16 tensors.
//
// The walk is group_walk of spmm_group.hip with a table of bf16 rows: the SAME 15-bit slice-major stream, chunk
// metadata, cut lists, XCD-ordered chunk assignment, segment order of the tiles and non-temporal stream rule.  What
// changes is what one lane gathers: 16 bytes are 8 bf16 columns, so a 16-lane engine covers 128 columns per tile pass
// (the fp32 walk: 64) — half the bytes behind every non-zero and, at k = 128, one walk over the stream instead of two.
// Every lane widens its 8 columns to fp32 by shift / mask (a bf16 is the top half of an fp32) and adds them in fp32;
// partial rows go to the fp32 slab Cv / P exactly as in the fp32 walk (32 bytes per lane: two non-temporal 16-byte
// stores), so the slice reduction and the cut-row pieces are unchanged.  Value-free pass: the table is
// bf16(u_col[c] * B[c, :]) (one RNE rounding: relative error <= 2^-9 per entry), the reduction scales by u_row.
// Weighted pass (values that do not factor): the table is B itself (exact), one fp32 value per entry beside the stream.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include "spmm_kernels.h"

namespace gcn {

namespace {

typedef float bf_f32x4 __attribute__((ext_vector_type(4)));
typedef float bf_f32x2 __attribute__((ext_vector_type(2)));

template <int UU>
__device__ __forceinline__ int bf_row_bcast(int v) {             // value held by lane UU of this lane's 16-lane row (DPP)
  return __builtin_amdgcn_mov_dpp(v, 0x150 + UU, 0xf, 0xf, true);
}

__device__ __forceinline__ float bf_lo(unsigned w) { return __uint_as_float(w << 16); }          // column 2i of a word
__device__ __forceinline__ float bf_hi(unsigned w) { return __uint_as_float(w & 0xFFFF0000u); }  // column 2i + 1
__device__ __forceinline__ float bf2f(unsigned short h) { return __uint_as_float((unsigned)h << 16); }
__device__ __forceinline__ unsigned short f2bf(float f) { return __bfloat16_as_ushort(__float2bfloat16(f)); }   // RNE

// 8 finished fp32 columns of a partial row: two non-temporal 16-byte stores (the slab is read back once, by the reduction)
__device__ __forceinline__ void store_row_piece8(float* dst, const bf_f32x2* a) {
  const bf_f32x4 t0 = {a[0].x, a[0].y, a[1].x, a[1].y}, t1 = {a[2].x, a[2].y, a[3].x, a[3].y};
  __builtin_nontemporal_store(t0, reinterpret_cast<bf_f32x4*>(dst));
  __builtin_nontemporal_store(t1, reinterpret_cast<bf_f32x4*>(dst + 4));
}

// stream / vals / chunk_meta: as group_walk (spmm_group.hip).  Bh: bf16 table, slice s at rows [s*(w+1), (s+1)*(w+1)),
// row w of every slice zero, rows ldh bf16 (2*ldh bytes) apart.  Cv / P: fp32, rows k floats apart.  k % 8 == 0.
template <bool VALS, bool RING, bool BIG>
__device__ __forceinline__ void
group_walk_bf16(const unsigned short* __restrict__ stream, const float* __restrict__ vals, const int2* __restrict__ chunk_meta,
                const unsigned short* __restrict__ Bh, float* __restrict__ Cv, float* __restrict__ P,
                int nchunks, int T, int k, int seg_blocks, int ldh, int stream_nt, int blocks_per_tile) {
  const int lane = threadIdx.x & 63;
  const int wib  = threadIdx.x >> 6;
  const int g    = lane >> 4;
  const int f    = lane & 15;
  const int per_xcd = nchunks >> 3;
  // (tile, block) order inside the launch: as group_walk, with 128-column tiles
  int bx, col_tile;
  if (seg_blocks > 0) {
    const int Q = seg_blocks, nbx = blocks_per_tile >> 3, tiles = (k + 127) >> 7;
    const int x = (int)blockIdx.x & 7, i = (int)blockIdx.x >> 3;
    const int nseg = (nbx + Q - 1) / Q, full = (nseg - 1) * tiles * Q;
    int j;
    if (i < full) { const int seg = i / (tiles * Q), r = i - seg * tiles * Q; col_tile = r / Q; j = seg * Q + (r - col_tile * Q); }
    else { const int last = nbx - (nseg - 1) * Q, r = i - full; col_tile = r / last; j = (nseg - 1) * Q + (r - col_tile * last); }
    bx = j * 8 + x;
  } else {
    col_tile = (int)blockIdx.x / blocks_per_tile;
    bx = (int)blockIdx.x - col_tile * blocks_per_tile;
  }
  const int c_in = ((bx >> 3) * 4 + wib) * 4;
  if (c_in >= per_xcd) return;                                  // (whole wave: per_xcd % 4 == 0)
  const int c = (bx & 7) * per_xcd + c_in + g;                  // this group's chunk

  const int fcol = col_tile * 128 + f * 8;
  const bool fok = fcol < k;                                    // (k % 8 == 0: 8 columns are all in or all out)
  const unsigned row_bytes = (unsigned)ldh * 2u;
  const unsigned foff = (unsigned)(fok ? fcol : col_tile * 128) * 2u;
  const char* Bb = reinterpret_cast<const char*>(Bh);
  const size_t kk = (size_t)k;

  const int2 meta = chunk_meta[c];
  const int vrow = meta.x >> 1;
  const bool head = meta.x & 1;
  const int base = BIG ? 0 : meta.y;
  if constexpr (BIG) Bb += (size_t)meta.y * (size_t)row_bytes;
  float* ptr  = head ? P + (size_t)(2 * c) * kk + fcol : Cv + (size_t)vrow * kk + fcol;
  float* nptr = Cv + (size_t)(vrow + 1) * kk + fcol;
  bool first = true;
  // RING: four finished rows of a group wait in LDS and leave with one 64-lane pass (as spmm_group_ring_kernel; a lane's
  // share of a row is 32 bytes here, so the ring is twice as large: 32 KiB per block)
  __shared__ bf_f32x4 ring[RING ? 4 : 1][4][4][16][2];
  int ring_n = 0;
  float* ring_base = nullptr;
#define GCN_B_DRAIN(G2, ROWS)                                                                       \
  {                                                                                                 \
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(uintptr_t)ring_base, 16 * G2);    \
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)((uintptr_t)ring_base >> 32), 16 * G2); \
    float* b0 = reinterpret_cast<float*>(((uintptr_t)hi << 32) | lo);                              \
    const bf_f32x4 r0 = ring[wib][G2][lane >> 4][f][0], r1 = ring[wib][G2][lane >> 4][f][1];        \
    if (fok && (lane >> 4) < (ROWS)) {                                                              \
      float* d = b0 + (size_t)(lane >> 4) * kk + f * 8;                                             \
      __builtin_nontemporal_store(r0, reinterpret_cast<bf_f32x4*>(d));                              \
      __builtin_nontemporal_store(r1, reinterpret_cast<bf_f32x4*>(d + 4));                          \
    }                                                                                               \
    if (g == G2) ring_n = 0;                                                                        \
  }

  typedef unsigned int u32x2_b __attribute__((ext_vector_type(2)));
  const u32x2_b* __restrict__ sp = reinterpret_cast<const u32x2_b*>(stream + (size_t)c * T) + f;
  const bf_f32x4* __restrict__ vp = VALS ? reinterpret_cast<const bf_f32x4*>(vals + (size_t)c * T) + f : nullptr;
  bf_f32x2 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = bf_f32x2{0.f, 0.f};
  u32x2_b eq = stream_nt ? __builtin_nontemporal_load(sp) : sp[0], eq_nx = eq;
  bf_f32x4 vq = {0.f, 0.f, 0.f, 0.f}, vq_nx = vq;
  if constexpr (VALS) { vq = stream_nt ? __builtin_nontemporal_load(vp) : vp[0]; vq_nx = vq; }
  unsigned fl = 0;
#pragma unroll 1
  for (int blk = 0; blk < T / 16; ++blk) {
    const int j = blk & 3;
    if (j == 0 && blk + 4 < T / 16) {                           // the next run, a whole run ahead of its use
      const int nx = (blk / 4 + 1) * 16;
      eq_nx = stream_nt ? __builtin_nontemporal_load(sp + nx) : sp[nx];
      if constexpr (VALS) vq_nx = stream_nt ? __builtin_nontemporal_load(vp + nx) : vp[nx];
    }
    const unsigned e = ((j & 2 ? eq.y : eq.x) >> (16 * (j & 1))) & 0xFFFFu;
    int vbits = 0;
    if constexpr (VALS) vbits = __builtin_bit_cast(int, j == 0 ? vq.x : j == 1 ? vq.y : j == 2 ? vq.z : vq.w);
    if (j == 3) { eq = eq_nx; vq = vq_nx; }
    const int rowoff = (int)(__umul24((e & 0x7FFFu) + (unsigned)base, row_bytes));
    fl = e >> 15;
    uint4 b[16];
#define GCN_B_ALL(M) M(0) M(1) M(2) M(3) M(4) M(5) M(6) M(7) M(8) M(9) M(10) M(11) M(12) M(13) M(14) M(15)
#define GCN_B_GATHER(UU) \
    b[UU] = *reinterpret_cast<const uint4*>(Bb + (size_t)((unsigned)bf_row_bcast<UU>(rowoff) + foff));
    GCN_B_ALL(GCN_B_GATHER)
#undef GCN_B_GATHER
    const unsigned long long ends = __ballot(fl != 0);          // bit g*16+u: entry u of group g ends a row
#define GCN_B_ADD(UU)                                                                               \
    {                                                                                               \
      const bf_f32x2 w0 = {bf_lo(b[UU].x), bf_hi(b[UU].x)}, w1 = {bf_lo(b[UU].y), bf_hi(b[UU].y)};  \
      const bf_f32x2 w2 = {bf_lo(b[UU].z), bf_hi(b[UU].z)}, w3 = {bf_lo(b[UU].w), bf_hi(b[UU].w)};  \
      if constexpr (VALS) {                                                                         \
        const float vu = __builtin_bit_cast(float, bf_row_bcast<UU>(vbits));                        \
        const bf_f32x2 v2 = {vu, vu};                                                               \
        acc[0] = __builtin_elementwise_fma(v2, w0, acc[0]); acc[1] = __builtin_elementwise_fma(v2, w1, acc[1]); \
        acc[2] = __builtin_elementwise_fma(v2, w2, acc[2]); acc[3] = __builtin_elementwise_fma(v2, w3, acc[3]); \
      } else { acc[0] += w0; acc[1] += w1; acc[2] += w2; acc[3] += w3; }                            \
    }
    if (ends == 0ull) {
      GCN_B_ALL(GCN_B_ADD)
    } else {
#define GCN_B_STEP(UU)                                                                              \
      GCN_B_ADD(UU)                                                                                 \
      if (ends & (0x0001000100010001ull << UU)) {                /* some group ends a row here */    \
        if (bf_row_bcast<UU>((int)fl)) {                                                            \
          if (RING && !(first && head) && ring_n < 4) {                                             \
            if (fok) {                                                                              \
              ring[wib][g][ring_n][f][0] = bf_f32x4{acc[0].x, acc[0].y, acc[1].x, acc[1].y};        \
              ring[wib][g][ring_n][f][1] = bf_f32x4{acc[2].x, acc[2].y, acc[3].x, acc[3].y};        \
            }                                                                                       \
            if (ring_n == 0) ring_base = ptr;                                                       \
            ++ring_n;                                                                               \
          } else if (fok) store_row_piece8(ptr, acc);                                               \
          _Pragma("unroll") for (int i = 0; i < 4; ++i) acc[i] = bf_f32x2{0.f, 0.f};                \
          ptr = nptr; nptr += kk; first = false;                                                    \
        }                                                                                           \
      }
      GCN_B_ALL(GCN_B_STEP)
#undef GCN_B_STEP
      if constexpr (RING) {
        const unsigned long long full = __ballot(ring_n == 4);
        if (full) {
          if (full & 0x0000000000000001ull) GCN_B_DRAIN(0, 4)
          if (full & 0x0000000000010000ull) GCN_B_DRAIN(1, 4)
          if (full & 0x0000000100000000ull) GCN_B_DRAIN(2, 4)
          if (full & 0x0001000000000000ull) GCN_B_DRAIN(3, 4)
        }
      }
    }
#undef GCN_B_ADD
#undef GCN_B_ALL
  }
  if constexpr (RING) {                                         // what is left in the rings
    const unsigned long long some = __ballot(ring_n > 0);
    if (some & 0x0000000000000001ull) GCN_B_DRAIN(0, __builtin_amdgcn_readlane(ring_n, 0))
    if (some & 0x0000000000010000ull) GCN_B_DRAIN(1, __builtin_amdgcn_readlane(ring_n, 16))
    if (some & 0x0000000100000000ull) GCN_B_DRAIN(2, __builtin_amdgcn_readlane(ring_n, 32))
    if (some & 0x0001000000000000ull) GCN_B_DRAIN(3, __builtin_amdgcn_readlane(ring_n, 48))
  }
#undef GCN_B_DRAIN
  // the piece that sticks out of the chunk's end goes where the row's partial sum lives (as group_walk)
  if (!bf_row_bcast<15>((int)fl)) {
    if (fok) store_row_piece8(ptr, acc);
  }
}

}  // namespace

template <bool BIG>
__global__ void __launch_bounds__(256)
spmm_group_bf16_kernel(const unsigned short* __restrict__ stream, const int2* __restrict__ chunk_meta,
                       const unsigned short* __restrict__ Bh, float* __restrict__ Cv, float* __restrict__ P,
                       int nchunks, int T, int k, int seg_blocks, int ldh, int stream_nt, int blocks_per_tile) {
  group_walk_bf16<false, true, BIG>(stream, nullptr, chunk_meta, Bh, Cv, P, nchunks, T, k, seg_blocks, ldh, stream_nt, blocks_per_tile);
}

// values beside the stream (no ring, as the fp32 weighted walk); Bh is the unscaled table
template <bool BIG>
__global__ void __launch_bounds__(256)
spmm_group_bf16_weighted_kernel(const unsigned short* __restrict__ stream, const float* __restrict__ vals,
                                const int2* __restrict__ chunk_meta, const unsigned short* __restrict__ Bh,
                                float* __restrict__ Cv, float* __restrict__ P, int nchunks, int T, int k, int seg_blocks,
                                int ldh, int stream_nt, int blocks_per_tile) {
  group_walk_bf16<true, false, BIG>(stream, vals, chunk_meta, Bh, Cv, P, nchunks, T, k, seg_blocks, ldh, stream_nt, blocks_per_tile);
}

namespace {

template <bool BIG>
hipError_t launch_group_bf16_t(const GroupArgs& a, const unsigned short* Bh, int ldh, hipStream_t s) {
  const int per_xcd = a.nchunks / 8;
  int nblocks = 8 * ((per_xcd + 15) / 16);
  const int tiles = (a.k + 127) / 128;
  // the stream and segment rules of launch_group_t (spmm_group.hip), unchanged
  const size_t stream_bytes = (size_t)a.nchunks * (size_t)a.T * (a.vals ? 6u : 2u);
  const int stream_nt = stream_bytes > ((size_t)64 << 20) ? 1 : 0;
  if ((long long)nblocks * tiles >= (1LL << 31)) return hipErrorInvalidValue;
  const int blocks_per_tile = nblocks;
  nblocks *= tiles;
  const int2* meta = reinterpret_cast<const int2*>(a.chunk_meta);
  const int nseg = (int)((stream_bytes + ((size_t)120 << 20) - 1) / ((size_t)120 << 20));
  const int nbx = blocks_per_tile / 8;
  const int seg_blocks = (nseg > 1 && tiles > 1 && nbx > 1) ? (nbx + nseg - 1) / nseg : 0;
  if (a.vals)
    spmm_group_bf16_weighted_kernel<BIG><<<dim3(nblocks), dim3(256), 0, s>>>(a.stream, a.vals, meta, Bh, a.Cv, a.P, a.nchunks, a.T, a.k, seg_blocks, ldh, stream_nt, blocks_per_tile);
  else
    spmm_group_bf16_kernel<BIG><<<dim3(nblocks), dim3(256), 0, s>>>(a.stream, meta, Bh, a.Cv, a.P, a.nchunks, a.T, a.k, seg_blocks, ldh, stream_nt, blocks_per_tile);
  return hipGetLastError();
}

}  // namespace

// BIG addressing counts BYTES: a bf16 row of ldh columns is ldh / 2 four-byte words (spmm_group_needs_big's unit)
bool spmm_group_bf16_needs_big(long long table_rows, int ldh) { return spmm_group_needs_big(table_rows, ldh / 2); }

hipError_t launch_spmm_group_bf16(const GroupArgs& a, const unsigned short* Bh, hipStream_t s) {
  if (a.nchunks <= 0 || a.k <= 0) return hipSuccess;
  if (a.nchunks % 32 != 0 || a.k % 8 != 0 || a.T < 64 || a.T % 64 != 0 || a.table_rows <= 0) return hipErrorInvalidValue;
  const int ldh = a.ldb > 0 ? a.ldb : a.k;
  if (ldh % 8 != 0 || ldh < a.k || ((uintptr_t)Bh & 15) != 0) return hipErrorInvalidValue;
  const bool big = spmm_group_bf16_needs_big(a.table_rows, ldh);
  if (big && ldh * 2 >= (1 << 17)) return hipErrorInvalidValue;   // (the offset inside a slice must still fit 32 bits)
  return big ? launch_group_bf16_t<true>(a, Bh, ldh, s) : launch_group_bf16_t<false>(a, Bh, ldh, s);
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

// ---- slice reduction with a bf16 result: the S partial rows in slice order, then the cut-row pieces in chunk order (the
// order of slice_reduce_wide_kernel), row factor, bias, ReLU, the dropout mask of element r*k + x, one RNE rounding
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
      const bf_f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const bf_f32x4*>(Cv + (size_t)s * slab + off));
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    if (cuts.ptr) {
      for (int q = cuts.ptr[r]; q < cuts.ptr[r + 1]; ++q) {
        const bf_f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const bf_f32x4*>(cuts.P + (size_t)(2 * cuts.chunk[q]) * (size_t)k + x));
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
      }
    }
    if (rowscale) { const float rs = rowscale[r]; acc.x *= rs; acc.y *= rs; acc.z *= rs; acc.w *= rs; }
    if (bias) { acc.x += bias[x]; acc.y += bias[x + 1]; acc.z += bias[x + 2]; acc.w += bias[x + 3]; }
    if (relu) { acc.x = fmaxf(acc.x, 0.f); acc.y = fmaxf(acc.y, 0.f); acc.z = fmaxf(acc.z, 0.f); acc.w = fmaxf(acc.w, 0.f); }
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

hipError_t launch_slice_reduce_bf16(const float* Cv, unsigned short* C, const float* bias, int relu, int m, int S, int k,
                                    const float* rowscale, const DropoutSpec& drop, const CutLists& cuts, hipStream_t st) {
  if (m <= 0 || k <= 0) return hipSuccess;
  if (k % 4 != 0 || (((uintptr_t)Cv | (uintptr_t)cuts.P) & 15) != 0) return hipErrorInvalidValue;
  const int vec_out = ((uintptr_t)C & 7) == 0 ? 1 : 0;
  long long nb = ((long long)m * (k / 4) + 255) / 256;
  if (nb > 65536) nb = 65536;
  if (drop.on()) slice_reduce_bf16_kernel<true><<<(int)nb, 256, 0, st>>>(Cv, C, bias, relu, m, S, k, rowscale, drop, cuts, vec_out);
  else           slice_reduce_bf16_kernel<false><<<(int)nb, 256, 0, st>>>(Cv, C, bias, relu, m, S, k, rowscale, drop, cuts, vec_out);
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
