// spmm_narrow.hip — the SpMM kernel for narrow feature widths, k <= 16 (GCN hidden / class sizes;
// the reference dedicates four of its five kernels to them: flexspmm.cu:17-422, k4/k8/k16/k32).
//
// With k <= 16 a gathered feature row is only 16..64 bytes, so the wide kernel's "one wave
// instruction per non-zero" spends its time on instruction issue, not on bytes (measured: every
// k <= 32 took the same 1.66 ms on the Reddit-shaped graph).  Here a wave instruction covers
// NPI = 64/G non-zeros at once (G = 4/8/16 lanes per non-zero, the power of two >= k):
//
//   lane = sub*G + f:  sub = which of the NPI non-zeros of this step, f = feature column.
//   The column index and value of non-zero (j + sub) come from the coalesced 64-entry block by
//   one cross-lane read each; the gather is ONE load instruction with a per-lane offset
//   col*k*4 + f*4 (NPI rows of k floats); each lane accumulates its (sub, f) partial sum.
//   When a row ends — anywhere inside a step — the lanes that belong to it are reduced across
//   `sub` (log2(NPI) xor-shuffles) and lanes sub == 0 store the k floats.
//
// Chunk schedule, partial slab and fix-up are those of spmm_kernels.hip (same plan; prologue, chunk range and row cursor
// from chunk_walk.h), so results
// are deterministic; the summation order inside a row differs from the wide kernel (a tree over
// `sub` instead of a chain), within the 1e-5 contract.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "spmm_kernels.h"
#include "chunk_walk.h"

namespace gcn {


template <int G, int U, bool EPI, bool BUF>
__global__ void __launch_bounds__(256)
spmm_narrow_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                   const float* __restrict__ val, const float* __restrict__ B,
                   float* __restrict__ C, float* __restrict__ P,
                   const int* __restrict__ chunk_row, const float* __restrict__ bias,
                   const int* __restrict__ nnz_dev,
                   int relu, int nchunks, int T, int m, int nnz, int k) {
  constexpr int NPI = 64 / G;                       // non-zeros per gather instruction
  dropin_shape(nnz_dev, T, nnz, nchunks, col, val);
  const int lane = threadIdx.x & 63;
  const int wib  = sgpr(threadIdx.x >> 6);
  const int sub  = lane / G;
  const int f    = lane % G;
  const bool fok = f < k;

  const ChunkRange range(wib, nchunks);

  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(B), 0, 0xFFFFFFFFu, 0x00020000);
  const unsigned row_bytes = (unsigned)k * 4u;
  const float bias_f = (EPI && bias && fok) ? bias[f] : 0.f;

  for (int c = range.first; c < range.c_hi; c += range.stride) {
    const int start = c * T;
    const int end   = (int)min((long long)start + T, (long long)nnz);
    GCN_ROW_WALK_OPEN(rowptr, chunk_row, c, T, m);     // r, row_end, row_end_nx, head, pos, last_flush (chunk_walk.h)
    float acc = 0.f;                                // this lane's (sub, f) partial of the current row

    // the current row is complete at `pos`: reduce over sub, write, step to the next row
    auto flush = [&]() {
      float t = acc;
#pragma unroll
      for (int off = G; off < 64; off <<= 1) t += __shfl_xor(t, off);
      if (head) {
        if (sub == 0 && fok) P[(size_t)(2 * c) * k + f] = t;
      } else if (last_flush != pos) {               // (empty rows belong to launch_fill_empty_rows, spmm_kernels.hip)
        if (EPI) {
          t += bias_f;
          if (relu) t = relu_keep_nan(t);
        }
        if (sub == 0 && fok) C[(size_t)r * k + f] = t;
      }
      acc = 0.f;
      GCN_ROW_WALK_NEXT(rowptr, m)
    };

    while (pos == row_end) flush();                 // leading empty rows (chunk 0 only)

    int   cj_nx = 0;
    float vj_nx = 0.f;
    if (start + lane < end) { cj_nx = col[start + lane]; vj_nx = val[start + lane]; }
    for (int base = start; base < end; base += 64) {
      const int cnt = min(64, end - base);
      const int   cj = cj_nx;
      const float vj = vj_nx;
      if (base + 64 + lane < end) { cj_nx = col[base + 64 + lane]; vj_nx = val[base + 64 + lane]; }

      for (int j = 0; j < cnt; j += U * NPI) {
        float prod[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {               // U gather instructions back to back
          const int e = j + u * NPI + sub;          // this lane's non-zero inside the 64-block
          const int   cu = __shfl(cj, e & 63);
          const float vu = __shfl(vj, e & 63);
          float b = 0.f;
          if (e < cnt && fok) {
            if (BUF) {
              b = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                      rsrc, (int)((unsigned)cu * row_bytes + (unsigned)f * 4u), 0, 0));
            } else {
              b = B[(size_t)cu * (size_t)k + f];
            }
          }
          prod[u] = (e < cnt && fok) ? vu * b : 0.f;  // lanes past the block's end / past k add nothing
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int n_step = min(NPI, cnt - (j + u * NPI));     // non-zeros this step really holds
          if (n_step <= 0) break;
          if (row_end < 0 || row_end - pos > n_step) {          // fast path: no row ends in this step
            acc += prod[u];
            pos += n_step;
            continue;
          }
          int done = 0;                             // sub-slots of this step already summed
          while (true) {
            const int rel = row_end - pos;          // non-zeros the current row still has from `pos`
            if (row_end < 0 || rel > n_step - done) {           // row continues past this step
              acc += (sub >= done) ? prod[u] : 0.f;
              pos += n_step - done;
              break;
            }
            acc += (sub >= done && sub < done + rel) ? prod[u] : 0.f;
            pos += rel;
            done += rel;
            flush();                                // (may run again at once for empty rows)
            if (done == n_step && pos != row_end) break;
          }
        }
      }
    }

    if (last_flush != end) {                        // the row piece that sticks out of the chunk
      float t = acc;
#pragma unroll
      for (int off = G; off < 64; off <<= 1) t += __shfl_xor(t, off);
      const int slot = head ? 2 * c : 2 * c + 1;
      if (sub == 0 && fok) P[(size_t)slot * k + f] = t;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// k in 9..16 (G = 16, four non-zeros per gather) with the cross-lane traffic on DPP instead of
// ds_bpermute: the 64-entry (col, val) block is loaded TRANSPOSED — lane s*16 + u holds entry
// u*4 + s — so that at step u every 16-lane DPP row broadcasts its lane u (`row_newbcast:u`,
// a modifier on a full-rate v_mov) and lane (s, f) receives exactly the non-zero 4u + s it
// gathers for.  Per-lane byte offsets use the 24-bit multiplier (needs n < 2^24 and buffer
// addressing; otherwise the generic kernel above runs).
// ---------------------------------------------------------------------------------------------
template <bool EPI>
__global__ void __launch_bounds__(256)
spmm_narrow16_dpp_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                         const float* __restrict__ val, const float* __restrict__ B,
                         float* __restrict__ C, float* __restrict__ P,
                         const int* __restrict__ chunk_row, const float* __restrict__ bias,
                         const int* __restrict__ nnz_dev,
                         int relu, int nchunks, int T, int m, int nnz, int k) {
  constexpr int NPI = 4;
  dropin_shape(nnz_dev, T, nnz, nchunks, col, val);
  const int lane = threadIdx.x & 63;
  const int wib  = sgpr(threadIdx.x >> 6);
  const int sub  = lane >> 4;
  const int f    = lane & 15;
  const bool fok = f < k;
  const int tl   = (lane & 15) * 4 + (lane >> 4);   // transposed position this lane loads

  const ChunkRange range(wib, nchunks);

  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(B), 0, 0xFFFFFFFFu, 0x00020000);
  const unsigned row_bytes = (unsigned)k * 4u;
  const unsigned foff = (unsigned)f * 4u;
  const float bias_f = (EPI && bias && fok) ? bias[f] : 0.f;

  for (int c = range.first; c < range.c_hi; c += range.stride) {
    const int start = c * T;
    const int end   = (int)min((long long)start + T, (long long)nnz);
    GCN_ROW_WALK_OPEN(rowptr, chunk_row, c, T, m);     // r, row_end, row_end_nx, head, pos, last_flush (chunk_walk.h)
    float acc = 0.f;

    auto flush = [&]() {
      float t = acc;
      t += __shfl_xor(t, 16);
      t += __shfl_xor(t, 32);
      if (head) {
        if (sub == 0 && fok) P[(size_t)(2 * c) * k + f] = t;
      } else if (last_flush != pos) {               // (empty rows belong to launch_fill_empty_rows, spmm_kernels.hip)
        if (EPI) {
          t += bias_f;
          if (relu) t = relu_keep_nan(t);
        }
        if (sub == 0 && fok) C[(size_t)r * k + f] = t;
      }
      acc = 0.f;
      GCN_ROW_WALK_NEXT(rowptr, m)
    };
    // one step = the 4 non-zeros at [pos, pos + n_step)
    auto step = [&](float prod, int n_step) {
      if (row_end < 0 || row_end - pos > n_step) { acc += prod; pos += n_step; return; }
      int done = 0;
      while (true) {
        const int rel = row_end - pos;
        if (row_end < 0 || rel > n_step - done) {
          acc += (sub >= done) ? prod : 0.f;
          pos += n_step - done;
          return;
        }
        acc += (sub >= done && sub < done + rel) ? prod : 0.f;
        pos += rel;
        done += rel;
        flush();
        if (done == n_step && pos != row_end) return;
      }
    };

    while (pos == row_end) flush();

    int   cj_nx = 0;
    float vj_nx = 0.f;
    if (start + tl < end) { cj_nx = col[start + tl]; vj_nx = val[start + tl]; }
    for (int base = start; base < end; base += 64) {
      const int cnt = min(64, end - base);
      const int cj = cj_nx;
      const int vj = __builtin_bit_cast(int, vj_nx);
      if (base + 64 + tl < end) { cj_nx = col[base + 64 + tl]; vj_nx = val[base + 64 + tl]; }

#define GCN_N16_GATHER(UU)                                                                      \
      {                                                                                         \
        const int cu = quad_bcast<16, UU>(cj);                                                   \
        const float vu = __builtin_bit_cast(float, quad_bcast<16, UU>(vj));                      \
        const bool ok = (UU * 4 + sub < cnt) && fok;                                            \
        float b = 0.f;                                                                          \
        if (ok) b = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(             \
                        rsrc, (int)(__umul24((unsigned)cu, row_bytes) + foff), 0, 0));          \
        prod[UU] = ok ? vu * b : 0.f;                                                       \
      }
#define GCN_N16_STEP(UU)                                                                        \
      { const int ns = min(NPI, cnt - UU * 4); if (ns > 0) step(prod[UU], ns); }
      float prod[16];
      GCN_N16_GATHER(0) GCN_N16_GATHER(1) GCN_N16_GATHER(2) GCN_N16_GATHER(3)
      GCN_N16_GATHER(4) GCN_N16_GATHER(5) GCN_N16_GATHER(6) GCN_N16_GATHER(7)
      GCN_N16_GATHER(8) GCN_N16_GATHER(9) GCN_N16_GATHER(10) GCN_N16_GATHER(11)
      GCN_N16_GATHER(12) GCN_N16_GATHER(13) GCN_N16_GATHER(14) GCN_N16_GATHER(15)
      GCN_N16_STEP(0) GCN_N16_STEP(1) GCN_N16_STEP(2) GCN_N16_STEP(3)
      GCN_N16_STEP(4) GCN_N16_STEP(5) GCN_N16_STEP(6) GCN_N16_STEP(7)
      GCN_N16_STEP(8) GCN_N16_STEP(9) GCN_N16_STEP(10) GCN_N16_STEP(11)
      GCN_N16_STEP(12) GCN_N16_STEP(13) GCN_N16_STEP(14) GCN_N16_STEP(15)
#undef GCN_N16_GATHER
#undef GCN_N16_STEP
    }

    if (last_flush != end) {
      float t = acc;
      t += __shfl_xor(t, 16);
      t += __shfl_xor(t, 32);
      const int slot = head ? 2 * c : 2 * c + 1;
      if (sub == 0 && fok) P[(size_t)slot * k + f] = t;
    }
  }
}

template <int G>
static hipError_t launch_g(const SpmmArgs& a, const ChunkChoice& c, int nblocks, hipStream_t s) {
  const dim3 grid(nblocks), block(256);
  if (c.buf) {
    if (c.epi) spmm_narrow_kernel<G, G, true, true><<<grid, block, 0, s>>>(GCN_CHUNK_ARGS(a));
    else       spmm_narrow_kernel<G, G, false, true><<<grid, block, 0, s>>>(GCN_CHUNK_ARGS(a));
  } else {
    if (c.epi) spmm_narrow_kernel<G, G, true, false><<<grid, block, 0, s>>>(GCN_CHUNK_ARGS(a));
    else       spmm_narrow_kernel<G, G, false, false><<<grid, block, 0, s>>>(GCN_CHUNK_ARGS(a));
  }
  return hipGetLastError();
}

// G lanes per non-zero and U = G gather instructions per batch: one 64-entry (col, val) block per batch
hipError_t launch_spmm_narrow(const SpmmArgs& a, const ChunkChoice& c, int nblocks, hipStream_t s) {
  if (c.family == ChunkFamily::narrow16_dpp) {
    if (c.epi) spmm_narrow16_dpp_kernel<true><<<dim3(nblocks), dim3(256), 0, s>>>(GCN_CHUNK_ARGS(a));
    else       spmm_narrow16_dpp_kernel<false><<<dim3(nblocks), dim3(256), 0, s>>>(GCN_CHUNK_ARGS(a));
    return hipGetLastError();
  }
  switch (c.lanes) {
    case 4:  return launch_g<4>(a, c, nblocks, s);
    case 8:  return launch_g<8>(a, c, nblocks, s);
    default: return launch_g<16>(a, c, nblocks, s);
  }
}

}  // namespace gcn
