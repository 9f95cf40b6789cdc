// sddmm.hip — sampled dense-dense product on the pattern of a plan: out[e] = sum_j A[row(e), j] * B[col(e), j] for every
// stored entry e.  It is the gradient of an SpMM with respect to its values (d(A_hat B)/d val = SDDMM(grad_out, B)).
//
// Its traffic is the SpMM's: one gathered row of B per entry.  So on a sliced plan it walks the slice-major virtual CSR
// (slicing.hip) for the same L2 reason the SpMM does — XCD x walks the contiguous eighth x of the chunks, i.e. about S/8
// column slices of B one after the other.  Sliced plans have column-sorted rows, so the entries of virtual row (s, r) are
// one contiguous run of CSR row r; Slicing::vsrc holds where that run starts, and results go straight back to CSR order.
//
// Engine: 16 lanes per chunk of T entries, four engines per wave.  A batch is 16 consecutive entries: lane q finds the row
// of entry q from the next 16 row ends (no per-entry map), then, per 64-column pass, the engine gathers 16 B bytes per lane
// for each of the 16 entries and multiplies them with A[row] held in registers (the row of the batch's first and last
// entry; a third row in one batch is read where it is met).  The 16 lanes' partial sums of the 16 entries are reduced by
// one reduce-scatter (8 + 4 + 2 + 1 exchanges), after which lane q owns entry q: one store per lane, one writer per output,
// no atomics.  Every entry is summed in the same order — its lane's columns in pass order, then the same tree over the 16
// lanes — whatever walk (sliced, CSR) or batch slot feeds it, so results are bit-identical across plans and calls.
#include <hip/hip_runtime.h>

#include <climits>

#include "spmm_kernels.h"

namespace gcn {
namespace {

constexpr int kSddmmEngines = 16;                      // engines (chunks) per block of 256 threads

template <bool VEC>
__device__ __forceinline__ float4 load4(const float* __restrict__ row, int c0, int k) {
  if (VEC) return c0 < k ? *reinterpret_cast<const float4*>(row + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
  float4 v;
  v.x = c0 < k ? row[c0] : 0.f;
  v.y = c0 + 1 < k ? row[c0 + 1] : 0.f;
  v.z = c0 + 2 < k ? row[c0 + 2] : 0.f;
  v.w = c0 + 3 < k ? row[c0 + 3] : 0.f;
  return v;
}

__device__ __forceinline__ float dot4(float acc, const float4& a, const float4& b) {
  acc = fmaf(a.x, b.x, acc);
  acc = fmaf(a.y, b.y, acc);
  acc = fmaf(a.z, b.z, acc);
  return fmaf(a.w, b.w, acc);
}

// acc[j] = lane q's partial sum of entry j -> the whole sum of entry q.  Each step halves the entries a lane keeps and
// adds its partner's share: entry j is always summed over the lane pairs {l, l^8}, then {.., ^4}, {.., ^2}, {.., ^1}
// (float addition commutes, so it does not matter which of the two lanes adds).
__device__ __forceinline__ float reduce_scatter16(float (&acc)[16], int q) {
  float v8[8], v4[4], v2[2];
  const bool h8 = q & 8, h4 = q & 4, h2 = q & 2, h1 = q & 1;
#pragma unroll
  for (int i = 0; i < 8; ++i) v8[i] = (h8 ? acc[i + 8] : acc[i]) + __shfl_xor(h8 ? acc[i] : acc[i + 8], 8, 16);
#pragma unroll
  for (int i = 0; i < 4; ++i) v4[i] = (h4 ? v8[i + 4] : v8[i]) + __shfl_xor(h4 ? v8[i] : v8[i + 4], 4, 16);
#pragma unroll
  for (int i = 0; i < 2; ++i) v2[i] = (h2 ? v4[i + 2] : v4[i]) + __shfl_xor(h2 ? v4[i] : v4[i + 2], 2, 16);
  return (h1 ? v2[1] : v2[0]) + __shfl_xor(h1 ? v2[0] : v2[1], 1, 16);
}

}  // namespace

// SLICED: rowptr / col / chunk_row are the virtual CSR of the plan's slicing (rows = S*m, row vr is part of row vr % m
// and its entries start at CSR position vsrc[vr]); otherwise the caller's CSR (rows = m).
template <bool SLICED, bool VEC>
__global__ void __launch_bounds__(256)
sddmm_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, const int* __restrict__ chunk_row,
             const int* __restrict__ vsrc, const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ out,
             int rows, int m, int nnz, int T, int nchunks, int k) {
  const int q = threadIdx.x & 15;
  // XCD-aware chunk ranges (as spmm_chunk_kernel): blocks b and b+8 share an XCD, so XCD x walks blocks
  // [x*G/8, (x+1)*G/8) of the chunk stream — on a sliced plan about S/8 consecutive column slices
  const int lb = (blockIdx.x & 7) * (int)(gridDim.x >> 3) + (int)(blockIdx.x >> 3);
  const int c = lb * kSddmmEngines + (int)(threadIdx.x >> 4);
  const bool live = c < nchunks;
  const long long e_lo = (long long)c * T;
  const long long e_hi = live ? (e_lo + T < nnz ? e_lo + T : (long long)nnz) : e_lo;
  int cur = live ? chunk_row[c] : 0;                   // the row holding the batch's first entry
  const int passes = (k + 63) >> 6;
  // every lane runs T / 16 batches (shuffles need the whole engine); a batch past the chunk's end has nb = 0
  for (int bi = 0; bi < T / 16; ++bi) {
    const long long b = e_lo + 16LL * bi;
    const int nb = e_hi - b >= 16 ? 16 : (e_hi > b ? (int)(e_hi - b) : 0);
    const bool mine = q < nb;
    const int e = mine ? (int)(b + q) : 0;
    // row of entry e: cur + the number of the next 16 row ends that are <= e (more only past empty rows: walked on)
    const int rr = cur + 1 + q;
    const int rend = (nb > 0 && rr <= rows) ? rowptr[rr] : INT_MAX;
    int cnt = 0;
#pragma unroll
    for (int l = 0; l < 16; ++l) cnt += __shfl(rend, l, 16) <= e ? 1 : 0;
    int rq = cur + cnt, cq = 0, aq = 0, dst = 0;
    if (mine) {
      if (cnt == 16)
        while (rowptr[rq + 1] <= e) ++rq;
      cq = col[e];
      if (SLICED) {
        aq = rq % m;
        dst = vsrc[rq] + (e - rowptr[rq]);
      } else {
        aq = rq;
        dst = e;
      }
    }
    // (columns and rows of the 16 entries are fetched from their lanes where they are used, each pass: the registers
    //  they would hold cost more occupancy than the exchanges cost time)
    const int a_first = __shfl(aq, 0, 16), a_last = __shfl(aq, nb > 0 ? nb - 1 : 0, 16);
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
    for (int p = 0; p < passes; ++p) {
      const int c0 = p * 64 + 4 * q;
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 a0 = nb > 0 ? load4<VEC>(A + (size_t)a_first * k, c0, k) : z;
      const float4 a1 = nb > 0 ? load4<VEC>(A + (size_t)a_last * k, c0, k) : z;
#pragma unroll
      for (int h = 0; h < 16; h += 8) {                // eight gathers in flight per lane, then their FMAs
        float4 bv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int cb = __shfl(cq, h + j, 16);
          bv[j] = h + j < nb ? load4<VEC>(B + (size_t)cb * k, c0, k) : z;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (h + j < nb) {
            const int r = __shfl(aq, h + j, 16);
            const float4 a = r == a_first ? a0 : (r == a_last ? a1 : load4<VEC>(A + (size_t)r * k, c0, k));
            acc[h + j] = dot4(acc[h + j], a, bv[j]);
          }
        }
      }
    }
    const float tot = reduce_scatter16(acc, q);
    if (mine) out[dst] = tot;
    cur = __shfl(rq, 15, 16);                          // (entry b+15's row: where the next batch starts)
  }
}

bool sddmm_vec(const float* A, const float* B, int k) {
  return k % 4 == 0 && (((uintptr_t)A | (uintptr_t)B) & 15) == 0;
}

hipError_t launch_sddmm(const SddmmArgs& s, hipStream_t st) {
  if (s.nchunks <= 0 || s.k <= 0) return hipSuccess;
  if (s.T <= 0 || s.T % 16 != 0) return hipErrorInvalidValue;
  int blocks = (s.nchunks + kSddmmEngines - 1) / kSddmmEngines;
  blocks = (blocks + 7) / 8 * 8;                       // a whole number of blocks per XCD
  const bool vec = sddmm_vec(s.A, s.B, s.k);
  const bool sliced = s.vsrc != nullptr;
#define GCN_SDDMM(SL, V) sddmm_kernel<SL, V><<<blocks, 256, 0, st>>>(s.rowptr, s.col, s.chunk_row, s.vsrc, s.A, s.B, s.out, \
                                                                    s.rows, s.m, s.nnz, s.T, s.nchunks, s.k)
  if (sliced) { if (vec) GCN_SDDMM(true, true); else GCN_SDDMM(true, false); }
  else        { if (vec) GCN_SDDMM(false, true); else GCN_SDDMM(false, false); }
#undef GCN_SDDMM
  return hipGetLastError();
}

}  // namespace gcn
