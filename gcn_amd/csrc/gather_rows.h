// gather_rows.h — "walk a row's entries, gather a feature row per entry, fold it into a per-column state", the dispatch by
// row length written once for the plan-free gather units: aggregate.hip (max / min and its backward) and multihead.hip
// (spmm_heads and the two backward walks of gatv2_scores).  What a lane keeps and how a wave walks a run of entries is the
// unit's; everything around the walk is here.
//
// The shape.  A wave is 64 / LPS entry slots x LPS lanes x VEC columns; lane l has the columns j .. j + VEC,
// j = (blockIdx.y * LPS + l % LPS) * VEC: a k wider than LPS * VEC columns is tiled over blockIdx.y.  The host never reads
// a row length:
//   * gather_rows_kernel: a wave owns 8 consecutive rows and takes them one after the other (for_wave_rows, long_chunks.h);
//     a row of more than kAggChunk entries is left alone and a flag, the first word of the workspace, is raised;
//   * gather_long_partial_kernel: a fixed grid of waves walks the chunks of kAggChunk entries (for_long_segments; they
//     return at once while the flag is down), finds the at most two long rows that meet a chunk and writes the state of
//     each segment to the workspace, one Partial per (chunk, row, column): 16 bytes behind the flag, plane t of Op::NS (a
//     lane may keep NS states per column), row 2 c + slot, column j, the planes one behind the other;
//   * gather_long_finish_kernel: one writer per row — the wave whose chunk holds the row's first entry merges the row's
//     partials in chunk order, a column per lane, and writes the row.  A hub row is spread over the chip.
// Only a memset node and kernels (legal inside a stream capture), no atomics, every reduction in a fixed order.
//
// An Op (a kernel argument, passed by value) supplies
//   VEC, LPS, NS; int k                 columns per lane, lanes per slot, states per column; the row width
//   Acc                                 the lane's state for its VEC columns (a plain array or an aggregate)
//   Row                                 what reduce fetches of the row itself (declared beside Acc, in the kernel: as a local
//                                       of reduce it moves the GATv2 backward kernels by an occupancy step)
//   Partial                             one column of one state in the workspace
//   Lane lane_ctx(j, jok)               what is fixed per lane for the whole kernel, computed once before the row loop
//   void reduce(r, b, n, lane, j, jok, const Lane&, Row&, Acc&)
//                                       init, the unit's walk over the entries [b, b + n) of row r (n <= kAggChunk) and
//                                       the merge of the slots: lanes 0 .. LPS - 1 end with the state of their columns
//                                       (jok: the lane's columns exist; the other lanes walk along and keep nothing)
//   void store(r, j, const Acc&)        columns j .. j + VEC of row r from the state of the whole row
//   static Partial partial(const Acc&, t, v)
//                                       state t of column j + v
//   static void merge_next(Partial&, Partial)
//                                       a partial of LATER entries into the state of earlier ones
//   void store_one(r, j, t, Partial)    column j of row r from its merged state t
// Device code and its launcher only: the ops live in the two units' anonymous namespaces.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "long_chunks.h"
#include "spmm_kernels.h"

namespace gcn {

constexpr int kRowsPerWave = 8;
constexpr int kGatherChunk = kAggChunk;                // entries per chunk of the long-row kernels
constexpr int kGatherLong = kAggChunk;                 // rows longer than this are split over waves (>= the chunk: long_segment)
constexpr int kGatherLongWaves = 8192;                 // waves of the long-row kernels (they loop over the chunks)

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// VEC consecutive floats at p: one 16-byte access (p on a 16-byte boundary) or one element.  (ROUND: for the overloads
// that store a narrower type.)
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
template <int VEC, bool ROUND = false>
__device__ __forceinline__ void store_row(float* p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    static_assert(VEC == 1);
    p[0] = v[0];
  }
}

template <class Op>
__global__ void __launch_bounds__(256) gather_rows_kernel(Op op, const int* __restrict__ rowptr, int rows, int* __restrict__ long_flag) {
  const int lane = threadIdx.x & 63;
  const int j = (blockIdx.y * Op::LPS + lane % Op::LPS) * Op::VEC;
  const bool jok = j < op.k;
  const typename Op::Lane ctx = op.lane_ctx(j, jok);
  for_wave_rows<kRowsPerWave, kGatherLong>(rowptr, rows, lane, long_flag, [&](int r, int b, int n) {
    typename Op::Row row;
    typename Op::Acc acc;
    op.reduce(r, b, n, lane, j, jok, ctx, row, acc);
    if (lane < Op::LPS && jok) op.store(r, j, acc);
  });
}

template <class Op>
__global__ void __launch_bounds__(256) gather_long_partial_kernel(Op op, const int* __restrict__ rowptr, int rows, int nnz, int nchunks,
                                                                  const int* __restrict__ long_flag,
                                                                  typename Op::Partial* __restrict__ part) {
  if (*long_flag == 0) return;
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = gridDim.x * 4;
  const int j = (blockIdx.y * Op::LPS + lane % Op::LPS) * Op::VEC;
  const bool jok = j < op.k;
  const typename Op::Lane ctx = op.lane_ctx(j, jok);
  for_long_segments<kGatherChunk, kGatherLong>(rowptr, rows, nnz, nchunks, wave, nwaves, lane, [&](int c, int slot, const Segment& sg) {
    typename Op::Row row;
    typename Op::Acc acc;
    op.reduce(sg.r, sg.sb, sg.se - sg.sb, lane, j, jok, ctx, row, acc);
    if (lane < Op::LPS && jok) {
#pragma unroll
      for (int t = 0; t < Op::NS; ++t) {
        typename Op::Partial* p = part + ((size_t)t * 2 * nchunks + 2 * (size_t)c + slot) * op.k + j;
#pragma unroll
        for (int v = 0; v < Op::VEC; ++v) p[v] = Op::partial(acc, t, v);
      }
    }
  });
}

template <class Op>
__global__ void __launch_bounds__(256) gather_long_finish_kernel(Op op, const int* __restrict__ rowptr, int rows, int nnz, int nchunks,
                                                                 const int* __restrict__ long_flag,
                                                                 const typename Op::Partial* __restrict__ part) {
  if (*long_flag == 0) return;
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = gridDim.x * 4;
  const int j0 = blockIdx.y * Op::LPS * Op::VEC;
  const int j1 = j0 + Op::LPS * Op::VEC < op.k ? j0 + Op::LPS * Op::VEC : op.k;
  for_long_segments<kGatherChunk, kGatherLong>(rowptr, rows, nnz, nchunks, wave, nwaves, lane, [&](int c, int slot, const Segment& sg) {
    // the row's partials: chunks c_first..c_last, the first in slot 1 unless the row starts on the chunk's first entry
    const int c_first = sg.rb / kGatherChunk, c_last = (sg.re - 1) / kGatherChunk;
    if (c != c_first) return;
    const int first_slot = sg.rb > c_first * kGatherChunk ? 1 : 0;
    for (int j = j0 + lane; j < j1; j += 64) {
#pragma unroll
      for (int t = 0; t < Op::NS; ++t) {
        const typename Op::Partial* pt = part + (size_t)t * 2 * nchunks * op.k;
        typename Op::Partial acc = pt[(2 * (size_t)c_first + first_slot) * op.k + j];
        for (int cc = c_first + 1; cc <= c_last; ++cc) Op::merge_next(acc, pt[2 * (size_t)cc * op.k + j]);
        op.store_one(sg.r, j, t, acc);
      }
    }
  });
}

// ws: the flag word, and from byte 16 on Op::NS planes of 2 * ceil(nnz / kAggChunk) rows of k partials
template <class Op>
hipError_t run_gather(const Op& op, const int* rowptr, int rows, int nnz, void* ws, hipStream_t st) {
  int* flag = static_cast<int*>(ws);
  auto part = reinterpret_cast<typename Op::Partial*>(static_cast<char*>(ws) + 16);
  const long long tiles = ((long long)op.k + Op::LPS * Op::VEC - 1) / (Op::LPS * Op::VEC);
  if (tiles > 65535) return hipErrorInvalidValue;      // (the grid's y extent)
  if (hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), st); e != hipSuccess) return e;
  const long long waves = ((long long)rows + kRowsPerWave - 1) / kRowsPerWave;
  gather_rows_kernel<Op><<<dim3((unsigned)((waves + 3) / 4), (unsigned)tiles), 256, 0, st>>>(op, rowptr, rows, flag);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  if (nnz <= kGatherLong) return hipSuccess;           // (no row can be long)
  const int nchunks = (int)(((long long)nnz + kGatherChunk - 1) / kGatherChunk);
  const int nw = nchunks < kGatherLongWaves ? nchunks : kGatherLongWaves;
  const dim3 grid((unsigned)((nw + 3) / 4), (unsigned)tiles);
  gather_long_partial_kernel<Op><<<grid, 256, 0, st>>>(op, rowptr, rows, nnz, nchunks, flag, part);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  gather_long_finish_kernel<Op><<<grid, 256, 0, st>>>(op, rowptr, rows, nnz, nchunks, flag, part);
  return hipGetLastError();
}

}  // namespace gcn
