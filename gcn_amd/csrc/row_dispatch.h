// row_dispatch.h — "one row per workgroup, long rows to a bigger workgroup", written once for the plan-free units that
// work row by row: sample.hip, subgraph.hip (induced subgraph) and coalesce.hip (merge, degrees, normalisation).  An item
// (a row, a node, a seed) gets one wave when its row has at most kSampleLongRow entries and a 256-thread workgroup when it
// has more; both run the op's row function, which is written once over THREADS.  An Op supplies
//   int count, nnz                      items to serve; entries of the matrix (nnz <= kSampleLongRow: no row can be long)
//   using Row                           an aggregate with at least int b, e: the row's entries [b, e)
//   bool locate(int i, Row&) const      item i's row, or false when the item, its row pointer or its output slot is unusable
//   template <int THREADS> Scratch      the op's own LDS
//   template <int THREADS> void row(int i, const Row&, Scratch<THREADS>&) const
//                                       called by every thread of the workgroup with the same arguments
// Device code and its launcher only: included by the three units, whose ops live in their anonymous namespaces.
// FLAG says at compile time whether the call has a flag word (launch_rows: an int*, or the literal nullptr): tested at run
// time, the pointer costs the long kernel of the sampler four more spilled SGPRs and 111 more reloads of them.
//
// The screening loop.  rows_kernel (one wave per item) leaves a long row alone and raises the flag.  long_rows_kernel is a
// fixed grid of G <= kLongBlocks workgroups that leave at once while the flag is down; workgroup b owns the items b, b + G,
// b + 2G, ... (`mine` of them: neighbouring hubs land on different workgroups) and screens them 256 at a time, thread t the
// item b + (q0 + t) * G, into is_long[].  After the first barrier every thread reads the same is_long[t], so the `continue`
// and the call of row() are workgroup-uniform and the barriers inside row() are met by all 256 threads.  The barrier after a
// row keeps the next row from overwriting the op's scratch under a wave that is still reading it; the barrier at the end of
// a window keeps the next screening from overwriting is_long[] under a wave that is still walking it.  A single row is never
// spread over several workgroups.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>

#include "spmm_kernels.h"

namespace gcn {

constexpr int kLongBlocks = 1024;                      // workgroups of the long-row kernel (they loop over the items)

template <class Op, bool FLAG>
__global__ void __launch_bounds__(64) rows_kernel(Op op, int* __restrict__ long_flag) {
  __shared__ typename Op::template Scratch<64> L;
  const int i = blockIdx.x;
  typename Op::Row r;
  if (!op.locate(i, r)) return;                        // (the workgroup's one wave leaves as a whole)
  if (r.e - r.b > kSampleLongRow) {
    if constexpr (FLAG)
      if (threadIdx.x == 0) *long_flag = 1;            // (every writer writes the same word)
    return;
  }
  op.template row<64>(i, r, L);
}

template <class Op, bool FLAG>
__global__ void __launch_bounds__(256) long_rows_kernel(Op op, const int* __restrict__ long_flag) {
  __shared__ struct {                                  // (one object: two would each be padded to 16 bytes)
    typename Op::template Scratch<256> L;
    int is_long[256];
  } S;
  if constexpr (FLAG)
    if (*long_flag == 0) return;
  const int G = gridDim.x;
  const int mine = (op.count - (int)blockIdx.x + G - 1) / G;
  for (int q0 = 0; q0 < mine; q0 += 256) {
    const int q = q0 + threadIdx.x;
    typename Op::Row r;
    S.is_long[threadIdx.x] = q < mine && op.locate(blockIdx.x + q * G, r) && r.e - r.b > kSampleLongRow;
    __syncthreads();
    const int top = mine - q0 < 256 ? mine - q0 : 256;
    for (int t = 0; t < top; ++t) {
      if (!S.is_long[t]) continue;                      // (workgroup-uniform)
      const int i = blockIdx.x + (q0 + t) * G;
      op.locate(i, r);
      op.template row<256>(i, r, S.L);
      __syncthreads();                                 // (the next row overwrites the op's scratch)
    }
    __syncthreads();                                   // (the next screening overwrites is_long)
  }
}

// flag: one int of device scratch (an int*, zeroed here) or the literal nullptr, in which case the long kernel screens
// unconditionally
template <class Op, class Flag>
hipError_t launch_rows(const Op& op, Flag flag, hipStream_t st) {
  constexpr bool FLAG = !std::is_same_v<Flag, std::nullptr_t>;
  int* const word = flag;
  if constexpr (FLAG)
    if (hipError_t err = hipMemsetAsync(word, 0, sizeof(int), st); err != hipSuccess) return err;
  rows_kernel<Op, FLAG><<<(unsigned)op.count, 64, 0, st>>>(op, word);
  if (hipError_t err = hipGetLastError(); err != hipSuccess) return err;
  if (op.nnz <= kSampleLongRow) return hipSuccess;     // (no row can be long)
  long_rows_kernel<Op, FLAG><<<(unsigned)(op.count < kLongBlocks ? op.count : kLongBlocks), 256, 0, st>>>(op, word);
  return hipGetLastError();
}

// The ordered slot hand-out of a pass over a row: `mask` is this wave's ballot of the lanes that take an output slot in pass
// p, `run` the slots handed out by the passes so far (workgroup-uniform; advanced here).  Returns the first slot of this
// wave: run + the counts of the lower waves, exchanged through cnt[p & 1][] with ONE barrier per pass — the other parity
// is what a wave one pass ahead writes, and two passes ahead it has met this pass's barrier.  A lane's own slot is the
// return value + the popcount of mask below it.  Every thread of the workgroup calls it, once per pass.
template <int WAVES>
__device__ __forceinline__ int ordered_slots(unsigned long long mask, int p, int (&cnt)[2][WAVES], int& run) {
  int base = run;
  if constexpr (WAVES > 1) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) cnt[p & 1][wave] = __popcll(mask);
    __syncthreads();
    for (int w = 0; w < WAVES; ++w) {
      const int k = cnt[p & 1][w];
      if (w < wave) base += k;
      run += k;
    }
  } else {
    run += __popcll(mask);
  }
  return base;
}

}  // namespace gcn
