// segment_mm.h — launchers of segment_mm.hip: the gathered, segmented matrix product (a weight per segment of rows: DGL's
// segment_mm / gather_mm, pyg_lib's segment_matmul) on the matrix cores, and its weight gradient (plan-free, capturable, no
// atomics: see the file's header).  All operands fp32, row-major; segptr int32 [T + 1] on the device, never read by the host.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace gcn {

constexpr int kSegTM = 64;                             // rows of a forward tile (one segment's)
constexpr int kSegTN = 64;                             // output columns of a tile, both kernels; also the weight gradient's K tile
constexpr int kSegChunk = 512;                         // rows of one partial of the weight gradient: a constant of the ABI

// ws: 3 T + 7 ints (the segment bounds made monotone, the tile prefix, the chunk prefix), padded to 16 bytes, then one
// [K, O] partial per possible chunk of the weight gradient: ceil(N / kSegChunk) + T of them
size_t segment_mm_workspace_bytes(int N, int T, int K, int O);

// y [N, O]: y[i] = scale[i] * (x[x_index ? x_index[i] : i] @ op(W[t(i)])); rows outside [segptr[0], segptr[T]) are zeroed.
// W [T, K, O], or [T, O, K] read as its transpose with transpose_w.  An index outside [0, x_rows) reads a row of zeros.
hipError_t launch_segment_mm(const float* x, int x_rows, const int* x_index, const float* scale, const int* segptr,
                             const float* W, int transpose_w, int N, int T, int K, int O, float* y, void* ws, hipStream_t st);
// dW [T, K, O]: dW[t] = sum over the rows i of segment t of scale[i] * x[xi(i)]^T (x) g[gi(i)], chunks added in order
hipError_t launch_segment_mm_wgrad(const float* x, int x_rows, const int* x_index, const float* g, int g_rows,
                                   const int* g_index, const float* scale, const int* segptr, int N, int T, int K, int O,
                                   float* dW, void* ws, hipStream_t st);

}  // namespace gcn
