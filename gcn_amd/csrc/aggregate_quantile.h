// aggregate_quantile.h — launchers of aggregate_quantile.hip: up to four order statistics (PyG's QuantileAggregation with
// interpolation="lower"; q = 0.5 is torch.median's lower median, Median-GCN's reduction) of every CSR row's neighbourhood,
// with the entry that supplied each (plan-free, capturable, kernels only: see the file's header).  All operands fp32.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace gcn {

constexpr int kQuantileMax = 4;                        // ranks per call
constexpr int kQuantileShort = 32;                     // rows of at most this many entries are sorted in registers
constexpr size_t kQuantileWsBytes = 16;                // two flag words (a row above kQuantileShort / above kSampleLongRow)

// out, arg [m, nq * k]: plane i (columns i k ..) is the element of rank floor(q[i] (d - 1)) of every column of a row of d
// entries and its index into col; q: nq <= kQuantileMax HOST doubles in [0, 1]; ws: kQuantileWsBytes
hipError_t launch_aggregate_quantile(const int* rowptr, const int* col, int m, int nnz, const float* x, int k, const double* q,
                                     int nq, float* out, int* arg, void* ws, hipStream_t st);

}  // namespace gcn
