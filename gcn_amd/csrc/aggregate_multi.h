// aggregate_multi.h — launchers of aggregate_multi.hip: max, min, sum, mean, variance and standard deviation over the stored
// entries of every CSR row from ONE gather per entry, and the gradient of all of them in one walk of the transposed pattern
// (plan-free, capturable, no atomics: see the file's header).  All operands fp32, row-major.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace gcn {

// the statistics, numbered as GCN_REDUCE_* (include/gcn_spmm.h)
constexpr int kMultiMax = 0, kMultiMin = 1, kMultiSum = 2, kMultiMean = 3, kMultiVar = 4, kMultiStd = 5, kMultiStats = 6;

// where each statistic goes: plane at[s] of the nred planes of out (columns at[s] * k ..), -1 = not requested
struct MultiPlanes {
  signed char at[kMultiStats];
  int nred;
  bool has(int s) const { return at[s] >= 0; }
  bool moments() const { return has(kMultiVar) || has(kMultiStd); }
  bool extrema() const { return has(kMultiMax) || has(kMultiMin); }
  bool affine() const { return has(kMultiSum) || has(kMultiMean) || moments(); }
};

// ws: a flag and one 32-byte whole-column state per (chunk of kAggChunk entries, long row, column)
size_t aggregate_multi_workspace_bytes(int nnz, int k);

// out [m, nred * k]; argmax / argmin [m, k] where that plane is requested; save_mean [m, k] or null (the mean again, for a
// backward of var / std without a mean plane)
hipError_t launch_aggregate_multi(const int* rowptr, const int* col, int m, int nnz, const float* x, int k, MultiPlanes pl, float eps,
                                  float* out, int* argmax, int* argmin, float* save_mean, void* ws, hipStream_t st);
// every row empty: zeros, and -1 in the arg arrays
hipError_t launch_aggregate_multi_empty(int m, int k, MultiPlanes pl, float* out, int* argmax, int* argmin, float* save_mean,
                                        hipStream_t st);
// g [m, nred * k]; out: the forward's (read where var / std need the mean and std planes); ab [m, 2 k]: scratch of the
// prepass (null without sum / mean / var / std); gx [n, k]
hipError_t launch_aggregate_multi_backward(const int* trowptr, const int* trow, const int* tperm, const int* rowptr, int n, int m,
                                           int nnz, const float* g, const float* x, int k, MultiPlanes pl, const float* out,
                                           const int* argmax, const int* argmin, const float* save_mean, float* ab, float* gx,
                                           void* ws, hipStream_t st);
// count 32-bit words at p set to `word`, by a kernel (count > 0)
hipError_t launch_fill_words(void* p, size_t count, unsigned word, hipStream_t st);

}  // namespace gcn
