// relational.h — launchers of relational.hip: the relation-typed aggregation of basis R-GCN (one gather per stored entry,
// B planes side by side) and its two gradients (plan-free, capturable, no atomics: see the file's header).  All operands
// fp32, row-major; etype int32 [nnz] in entry order; coeff [R, B] or null (typed mode, B == R); values [nnz] or null (ones).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace gcn {

constexpr int kRelMaxPlanes = 8;                       // planes (bases) of one pass of the forward and of the coeff gradient

// ws: a flag and one float per (chunk of kAggChunk entries, long row, column, plane of the widest pass: 1, 2, 4 or 8);
// every pass of the three walks on a pattern, its transpose and its relation-major view shares it
size_t relation_workspace_bytes(int nnz, int k, int B);

// out [m, B k], plane b at columns b k .. b k + k - 1
hipError_t launch_relation_aggregate(const int* rowptr, const int* col, const int* etype, int m, int nnz, const float* x, int k,
                                     const float* coeff, int R, int B, const float* values, float* out, void* ws, hipStream_t st);
// g [m, B k]; gx [n, k]; the transposed pattern, etype and values addressed through tperm
hipError_t launch_relation_aggregate_backward_x(const int* trowptr, const int* trow, const int* tperm, const int* etype, int n,
                                                int nnz, const float* g, int k, const float* coeff, int R, int B,
                                                const float* values, float* gx, void* ws, hipStream_t st);
// the relation-major view: relptr [R + 1] and, per entry in type-major stable order, its row, its column and its index in
// the CSR (rperm; values is read through it); entries from relptr[R] on (types outside [0, R)) are not walked.
// gcoeff [R, B]
hipError_t launch_relation_aggregate_backward_coeff(const int* relptr, const int* rrow, const int* rcol, const int* rperm, int R,
                                                    int nnz, const float* g, const float* x, int k, int B, const float* values,
                                                    float* gcoeff, void* ws, hipStream_t st);

}  // namespace gcn
