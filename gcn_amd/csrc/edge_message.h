// Internal interface between api_units.cpp and edge_message.hip, in the manner of spmm_kernels.h: the launchers of the
// edge-feature aggregation (u_op_e -> reduce) and its two backward kernels.  Not installed; the public contract is
// include/gcn_spmm.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace gcn {

// edge_message.hip — out[r, :] = reduce over the entries e of row r of act(x[col[e], :] op w[e, :]), with the entry index
// of a max / min, and the gradients of the sum in x (a walk of the transposed pattern) and in w (a per-entry kernel)
// (plan-free, capturable, no atomics: see the file's header).  x [n x k], w [nnz x k] in the CSR's entry order, out [m x k],
// all fp32 row-major; offsets into w and ge are size_t (nnz * k may pass 2^31).  ws: edge_aggregate_workspace_bytes(nnz, k)
// bytes of device memory — a flag and one partial per (chunk of kAggChunk entries, long row, column).
constexpr int kEdgeOpAdd = 0, kEdgeOpMul = 1;          // GCN_EDGE_OP_ADD / GCN_EDGE_OP_MUL
constexpr int kEdgeActNone = 0, kEdgeActRelu = 1;      // GCN_EDGE_ACT_NONE / GCN_EDGE_ACT_RELU
constexpr int kEdgeReduceSum = 2;                      // GCN_REDUCE_SUM, beside kAggMax / kAggMin
size_t edge_aggregate_workspace_bytes(int nnz, int k);
hipError_t launch_edge_aggregate(const int* rowptr, const int* col, int m, int nnz, const float* x, const float* w, int k, int op,
                                 int act, int reduce, float* out, int* arg, void* ws, hipStream_t st);
hipError_t launch_edge_aggregate_backward_x(const int* trowptr, const int* trow, const int* tperm, int n, int nnz, const float* g,
                                            const float* x, const float* w, int k, int op, int act, float* gx, void* ws,
                                            hipStream_t st);
hipError_t launch_edge_aggregate_backward_e(const int* rowptr, const int* col, int m, int nnz, const float* g, const float* x,
                                            const float* w, int k, int op, int act, float* ge, void* ws, hipStream_t st);

}  // namespace gcn
