// api_units.cpp — the native C ABI of libgcnspmm.so: the plan-free units (edge softmax, head-batched attention, GATv2 scores,
// max / min aggregation, edge-feature aggregation, sampling, subgraphs and walks, entry lookup, bucketing, coalescing, SpGEMM, sampled dot, kNN, row
// gather).  Each entry point is the argument checks of include/gcn_spmm.h in front of one launcher of spmm_kernels.h (edge_message.h).
#include "edge_message.h"
#include "plan_policy.h"

using namespace gcn;

extern "C" {

// Edge softmax family (edge_softmax.hip): plan-free, on the caller's CSR.  Common argument check: sizes, the row pointer
// and the workspace (GCN_EDGE_WS_BYTES(nnz)); 1 = nothing to do, 0 = go on, else the status to return.
static int edge_args(const int32_t* rowptr, int32_t m, int32_t nnz, const void* ws, size_t ws_bytes, int* status) {
  *status = GCN_OK;
  if (m < 0 || nnz < 0) { *status = GCN_ERR_INVALID_ARG; return 1; }
  if (m == 0 || nnz == 0) return 1;
  if (!rowptr || !ws || ws_bytes < edge_workspace_bytes(nnz)) { *status = GCN_ERR_INVALID_ARG; return 1; }
  return 0;
}

int gcn_edge_softmax_csr_f32(const int32_t* rowptr, int32_t m, int32_t nnz, const float* scores, float* p, void* ws,
                             size_t ws_bytes, void* stream) {
  int rc;
  if (edge_args(rowptr, m, nnz, ws, ws_bytes, &rc)) return rc;
  if (!scores || !p) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_edge_softmax(rowptr, m, nnz, scores, p, ws, (hipStream_t)stream));
}

int gcn_edge_softmax_backward_csr_f32(const int32_t* rowptr, int32_t m, int32_t nnz, const float* p, const float* g,
                                      float* ds, void* ws, size_t ws_bytes, void* stream) {
  int rc;
  if (edge_args(rowptr, m, nnz, ws, ws_bytes, &rc)) return rc;
  if (!p || !g || !ds) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_edge_softmax_backward(rowptr, m, nnz, p, g, ds, ws, (hipStream_t)stream));
}

int gcn_gat_edge_softmax_csr_f32(const int32_t* rowptr, const int32_t* col, int32_t m, int32_t nnz, const float* a_dst,
                                 const float* a_src, float negative_slope, float* p, void* ws, size_t ws_bytes, void* stream) {
  int rc;
  if (edge_args(rowptr, m, nnz, ws, ws_bytes, &rc)) return rc;
  if (!col || !a_dst || !a_src || !p) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_gat_edge_softmax(rowptr, col, m, nnz, a_dst, a_src, negative_slope, p, ws, (hipStream_t)stream));
}

int gcn_gat_edge_softmax_backward_csr_f32(const int32_t* rowptr, const int32_t* col, int32_t m, int32_t nnz,
                                          const float* a_dst, const float* a_src, float negative_slope, const float* p,
                                          const float* g, float* ds, float* grad_a_dst, void* ws, size_t ws_bytes,
                                          void* stream) {
  int rc;
  if (edge_args(rowptr, m, nnz, ws, ws_bytes, &rc)) return rc;
  if (!col || !a_dst || !a_src || !p || !g || !ds || !grad_a_dst) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_gat_edge_softmax_backward(rowptr, col, m, nnz, a_dst, a_src, negative_slope, p, g, ds, grad_a_dst, ws,
                                                     (hipStream_t)stream));
}

int gcn_segment_sum_csr_f32(const int32_t* rowptr, int32_t m, int32_t nnz, const float* x, const int32_t* perm, float* out,
                            void* ws, size_t ws_bytes, void* stream) {
  int rc;
  if (edge_args(rowptr, m, nnz, ws, ws_bytes, &rc)) return rc;
  if (!x || !out) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_segment_sum(rowptr, m, nnz, x, perm, out, ws, (hipStream_t)stream));
}

// Head-batched attention primitives (edge_softmax.hip with H heads, multihead.hip).  Sizes first — heads, k and nnz * heads < 2^31 before any pointer is
// looked at — then the empty problem, then the row pointer and the workspace; 1 = return *status.  k = 0: the call takes no k.
static int heads_args(const int32_t* rowptr, int32_t rows, int32_t nnz, int32_t heads, int32_t k, const void* ws, size_t ws_bytes,
                      size_t ws_need, int* status) {
  *status = GCN_ERR_INVALID_ARG;
  if (rows < 0 || nnz < 0 || heads < 1 || k < 0) return 1;
  if ((long long)nnz * heads >= (1LL << 31)) return 1;
  if (k && (k < heads || k % heads != 0 || k > 16 * 65535)) return 1;
  *status = GCN_OK;
  if (rows == 0 || nnz == 0) return 1;
  if (!rowptr || !ws || ws_bytes < ws_need) { *status = GCN_ERR_INVALID_ARG; return 1; }
  return 0;
}

int gcn_heads_ws_bytes(int32_t m, int32_t nnz, int32_t heads, int32_t k, size_t* bytes) {
  int rc;
  if (!bytes || k < 1) return GCN_ERR_INVALID_ARG;
  heads_args(nullptr, 0, nnz, heads, k, nullptr, 0, 0, &rc);                  // (the size rules alone)
  if (rc != GCN_OK || m < 0) return GCN_ERR_INVALID_ARG;
  const size_t e = edge_workspace_bytes(nnz, heads), s = heads_spmm_workspace_bytes(nnz, k);
  *bytes = e > s ? e : s;
  return GCN_OK;
}

int gcn_edge_softmax_heads_csr_f32(const int32_t* rowptr, int32_t m, int32_t nnz, int32_t heads, const float* scores, float* p,
                                   void* ws, size_t ws_bytes, void* stream) {
  int rc;
  if (heads_args(rowptr, m, nnz, heads, 0, ws, ws_bytes, edge_workspace_bytes(nnz, heads > 0 ? heads : 1), &rc)) return rc;
  if (!scores || !p) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_edge_softmax_heads(rowptr, m, nnz, heads, scores, p, ws, (hipStream_t)stream));
}

int gcn_edge_softmax_heads_backward_csr_f32(const int32_t* rowptr, int32_t m, int32_t nnz, int32_t heads, const float* p,
                                            const float* g, float* ds, void* ws, size_t ws_bytes, void* stream) {
  int rc;
  if (heads_args(rowptr, m, nnz, heads, 0, ws, ws_bytes, edge_workspace_bytes(nnz, heads > 0 ? heads : 1), &rc)) return rc;
  if (!p || !g || !ds) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_edge_softmax_heads_backward(rowptr, m, nnz, heads, p, g, ds, ws, (hipStream_t)stream));
}

int gcn_gat_edge_softmax_heads_csr_f32(const int32_t* rowptr, const int32_t* col, int32_t m, int32_t nnz, int32_t heads,
                                       const float* a_dst, const float* a_src, float negative_slope, float* p, void* ws,
                                       size_t ws_bytes, void* stream) {
  int rc;
  if (heads_args(rowptr, m, nnz, heads, 0, ws, ws_bytes, edge_workspace_bytes(nnz, heads > 0 ? heads : 1), &rc)) return rc;
  if (!col || !a_dst || !a_src || !p) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_gat_edge_softmax_heads(rowptr, col, m, nnz, heads, a_dst, a_src, negative_slope, p, ws,
                                                  (hipStream_t)stream));
}

int gcn_gat_edge_softmax_heads_backward_csr_f32(const int32_t* rowptr, const int32_t* col, int32_t m, int32_t nnz, int32_t heads,
                                                const float* a_dst, const float* a_src, float negative_slope, const float* p,
                                                const float* g, float* ds, float* grad_a_dst, void* ws, size_t ws_bytes,
                                                void* stream) {
  int rc;
  if (heads_args(rowptr, m, nnz, heads, 0, ws, ws_bytes, edge_workspace_bytes(nnz, heads > 0 ? heads : 1), &rc)) return rc;
  if (!col || !a_dst || !a_src || !p || !g || !ds || !grad_a_dst) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_gat_edge_softmax_heads_backward(rowptr, col, m, nnz, heads, a_dst, a_src, negative_slope, p, g, ds,
                                                           grad_a_dst, ws, (hipStream_t)stream));
}

int gcn_segment_sum_heads_csr_f32(const int32_t* rowptr, int32_t rows, int32_t nnz, int32_t heads, const float* x,
                                  const int32_t* perm, float* out, void* ws, size_t ws_bytes, void* stream) {
  int rc;
  if (heads_args(rowptr, rows, nnz, heads, 0, ws, ws_bytes, edge_workspace_bytes(nnz, heads > 0 ? heads : 1), &rc)) return rc;
  if (!x || !out) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_segment_sum_heads(rowptr, rows, nnz, heads, x, perm, out, ws, (hipStream_t)stream));
}

int gcn_spmm_heads_csr_f32(const int32_t* rowptr, const int32_t* idx, const int32_t* perm, int32_t rows, int32_t nnz, int32_t heads,
                           int32_t k, const float* vals, const float* x, float* out, void* ws, size_t ws_bytes, void* stream) {
  int rc;
  if (k < 1) return GCN_ERR_INVALID_ARG;
  if (heads_args(rowptr, rows, nnz, heads, k, ws, ws_bytes, heads_spmm_workspace_bytes(nnz, k), &rc)) return rc;
  if (!idx || !vals || !x || !out) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_spmm_heads(rowptr, idx, perm, rows, nnz, heads, k, vals, x, out, ws, (hipStream_t)stream));
}

int gcn_sddmm_heads_csr_f32(const int32_t* rowptr, const int32_t* col, int32_t m, int32_t nnz, int32_t heads, int32_t k,
                            const float* a, const float* b, float* out, void* ws, size_t ws_bytes, void* stream) {
  int rc;
  if (k < 1) return GCN_ERR_INVALID_ARG;
  if (heads_args(rowptr, m, nnz, heads, k, ws, ws_bytes, kHeadsSddmmWsBytes, &rc)) return rc;
  if (!col || !a || !b || !out) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_sddmm_heads(rowptr, col, m, nnz, heads, k, a, b, out, ws, (hipStream_t)stream));
}

int gcn_gatv2_ws_bytes(int32_t m, int32_t nnz, int32_t heads, int32_t k, size_t* bytes) {
  int rc;
  if (!bytes || k < 1) return GCN_ERR_INVALID_ARG;
  heads_args(nullptr, 0, nnz, heads, k, nullptr, 0, 0, &rc);                  // (the size rules alone)
  if (rc != GCN_OK || m < 0) return GCN_ERR_INVALID_ARG;
  *bytes = gatv2_workspace_bytes(nnz, k);
  return GCN_OK;
}

int gcn_gatv2_scores_csr_f32(const int32_t* rowptr, const int32_t* col, int32_t m, int32_t nnz, int32_t heads, int32_t k,
                             const float* h_dst, const float* h_src, const float* att, float negative_slope, float* out, void* ws,
                             size_t ws_bytes, void* stream) {
  int rc;
  if (k < 1) return GCN_ERR_INVALID_ARG;
  if (heads_args(rowptr, m, nnz, heads, k, ws, ws_bytes, gatv2_workspace_bytes(nnz, k), &rc)) return rc;
  if (!col || !h_dst || !h_src || !att || !out) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_gatv2_scores(rowptr, col, m, nnz, heads, k, h_dst, h_src, att, negative_slope, out, ws,
                                        (hipStream_t)stream));
}

int gcn_gatv2_scores_backward_csr_f32(const int32_t* rowptr, const int32_t* idx, const int32_t* perm, int32_t rows, int32_t nnz,
                                      int32_t heads, int32_t k, const float* own, const float* other, const float* att,
                                      float negative_slope, const float* g, float* grad_own, float* act_sums, void* ws,
                                      size_t ws_bytes, void* stream) {
  int rc;
  if (k < 1) return GCN_ERR_INVALID_ARG;
  if (heads_args(rowptr, rows, nnz, heads, k, ws, ws_bytes, gatv2_workspace_bytes(nnz, k), &rc)) return rc;
  if (!idx || !own || !other || !att || !g || !grad_own) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_gatv2_scores_backward(rowptr, idx, perm, rows, nnz, heads, k, own, other, att, negative_slope, g,
                                                 grad_own, act_sums, ws, (hipStream_t)stream));
}

// k, op / dtype and the sizes first; then what an empty problem still needs; 1 = return *status
static int aggregate_args(int32_t rows_out, int32_t rows_in, int32_t nnz, int32_t dtype, int32_t k, int* status) {
  *status = GCN_OK;
  if (rows_out < 0 || rows_in < 0 || nnz < 0 || k < 1 || (dtype != GCN_DTYPE_F32 && dtype != GCN_DTYPE_BF16)) {
    *status = GCN_ERR_INVALID_ARG;
    return 1;
  }
  if (k > 16 * 65535) { *status = GCN_ERR_INVALID_ARG; return 1; }       // (column tiles ride in gridDim.y)
  return rows_out == 0;
}

int gcn_aggregate_csr(const int32_t* rowptr, const int32_t* col, int32_t m, int32_t n, int32_t nnz, const void* x, int32_t dtype,
                      int32_t k, int32_t op, void* out, int32_t* arg, void* ws, size_t ws_bytes, void* stream) {
  int rc;
  if (op != GCN_REDUCE_MAX && op != GCN_REDUCE_MIN) return GCN_ERR_INVALID_ARG;
  if (aggregate_args(m, n, nnz, dtype, k, &rc)) return rc;
  if (!out || !arg) return GCN_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const size_t elems = (size_t)m * (size_t)k, esize = dtype == GCN_DTYPE_BF16 ? 2 : 4;
  if (nnz == 0) {                                       // every row is empty: zeros and -1, as memset nodes
    if (hipMemsetAsync(out, 0, elems * esize, st) != hipSuccess) return GCN_ERR_HIP;
    return hip_status(hipMemsetAsync(arg, 0xff, elems * 4, st));
  }
  if (!rowptr || !col || !x || !ws || ws_bytes < aggregate_workspace_bytes(nnz, k)) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_aggregate(rowptr, col, m, nnz, x, dtype == GCN_DTYPE_BF16, k, op == GCN_REDUCE_MAX ? kAggMax : kAggMin,
                                     out, arg, ws, st));
}

int gcn_aggregate_backward_csr(const int32_t* trowptr, const int32_t* trow, const int32_t* tperm, int32_t n, int32_t m, int32_t nnz,
                               const void* g, int32_t dtype, const int32_t* arg, int32_t k, void* gx, void* ws, size_t ws_bytes,
                               void* stream) {
  int rc;
  if (aggregate_args(n, m, nnz, dtype, k, &rc)) return rc;
  if (!gx) return GCN_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (nnz == 0)
    return hip_status(hipMemsetAsync(gx, 0, (size_t)n * (size_t)k * (dtype == GCN_DTYPE_BF16 ? 2 : 4), st));
  if (!trowptr || !trow || !tperm || !g || !arg || !ws || ws_bytes < aggregate_workspace_bytes(nnz, k)) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_aggregate_backward(trowptr, trow, tperm, n, nnz, g, dtype == GCN_DTYPE_BF16, arg, k, gx, ws, st));
}

static_assert(kEdgeOpAdd == GCN_EDGE_OP_ADD && kEdgeOpMul == GCN_EDGE_OP_MUL && kEdgeActNone == GCN_EDGE_ACT_NONE &&
              kEdgeActRelu == GCN_EDGE_ACT_RELU && kEdgeReduceSum == GCN_REDUCE_SUM && kAggMax == GCN_REDUCE_MAX &&
              kAggMin == GCN_REDUCE_MIN, "include/gcn_spmm.h");

// Edge-feature aggregation (edge_message.hip).  k, the constants and the sizes first (nnz * k may pass 2^31: it is no
// bound); then what an empty problem still needs; 1 = return *status
static int edge_aggregate_args(int32_t rows_out, int32_t rows_in, int32_t nnz, int32_t k, int32_t op, int32_t act, int* status) {
  *status = GCN_ERR_INVALID_ARG;
  if (rows_out < 0 || rows_in < 0 || nnz < 0 || k < 1 || k > 16 * 65535) return 1;     // (column tiles ride in gridDim.y)
  if ((op != GCN_EDGE_OP_ADD && op != GCN_EDGE_OP_MUL) || (act != GCN_EDGE_ACT_NONE && act != GCN_EDGE_ACT_RELU)) return 1;
  *status = GCN_OK;
  return rows_out == 0;
}

int gcn_edge_aggregate_csr_f32(const int32_t* rowptr, const int32_t* col, int32_t m, int32_t n, int32_t nnz, const float* x,
                               const float* w, int32_t k, int32_t op, int32_t act, int32_t reduce, float* out, int32_t* arg,
                               void* ws, size_t ws_bytes, void* stream) {
  int rc;
  if (reduce != GCN_REDUCE_MAX && reduce != GCN_REDUCE_MIN && reduce != GCN_REDUCE_SUM) return GCN_ERR_INVALID_ARG;
  if (edge_aggregate_args(m, n, nnz, k, op, act, &rc)) return rc;
  const bool select = reduce != GCN_REDUCE_SUM;
  if (!out || (select && !arg)) return GCN_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const size_t elems = (size_t)m * (size_t)k;
  if (nnz == 0) {                                       // every row is empty: zeros and -1, as memset nodes
    if (hipMemsetAsync(out, 0, elems * 4, st) != hipSuccess) return GCN_ERR_HIP;
    return select ? hip_status(hipMemsetAsync(arg, 0xff, elems * 4, st)) : GCN_OK;
  }
  if (!rowptr || !col || !x || !w || !ws || ws_bytes < edge_aggregate_workspace_bytes(nnz, k)) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_edge_aggregate(rowptr, col, m, nnz, x, w, k, op, act, reduce, out, arg, ws, st));
}

int gcn_edge_aggregate_backward_x_csr_f32(const int32_t* trowptr, const int32_t* trow, const int32_t* tperm, int32_t n, int32_t m,
                                          int32_t nnz, const float* g, const float* x, const float* w, int32_t k, int32_t op,
                                          int32_t act, float* gx, void* ws, size_t ws_bytes, void* stream) {
  int rc;
  if (edge_aggregate_args(n, m, nnz, k, op, act, &rc)) return rc;
  if (!gx) return GCN_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (nnz == 0) return hip_status(hipMemsetAsync(gx, 0, (size_t)n * (size_t)k * 4, st));
  if (!trowptr || !trow || !tperm || !g || !x || !w || !ws || ws_bytes < edge_aggregate_workspace_bytes(nnz, k))
    return GCN_ERR_INVALID_ARG;
  return hip_status(launch_edge_aggregate_backward_x(trowptr, trow, tperm, n, nnz, g, x, w, k, op, act, gx, ws, st));
}

int gcn_edge_aggregate_backward_e_csr_f32(const int32_t* rowptr, const int32_t* col, int32_t m, int32_t n, int32_t nnz,
                                          const float* g, const float* x, const float* w, int32_t k, int32_t op, int32_t act,
                                          float* ge, void* ws, size_t ws_bytes, void* stream) {
  int rc;
  if (edge_aggregate_args(m, n, nnz, k, op, act, &rc)) return rc;
  if (nnz == 0) return GCN_OK;                          // (ge has no element)
  if (!rowptr || !col || !g || !x || !w || !ge || !ws || ws_bytes < edge_aggregate_workspace_bytes(nnz, k))
    return GCN_ERR_INVALID_ARG;
  return hip_status(launch_edge_aggregate_backward_e(rowptr, col, m, nnz, g, x, w, k, op, act, ge, ws, (hipStream_t)stream));
}

int gcn_sample_neighbors_csr(const int32_t* rowptr, const int32_t* col, int32_t m, int32_t nnz, const int32_t* seeds, int32_t n_seeds,
                             int32_t fanout, uint64_t seed, uint64_t offset, const int32_t* out_rowptr, int32_t* out_col,
                             int32_t* out_eid, void* ws, size_t ws_bytes, void* stream) {
  if (m < 0 || nnz < 0 || n_seeds < 0 || fanout == 0) return GCN_ERR_INVALID_ARG;
  if (n_seeds == 0) return GCN_OK;
  if (!seeds || !out_rowptr) return GCN_ERR_INVALID_ARG;
  if (m == 0 || nnz == 0) return GCN_OK;                // (no seed is in range / every row is empty: nothing to write)
  if (!rowptr || !col || !out_col || !out_eid || !ws || ws_bytes < kSampleWsBytes) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_sample_neighbors(rowptr, col, m, nnz, seeds, n_seeds, fanout, seed, offset, out_rowptr, out_col, out_eid,
                                            ws, (hipStream_t)stream));
}

static_assert(kSampleLongRow == GCN_SAMPLE_LONG_ROW && kSampleWsBytes == GCN_SAMPLE_WS_BYTES, "include/gcn_spmm.h");

// sizes first; then what an empty problem still needs; 1 = return *status
static int subgraph_args(int32_t m, int32_t nnz, int32_t n_nodes, const int32_t* nodes, int* status) {
  *status = GCN_OK;
  if (m < 0 || nnz < 0 || n_nodes < 0) { *status = GCN_ERR_INVALID_ARG; return 1; }
  if (n_nodes == 0) return 1;
  if (!nodes) { *status = GCN_ERR_INVALID_ARG; return 1; }
  return 0;
}

int gcn_induced_subgraph_count_csr(const int32_t* rowptr, const int32_t* col, int32_t m, int32_t nnz, const int32_t* nodes,
                                   int32_t n_nodes, const int32_t* vmap, int32_t* out_len, void* ws, size_t ws_bytes,
                                   void* stream) {
  int rc;
  if (subgraph_args(m, nnz, n_nodes, nodes, &rc)) return rc;
  if (!out_len) return GCN_ERR_INVALID_ARG;
  if (m == 0 || nnz == 0) return GCN_OK;                // (no node is in range / every row is empty: nothing to write)
  if (!rowptr || !col || !vmap || !ws || ws_bytes < kSubgraphWsBytes) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_induced_subgraph_count(rowptr, col, m, nnz, nodes, n_nodes, vmap, out_len, ws, (hipStream_t)stream));
}

int gcn_induced_subgraph_fill_csr(const int32_t* rowptr, const int32_t* col, int32_t m, int32_t nnz, const int32_t* nodes,
                                  int32_t n_nodes, const int32_t* vmap, const int32_t* out_rowptr, int32_t* out_col,
                                  int32_t* out_eid, void* ws, size_t ws_bytes, void* stream) {
  int rc;
  if (subgraph_args(m, nnz, n_nodes, nodes, &rc)) return rc;
  if (!out_rowptr) return GCN_ERR_INVALID_ARG;
  if (m == 0 || nnz == 0) return GCN_OK;
  if (!rowptr || !col || !vmap || !out_col || !out_eid || !ws || ws_bytes < kSubgraphWsBytes) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_induced_subgraph_fill(rowptr, col, m, nnz, nodes, n_nodes, vmap, out_rowptr, out_col, out_eid, ws,
                                                 (hipStream_t)stream));
}

static_assert(kSubgraphWsBytes == GCN_SUBGRAPH_WS_BYTES, "include/gcn_spmm.h");

int gcn_random_walk_csr(const int32_t* rowptr, const int32_t* col, int32_t m, int32_t nnz, const int32_t* starts, int32_t n_walks,
                        int32_t length, uint64_t seed, uint64_t offset, int32_t* out_walks, void* stream) {
  if (m < 0 || nnz < 0 || n_walks < 0 || length < 0) return GCN_ERR_INVALID_ARG;
  if (n_walks == 0) return GCN_OK;
  if (!starts || !out_walks || (m > 0 && !rowptr) || (m > 0 && nnz > 0 && !col)) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_random_walk(rowptr, col, m, nnz, starts, n_walks, length, seed, offset, out_walks, (hipStream_t)stream));
}

int gcn_csr_find_entries(const int32_t* rowptr, const int32_t* col, int32_t m, int32_t nnz, const int32_t* q_rows,
                         const int32_t* q_cols, int32_t n_queries, int32_t* out_eid, void* stream) {
  if (m < 0 || nnz < 0 || n_queries < 0) return GCN_ERR_INVALID_ARG;
  if (n_queries == 0) return GCN_OK;
  if (!q_rows || !q_cols || !out_eid || (m > 0 && !rowptr) || (m > 0 && nnz > 0 && !col)) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_find_entries(rowptr, col, m, nnz, q_rows, q_cols, n_queries, out_eid, (hipStream_t)stream));
}

int gcn_negative_sample_csr(const int32_t* rowptr, const int32_t* col, int32_t m, int32_t n, int32_t nnz, const int32_t* q_rows,
                            int32_t n_queries, int32_t num_neg, int32_t max_tries, int32_t exclude_self, uint64_t seed,
                            uint64_t offset, int32_t* out_cols, void* stream) {
  if (m < 0 || n < 0 || nnz < 0 || n_queries < 0 || num_neg < 1 || max_tries < 1 || max_tries > 64) return GCN_ERR_INVALID_ARG;
  if ((long long)n_queries * num_neg >= (1ll << 31)) return GCN_ERR_INVALID_ARG;
  if (n_queries == 0) return GCN_OK;
  if (n < 1 || !q_rows || !out_cols || (m > 0 && !rowptr) || (m > 0 && nnz > 0 && !col)) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_negative_sample(rowptr, col, m, n, nnz, q_rows, n_queries * num_neg, num_neg, max_tries,
                                           exclude_self != 0, seed, offset, out_cols, (hipStream_t)stream));
}

static_assert(kBucketWaveMax == GCN_BUCKET_WAVE_MAX && kBucketBlockMax == GCN_BUCKET_BLOCK_MAX, "include/gcn_spmm.h");

int gcn_bucket_count_i32(const int32_t* keys, int32_t count, int32_t nbuckets, int32_t* offsets, void* stream) {
  if (count < 0 || nbuckets < 0 || !offsets || (count > 0 && nbuckets > 0 && !keys)) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_bucket_count(keys, count, nbuckets, offsets, (hipStream_t)stream));
}

int gcn_bucket_fill_i32(const int32_t* keys, int32_t count, int32_t nbuckets, const int32_t* offsets, int32_t* perm, void* ws,
                        size_t ws_bytes, void* stream) {
  if (count < 0 || nbuckets < 0) return GCN_ERR_INVALID_ARG;
  if (count == 0 || nbuckets == 0) return GCN_OK;
  if (!keys || !offsets || !perm || !ws || ws_bytes < bucket_workspace_bytes(count, nbuckets)) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_bucket_fill(keys, count, nbuckets, offsets, perm, ws, (hipStream_t)stream));
}

int gcn_csr_transpose_gather(const int32_t* rowptr, int32_t m, int32_t nnz, const int32_t* perm, const float* val, int32_t* trow,
                             float* tval, void* stream) {
  if (m < 0 || nnz < 0 || (val == nullptr) != (tval == nullptr)) return GCN_ERR_INVALID_ARG;
  if (nnz == 0) return GCN_OK;
  if (m == 0 || !rowptr || !perm || !trow) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_transpose_gather(rowptr, m, nnz, perm, val, trow, tval, (hipStream_t)stream));
}

static_assert(kCoalesceWsBytes == GCN_COALESCE_WS_BYTES && kCoalesceSum == GCN_COALESCE_SUM && kCoalesceMax == GCN_COALESCE_MAX &&
              kCoalesceMin == GCN_COALESCE_MIN && kCoalesceFirst == GCN_COALESCE_FIRST && kDiagKeep == GCN_DIAG_KEEP &&
              kDiagDrop == GCN_DIAG_DROP && kDiagFill == GCN_DIAG_FILL && kDiagAdd == GCN_DIAG_ADD && kNormSym == GCN_NORM_SYM &&
              kNormRow == GCN_NORM_ROW, "include/gcn_spmm.h");

int gcn_csr_coalesce_count(const int32_t* rowptr, const int32_t* col, int32_t m, int32_t n, int32_t nnz, int32_t diagonal,
                           int32_t* out_len, void* ws, size_t ws_bytes, void* stream) {
  if (m < 0 || n < 0 || nnz < 0 || diagonal < GCN_DIAG_KEEP || diagonal > GCN_DIAG_ADD) return GCN_ERR_INVALID_ARG;
  if (m == 0) return GCN_OK;
  if (!rowptr || (nnz > 0 && !col) || !out_len || !ws || ws_bytes < kCoalesceWsBytes) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_csr_coalesce_count(rowptr, col, m, n, nnz, diagonal, out_len, ws, (hipStream_t)stream));
}

int gcn_csr_coalesce_fill(const int32_t* rowptr, const int32_t* col, const float* val, int32_t m, int32_t n, int32_t nnz,
                          int32_t reduce, int32_t diagonal, float diag_value, const int32_t* out_rowptr, int32_t* out_col,
                          float* out_val, int32_t* out_first, int32_t* seg, void* ws, size_t ws_bytes, void* stream) {
  if (m < 0 || n < 0 || nnz < 0 || reduce < GCN_COALESCE_SUM || reduce > GCN_COALESCE_FIRST || diagonal < GCN_DIAG_KEEP ||
      diagonal > GCN_DIAG_ADD || (val == nullptr) != (out_val == nullptr))
    return GCN_ERR_INVALID_ARG;
  if (m == 0) return GCN_OK;
  if (!rowptr || (nnz > 0 && !col) || !out_rowptr || !out_col || !ws || ws_bytes < kCoalesceWsBytes) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_csr_coalesce_fill(rowptr, col, val, m, n, nnz, reduce, diagonal, diag_value, out_rowptr, out_col,
                                             out_val, out_first, seg, ws, (hipStream_t)stream));
}

int gcn_csr_degree_f64(const int32_t* rowptr, const float* val, int32_t m, int32_t nnz, double* deg, void* stream) {
  if (m < 0 || nnz < 0) return GCN_ERR_INVALID_ARG;
  if (m == 0) return GCN_OK;
  if (!rowptr || !deg) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_csr_degree(rowptr, val, m, nnz, deg, (hipStream_t)stream));
}

int gcn_csr_normalize_f32(const int32_t* rowptr, const int32_t* col, const float* val, int32_t m, int32_t n, int32_t nnz,
                          const double* deg, int32_t mode, float* out_val, void* stream) {
  if (m < 0 || n < 0 || nnz < 0 || (mode != GCN_NORM_SYM && mode != GCN_NORM_ROW) || (mode == GCN_NORM_SYM && m != n))
    return GCN_ERR_INVALID_ARG;
  if (m == 0 || nnz == 0) return GCN_OK;
  if (!rowptr || !col || !deg || !out_val) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_csr_normalize(rowptr, col, val, m, n, nnz, deg, mode, out_val, (hipStream_t)stream));
}

static_assert(kSpgemmWaveMax == GCN_SPGEMM_WAVE_MAX && kSpgemmBlockMax == GCN_SPGEMM_BLOCK_MAX &&
              kSpgemmDenseBlocks == GCN_SPGEMM_DENSE_BLOCKS, "include/gcn_spmm.h");

int gcn_spgemm_ws_bytes(int32_t m, int32_t n, size_t* bytes) {
  if (m < 0 || n < 0 || !bytes) return GCN_ERR_INVALID_ARG;
  *bytes = spgemm_workspace_bytes(m, n);
  return GCN_OK;
}

int gcn_spgemm_count_csr(const int32_t* a_rowptr, const int32_t* a_col, int32_t m, int32_t p, int32_t nnz_a,
                         const int32_t* b_rowptr, const int32_t* b_col, int32_t n, int32_t nnz_b, int32_t* out_len, void* ws,
                         size_t ws_bytes, void* stream) {
  if (m < 0 || p < 0 || n < 0 || nnz_a < 0 || nnz_b < 0) return GCN_ERR_INVALID_ARG;
  if (m == 0) return GCN_OK;
  if (!out_len) return GCN_ERR_INVALID_ARG;
  if (nnz_a == 0 || nnz_b == 0 || p == 0 || n == 0)     // (no product exists: every row is empty)
    return hip_status(hipMemsetAsync(out_len, 0, (size_t)m * 4, (hipStream_t)stream));
  if (!a_rowptr || !a_col || !b_rowptr || !b_col || !ws || ws_bytes < spgemm_workspace_bytes(m, n)) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_spgemm_count(a_rowptr, a_col, m, p, nnz_a, b_rowptr, b_col, n, nnz_b, out_len, ws, (hipStream_t)stream));
}

int gcn_spgemm_fill_csr(const int32_t* a_rowptr, const int32_t* a_col, const float* a_val, int32_t m, int32_t p, int32_t nnz_a,
                        const int32_t* b_rowptr, const int32_t* b_col, const float* b_val, int32_t n, int32_t nnz_b,
                        const int32_t* out_rowptr, int32_t* out_col, float* out_val, void* ws, size_t ws_bytes, void* stream) {
  if (m < 0 || p < 0 || n < 0 || nnz_a < 0 || nnz_b < 0 || (out_val == nullptr) != (a_val == nullptr && b_val == nullptr))
    return GCN_ERR_INVALID_ARG;
  if (m == 0) return GCN_OK;
  if (!out_rowptr) return GCN_ERR_INVALID_ARG;
  if (nnz_a == 0 || nnz_b == 0 || p == 0 || n == 0) return GCN_OK;       // (nothing to write)
  if (!a_rowptr || !a_col || !b_rowptr || !b_col || !out_col || !ws || ws_bytes < spgemm_workspace_bytes(m, n))
    return GCN_ERR_INVALID_ARG;
  return hip_status(launch_spgemm_fill(a_rowptr, a_col, a_val, m, p, nnz_a, b_rowptr, b_col, b_val, n, nnz_b, out_rowptr, out_col,
                                       out_val, ws, (hipStream_t)stream));
}

static_assert(kSampledDotWsBytes == GCN_SAMPLED_DOT_WS_BYTES, "include/gcn_spmm.h");

int gcn_csr_sampled_dot_f32(const int32_t* p_rowptr, const int32_t* p_col, int32_t mp, int32_t np, int32_t nnz_p,
                            const int32_t* x_rowptr, const int32_t* x_col, const float* x_val, int32_t nnz_x,
                            const int32_t* y_rowptr, const int32_t* y_col, const float* y_val, int32_t nnz_y, int32_t w,
                            int32_t x_by_col, float* out, void* ws, size_t ws_bytes, void* stream) {
  if (mp < 0 || np < 0 || nnz_p < 0 || nnz_x < 0 || nnz_y < 0 || w < 0) return GCN_ERR_INVALID_ARG;
  if (mp == 0 || nnz_p == 0) return GCN_OK;
  if (!p_rowptr || !p_col || !x_rowptr || !y_rowptr || (nnz_x > 0 && !x_col) || (nnz_y > 0 && !y_col) || !out || !ws ||
      ws_bytes < kSampledDotWsBytes)
    return GCN_ERR_INVALID_ARG;
  return hip_status(launch_csr_sampled_dot(p_rowptr, p_col, mp, np, nnz_p, x_rowptr, x_col, x_val, nnz_x, y_rowptr, y_col, y_val,
                                           nnz_y, w, x_by_col, out, ws, (hipStream_t)stream));
}

static_assert(kKnnKMax == GCN_KNN_K_MAX &&kKnnTileQ == GCN_KNN_TILE_Q && kKnnTileC == GCN_KNN_TILE_C, "include/gcn_spmm.h");

namespace {
// the sizes every knn entry point refuses: negative, k outside [1, GCN_KNN_K_MAX], or more workgroups / part keys than fit
bool knn_sizes_ok(int32_t q, int32_t n, int32_t k, int32_t splits) {
  return q >= 0 && n >= 0 && k >= 1 && k <= GCN_KNN_K_MAX && splits >= 0;
}
bool knn_grid_ok(int32_t q, int eff) {
  return (((long long)q + kKnnTileQ - 1) / kKnnTileQ) * (long long)eff < (1LL << 31);
}
}  // namespace

int gcn_knn_splits(int32_t q, int32_t n, int32_t splits) {
  if (q < 0 || n < 0 || splits < 0) return -1;
  return knn_effective_splits(q, n, splits, cu_count_cached());
}

int gcn_knn_ws_bytes(int32_t q, int32_t n, int32_t k, int32_t splits, size_t* bytes) {
  if (!knn_sizes_ok(q, n, k, splits) || !bytes) return GCN_ERR_INVALID_ARG;
  const int eff = knn_effective_splits(q, n, splits, cu_count_cached());
  if (!knn_grid_ok(q, eff)) return GCN_ERR_INVALID_ARG;
  *bytes = knn_workspace_bytes(q, k, eff);
  return GCN_OK;
}

int gcn_knn_f32(const float* x, int64_t ldx, const float* y, int64_t ldy, int32_t q, int32_t n, int32_t d, int32_t k,
                int32_t self_offset, int32_t splits, int32_t* out_idx, float* out_dist2, double* out_sum, void* ws,
                size_t ws_bytes, void* stream) {
  if (!knn_sizes_ok(q, n, k, splits) || d < 1 || ldx < d || ldy < d || self_offset < -1) return GCN_ERR_INVALID_ARG;
  if (q == 0) return GCN_OK;
  const int eff = knn_effective_splits(q, n, splits, cu_count_cached());
  if (!knn_grid_ok(q, eff)) return GCN_ERR_INVALID_ARG;
  if (!x || (n > 0 && !y) || !out_idx || !ws || (reinterpret_cast<uintptr_t>(ws) & 7) != 0 ||
      ws_bytes < knn_workspace_bytes(q, k, eff))
    return GCN_ERR_INVALID_ARG;
  return hip_status(launch_knn(x, ldx, y, ldy, q, n, d, k, self_offset, eff, out_idx, out_dist2, out_sum, ws, (hipStream_t)stream));
}

int gcn_gather_rows_f32(float* dst, const float* src, const int32_t* idx, int32_t nrows, int32_t k,
                        void* stream) {
  if (nrows < 0 || k < 0) return GCN_ERR_INVALID_ARG;
  if (nrows == 0 || k == 0) return GCN_OK;
  if (!dst || !src || !idx || dst == src) return GCN_ERR_INVALID_ARG;
  return hip_status(launch_gather_rows(dst, src, idx, nrows, k, (hipStream_t)stream));
}

}  // extern "C"
