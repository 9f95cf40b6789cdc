// api_spmm.cpp — the native C ABI of libgcnspmm.so: the SpMM launches (see include/gcn_spmm.h for the contract and the
// reference interfaces each entry point replaces).  The plan behind them is built in plan_build.cpp, the rules that pick
// kernel family, tile, stride and slice set are plan_policy.cpp; the reorderers' entry points are in api_reorder.cpp, the
// reference's own symbols (flexspmm, csr2tile, ...) in api_dropin.cpp.
#include "plan_policy.h"

#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>

#define GCN_VERSION_STR "0.4.0"

using namespace gcn;

namespace {

// The copy of B a call's route asks for (r.copy), rows r.ldb floats apart (>= k, padding columns zero), scaled by u_col
// on a value-free route: row-padded, with one all-zero row more than B has (16-bit stream), or in the group kernels' layout,
// slice s at rows [s*(w+1), (s+1)*(w+1)) with row w of every slice zero (the weighted pass: the same, rows not scaled).
int relay_B(gcn_spmm_plan* p, const SpmmRoute& r, const float* B, int k, hipStream_t st) {
  const float* scale = r.valless ? p->factors.u_col : nullptr;
  if (r.copy == BCopy::group_layout) {
    const int rc = grow(p->bpad, (size_t)r.ss.table_rows() * (size_t)r.ldb);
    if (rc != GCN_OK) return rc;
    return launch_scale_rows_sliced(p->bpad, B, scale, p->n, k, r.ldb, r.ss.S, r.ss.g->w, st) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
  }
  const int rc = grow(p->bpad, ((size_t)p->n + 1) * (size_t)r.ldb);
  if (rc != GCN_OK) return rc;
  if (launch_pad_rows(p->bpad, B, p->n, k, r.ldb, st, scale) != hipSuccess ||
      hipMemsetAsync(p->bpad + (size_t)p->n * r.ldb, 0, sizeof(float) * (size_t)r.ldb, st) != hipSuccess)
    return GCN_ERR_HIP;
  return GCN_OK;
}

struct Epilogue {                                      // C = dropout(act(A*B + bias))
  const float* bias = nullptr;
  int relu = 0;
  DropoutSpec drop;
  // pre-laid output (gcn_spmm_csr_f32_prelaid; group kernels only): row r is written to row r + r / gap_w of the
  // destination and multiplied by outscale[r] — the slice-by-slice, column-scaled layout a following SpMM gathers from
  const float* outscale = nullptr;
  int gap_w = 0;
};

// The group walk of one call (spmm_group.hip; table: the sliced copy of B, fp32 or bf16, rows ld elements apart) into
// p->cv, between the events of the live kernel timing (gcn_spmm_profile_begin; null: off), and what its cut rows need.
// Rows cut by chunk ends: their later pieces are added by the caller's reduction itself (*cuts: the lists per output row),
// or — GCN_AMD_GROUP_FUSED_FIXUP=0, or a plan without the lists — by a pass of their own here, in front of it.
// (Both passes on a high-priority stream of their own, and the main kernels of two plans taking turns, were built and
//  measured for the two planes of the multi-GPU layer in r04: 0.417 / 0.450 ms against 0.377 — DESIGN §6; removed again.)
int run_group_walk(gcn_spmm_plan* p, const SliceSet& ss, bool weighted, const void* table, int elem_bytes, int ld, int k,
                   hipEvent_t ev0, hipEvent_t ev1, hipStream_t st, CutLists* cuts) {
  const GroupStream& G = *ss.g;
  GroupArgs ga = group_shape(ss, weighted, elem_bytes, ld, k);
  ga.Bp = table; ga.Cv = p->cv; ga.P = p->ws;
  if (ev0 && hipEventRecord(ev0, st) != hipSuccess) return GCN_ERR_HIP;
  if (launch_spmm_group(ga, st) != hipSuccess) return GCN_ERR_HIP;
  if (ev1 && hipEventRecord(ev1, st) != hipSuccess) return GCN_ERR_HIP;
  if (group_fused_fixup() && G.cutptr) { cuts->ptr = G.cutptr; cuts->chunk = G.cutchunk; cuts->P = p->ws; }
  else if (launch_group_fixup(G.fix, G.nfix, p->ws, p->cv, k, st) != hipSuccess) return GCN_ERR_HIP;
  return GCN_OK;
}

// One call along its route r (spmm_route) into C [m x r.k_run].  B: the caller's features (what the panel kernels read);
// Bg: what the main kernels gather from, rows r.ldb apart — B itself or the copy the route asked for.  Where
// r.reduce_epilogue is set the slice reduction carries the whole epilogue, the dropout mask included.
int spmm_impl(gcn_spmm_plan* p, const SpmmRoute& r, const int32_t* rowptr, const int32_t* col, const float* val, const float* B,
              const float* Bg, float* C, const Epilogue& epi, hipStream_t st) {
  const int k = r.k_run;
  if (grow(p->ws, ws_elems(p, k)) != GCN_OK) return GCN_ERR_ALLOC;
  if (r.S_run > 0 && grow(p->cv, (size_t)r.S_run * (size_t)p->m * (size_t)k) != GCN_OK) return GCN_ERR_ALLOC;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;             // live timing of the main kernel (gcn_spmm_profile_begin)
  if (p->prof.armed()) { const auto pr = p->prof.next(); ev0 = pr.first; ev1 = pr.second; }
  if (r.family == SpmmFamily::group) {
    // four independent 16-lane row engines per wave on the 15-bit slice-major stream (spmm_group.hip), then the per-row
    // reduction over slices
    CutLists cuts;
    if (const int rc = run_group_walk(p, r.ss, r.weighted, Bg, 4, r.ldb, k, ev0, ev1, st, &cuts); rc != GCN_OK) return rc;
    return launch_slice_reduce(p->cv, C, epi.bias, epi.relu, p->m, r.S_run, k, st, 0, r.weighted ? nullptr : p->factors.u_row.get(),
                               epi.drop, nullptr, epi.outscale, epi.gap_w, cuts) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
  }
  SpmmArgs a = spmm_args(p, r, epi.relu != 0);
  a.B = Bg; a.P = p->ws; a.ev_start = ev0; a.ev_stop = ev1;
  if (r.family == SpmmFamily::panels) {
    // A = A_in + A_out: the staged part from LDS (raw sums into C), then the rest accumulated by the
    // chunk kernel, which also carries the epilogue
    Panels& pn = p->panels;
    if (ev0 && hipEventRecord(ev0, st) != hipSuccess) return GCN_ERR_HIP;
    const int tiles = (k + 63) / 64;
    for (int t = 0; t < tiles; ++t) {
      if (launch_panel_in(pn.in_rowptr, pn.in_off, pn.in_val, B, C, pn.w0, p->m, p->n, k, pn.R, t, st, pn.dense_slot) != hipSuccess)
        return GCN_ERR_HIP;
      if (launch_panel_dense(pn.adense, pn.dense_panel, pn.ndense, B, C, pn.w0, p->m, p->n, k, pn.R, t, st) != hipSuccess)
        return GCN_ERR_HIP;
    }
    if (pn.out_nnz == 0) {
      if (launch_panel_epilogue(C, epi.bias, epi.relu, p->m, k, st) != hipSuccess) return GCN_ERR_HIP;
      if (ev1 && hipEventRecord(ev1, st) != hipSuccess) return GCN_ERR_HIP;
      return GCN_OK;
    }
    a.ev_start = nullptr;
    a.rowptr = pn.out_rowptr; a.col = pn.out_col; a.val = pn.out_val; a.chunk_row = pn.out_chunk_row;
    a.C = C; a.bias = epi.bias;
    return launch_spmm(a, p->cu_count, st) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
  }
  if (r.family == SpmmFamily::unsliced) {
    a.rowptr = rowptr; a.col = col; a.val = val; a.chunk_row = p->chunk_row;
    a.C = C; a.bias = epi.bias;
    return launch_spmm(a, p->cu_count, st) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
  }
  // sliced, four per gather: the slice-major virtual CSR (S*m rows) into the partial buffer, then the per-row reduction
  // over slices, which carries the whole epilogue (bias, ReLU, dropout mask, row factor)
  const Slicing& sl = p->slicing;
  const Col16Stream& c16 = p->col16;
  a.rowptr = sl.vrowptr; a.col = sl.vcol; a.val = r.valless ? nullptr : sl.vval.get(); a.chunk_row = sl.vchunk_row;
  if (r.col16) { a.rowptr = c16.vrowptr16; a.col = reinterpret_cast<const int*>(c16.vcol16.get()); a.chunk_row = c16.vchunk_row16; }
  a.C = p->cv;
  if (launch_spmm(a, p->cu_count, st) != hipSuccess) return GCN_ERR_HIP;
  return launch_slice_reduce(p->cv, C, epi.bias, epi.relu, p->m, r.S_run, k, st, 0, r.valless ? p->factors.u_row.get() : nullptr,
                             epi.drop) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
}

// Does a k-wide SDDMM walk the plan's slice-major copy?  Its traffic is the SpMM's (one gathered row of B per entry), so
// it follows the four-per-gather kernel's rule: from k = 33; narrower rows walk the caller's CSR.
bool sddmm_sliced(const gcn_spmm_plan* p, int k) { return p->slicing.S > 1 && p->nnz > 0 && k >= kSliceMinK; }

// The sliced SDDMM's output map (Slicing::vsrc): built with a mutable plan; a plan with fixed values builds it here, at its
// first sliced SDDMM or in gcn_spmm_plan_prepare_width (it allocates: not inside a stream capture)
int ensure_value_map(gcn_spmm_plan* p, const int32_t* rowptr, hipStream_t st) {
  Slicing& sl = p->slicing;
  std::lock_guard<std::mutex> lk(g_plan_mu);
  if (sl.vsrc) return GCN_OK;
  DevBuf<int> v;
  if (v.alloc((size_t)sl.S * (size_t)p->m) != hipSuccess) return GCN_ERR_ALLOC;
  if (build_value_map(rowptr, sl.vrowptr, p->m, sl.S, v, st) != hipSuccess) return GCN_ERR_HIP;
  sl.vsrc = std::move(v);
  return GCN_OK;
}

}  // namespace

extern "C" {

const char* gcn_version(void) { return GCN_VERSION_STR; }

int gcn_sddmm_csr_f32(gcn_spmm_plan_t* p, const int32_t* rowptr, const int32_t* col, const float* A, const float* B,
                      float* out_val, int32_t k, void* stream) {
  if (!p || k < 0) return GCN_ERR_INVALID_ARG;
  if (p->nnz == 0 || p->m == 0) return GCN_OK;
  if (!out_val) return GCN_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (k == 0)                                          // (empty sums)
    return hipMemsetAsync(out_val, 0, sizeof(float) * (size_t)p->nnz, st) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
  if (!rowptr || !col || !A || !B) return GCN_ERR_INVALID_ARG;
  SddmmArgs s;
  s.A = A; s.B = B; s.out = out_val; s.m = p->m; s.nnz = p->nnz; s.T = p->T; s.nchunks = p->nchunks; s.k = k;
  if (sddmm_sliced(p, k)) {
    const Slicing& sl = p->slicing;
    if (const int rc = ensure_value_map(p, rowptr, st); rc != GCN_OK) return rc;
    s.rowptr = sl.vrowptr; s.col = sl.vcol; s.chunk_row = sl.vchunk_row; s.vsrc = sl.vsrc; s.rows = sl.S * p->m;
  } else {
    s.rowptr = rowptr; s.col = col; s.chunk_row = p->chunk_row; s.rows = p->m;
  }
  return launch_sddmm(s, st) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
}

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
  return launch_edge_softmax(rowptr, m, nnz, scores, p, ws, (hipStream_t)stream) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
}

int gcn_edge_softmax_backward_csr_f32(const int32_t* rowptr, int32_t m, int32_t nnz, const float* p, const float* g,
                                      float* ds, void* ws, size_t ws_bytes, void* stream) {
  int rc;
  if (edge_args(rowptr, m, nnz, ws, ws_bytes, &rc)) return rc;
  if (!p || !g || !ds) return GCN_ERR_INVALID_ARG;
  return launch_edge_softmax_backward(rowptr, m, nnz, p, g, ds, ws, (hipStream_t)stream) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
}

int gcn_gat_edge_softmax_csr_f32(const int32_t* rowptr, const int32_t* col, int32_t m, int32_t nnz, const float* a_dst,
                                 const float* a_src, float negative_slope, float* p, void* ws, size_t ws_bytes, void* stream) {
  int rc;
  if (edge_args(rowptr, m, nnz, ws, ws_bytes, &rc)) return rc;
  if (!col || !a_dst || !a_src || !p) return GCN_ERR_INVALID_ARG;
  return launch_gat_edge_softmax(rowptr, col, m, nnz, a_dst, a_src, negative_slope, p, ws, (hipStream_t)stream) == hipSuccess
             ? GCN_OK : GCN_ERR_HIP;
}

int gcn_gat_edge_softmax_backward_csr_f32(const int32_t* rowptr, const int32_t* col, int32_t m, int32_t nnz,
                                          const float* a_dst, const float* a_src, float negative_slope, const float* p,
                                          const float* g, float* ds, float* grad_a_dst, void* ws, size_t ws_bytes,
                                          void* stream) {
  int rc;
  if (edge_args(rowptr, m, nnz, ws, ws_bytes, &rc)) return rc;
  if (!col || !a_dst || !a_src || !p || !g || !ds || !grad_a_dst) return GCN_ERR_INVALID_ARG;
  return launch_gat_edge_softmax_backward(rowptr, col, m, nnz, a_dst, a_src, negative_slope, p, g, ds, grad_a_dst, ws,
                                          (hipStream_t)stream) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
}

int gcn_segment_sum_csr_f32(const int32_t* rowptr, int32_t m, int32_t nnz, const float* x, const int32_t* perm, float* out,
                            void* ws, size_t ws_bytes, void* stream) {
  int rc;
  if (edge_args(rowptr, m, nnz, ws, ws_bytes, &rc)) return rc;
  if (!x || !out) return GCN_ERR_INVALID_ARG;
  return launch_segment_sum(rowptr, m, nnz, x, perm, out, ws, (hipStream_t)stream) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
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
  return launch_edge_softmax_heads(rowptr, m, nnz, heads, scores, p, ws, (hipStream_t)stream) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
}

int gcn_edge_softmax_heads_backward_csr_f32(const int32_t* rowptr, int32_t m, int32_t nnz, int32_t heads, const float* p,
                                            const float* g, float* ds, void* ws, size_t ws_bytes, void* stream) {
  int rc;
  if (heads_args(rowptr, m, nnz, heads, 0, ws, ws_bytes, edge_workspace_bytes(nnz, heads > 0 ? heads : 1), &rc)) return rc;
  if (!p || !g || !ds) return GCN_ERR_INVALID_ARG;
  return launch_edge_softmax_heads_backward(rowptr, m, nnz, heads, p, g, ds, ws, (hipStream_t)stream) == hipSuccess ? GCN_OK
                                                                                                                     : GCN_ERR_HIP;
}

int gcn_gat_edge_softmax_heads_csr_f32(const int32_t* rowptr, const int32_t* col, int32_t m, int32_t nnz, int32_t heads,
                                       const float* a_dst, const float* a_src, float negative_slope, float* p, void* ws,
                                       size_t ws_bytes, void* stream) {
  int rc;
  if (heads_args(rowptr, m, nnz, heads, 0, ws, ws_bytes, edge_workspace_bytes(nnz, heads > 0 ? heads : 1), &rc)) return rc;
  if (!col || !a_dst || !a_src || !p) return GCN_ERR_INVALID_ARG;
  return launch_gat_edge_softmax_heads(rowptr, col, m, nnz, heads, a_dst, a_src, negative_slope, p, ws, (hipStream_t)stream) ==
                 hipSuccess ? GCN_OK : GCN_ERR_HIP;
}

int gcn_gat_edge_softmax_heads_backward_csr_f32(const int32_t* rowptr, const int32_t* col, int32_t m, int32_t nnz, int32_t heads,
                                                const float* a_dst, const float* a_src, float negative_slope, const float* p,
                                                const float* g, float* ds, float* grad_a_dst, void* ws, size_t ws_bytes,
                                                void* stream) {
  int rc;
  if (heads_args(rowptr, m, nnz, heads, 0, ws, ws_bytes, edge_workspace_bytes(nnz, heads > 0 ? heads : 1), &rc)) return rc;
  if (!col || !a_dst || !a_src || !p || !g || !ds || !grad_a_dst) return GCN_ERR_INVALID_ARG;
  return launch_gat_edge_softmax_heads_backward(rowptr, col, m, nnz, heads, a_dst, a_src, negative_slope, p, g, ds, grad_a_dst, ws,
                                                (hipStream_t)stream) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
}

int gcn_segment_sum_heads_csr_f32(const int32_t* rowptr, int32_t rows, int32_t nnz, int32_t heads, const float* x,
                                  const int32_t* perm, float* out, void* ws, size_t ws_bytes, void* stream) {
  int rc;
  if (heads_args(rowptr, rows, nnz, heads, 0, ws, ws_bytes, edge_workspace_bytes(nnz, heads > 0 ? heads : 1), &rc)) return rc;
  if (!x || !out) return GCN_ERR_INVALID_ARG;
  return launch_segment_sum_heads(rowptr, rows, nnz, heads, x, perm, out, ws, (hipStream_t)stream) == hipSuccess ? GCN_OK
                                                                                                                  : GCN_ERR_HIP;
}

int gcn_spmm_heads_csr_f32(const int32_t* rowptr, const int32_t* idx, const int32_t* perm, int32_t rows, int32_t nnz, int32_t heads,
                           int32_t k, const float* vals, const float* x, float* out, void* ws, size_t ws_bytes, void* stream) {
  int rc;
  if (k < 1) return GCN_ERR_INVALID_ARG;
  if (heads_args(rowptr, rows, nnz, heads, k, ws, ws_bytes, heads_spmm_workspace_bytes(nnz, k), &rc)) return rc;
  if (!idx || !vals || !x || !out) return GCN_ERR_INVALID_ARG;
  return launch_spmm_heads(rowptr, idx, perm, rows, nnz, heads, k, vals, x, out, ws, (hipStream_t)stream) == hipSuccess
             ? GCN_OK : GCN_ERR_HIP;
}

int gcn_sddmm_heads_csr_f32(const int32_t* rowptr, const int32_t* col, int32_t m, int32_t nnz, int32_t heads, int32_t k,
                            const float* a, const float* b, float* out, void* ws, size_t ws_bytes, void* stream) {
  int rc;
  if (k < 1) return GCN_ERR_INVALID_ARG;
  if (heads_args(rowptr, m, nnz, heads, k, ws, ws_bytes, kHeadsSddmmWsBytes, &rc)) return rc;
  if (!col || !a || !b || !out) return GCN_ERR_INVALID_ARG;
  return launch_sddmm_heads(rowptr, col, m, nnz, heads, k, a, b, out, ws, (hipStream_t)stream) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
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
  return launch_gatv2_scores(rowptr, col, m, nnz, heads, k, h_dst, h_src, att, negative_slope, out, ws, (hipStream_t)stream) ==
                 hipSuccess ? GCN_OK : GCN_ERR_HIP;
}

int gcn_gatv2_scores_backward_csr_f32(const int32_t* rowptr, const int32_t* idx, const int32_t* perm, int32_t rows, int32_t nnz,
                                      int32_t heads, int32_t k, const float* own, const float* other, const float* att,
                                      float negative_slope, const float* g, float* grad_own, float* act_sums, void* ws,
                                      size_t ws_bytes, void* stream) {
  int rc;
  if (k < 1) return GCN_ERR_INVALID_ARG;
  if (heads_args(rowptr, rows, nnz, heads, k, ws, ws_bytes, gatv2_workspace_bytes(nnz, k), &rc)) return rc;
  if (!idx || !own || !other || !att || !g || !grad_own) return GCN_ERR_INVALID_ARG;
  return launch_gatv2_scores_backward(rowptr, idx, perm, rows, nnz, heads, k, own, other, att, negative_slope, g, grad_own, act_sums,
                                      ws, (hipStream_t)stream) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
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
    return hipMemsetAsync(arg, 0xff, elems * 4, st) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
  }
  if (!rowptr || !col || !x || !ws || ws_bytes < aggregate_workspace_bytes(nnz, k)) return GCN_ERR_INVALID_ARG;
  return launch_aggregate(rowptr, col, m, nnz, x, dtype == GCN_DTYPE_BF16, k, op == GCN_REDUCE_MAX ? kAggMax : kAggMin, out, arg, ws,
                          st) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
}

int gcn_aggregate_backward_csr(const int32_t* trowptr, const int32_t* trow, const int32_t* tperm, int32_t n, int32_t m, int32_t nnz,
                               const void* g, int32_t dtype, const int32_t* arg, int32_t k, void* gx, void* ws, size_t ws_bytes,
                               void* stream) {
  int rc;
  if (aggregate_args(n, m, nnz, dtype, k, &rc)) return rc;
  if (!gx) return GCN_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  if (nnz == 0)
    return hipMemsetAsync(gx, 0, (size_t)n * (size_t)k * (dtype == GCN_DTYPE_BF16 ? 2 : 4), st) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
  if (!trowptr || !trow || !tperm || !g || !arg || !ws || ws_bytes < aggregate_workspace_bytes(nnz, k)) return GCN_ERR_INVALID_ARG;
  return launch_aggregate_backward(trowptr, trow, tperm, n, nnz, g, dtype == GCN_DTYPE_BF16, arg, k, gx, ws, st) == hipSuccess
             ? GCN_OK : GCN_ERR_HIP;
}

int gcn_sample_neighbors_csr(const int32_t* rowptr, const int32_t* col, int32_t m, int32_t nnz, const int32_t* seeds, int32_t n_seeds,
                             int32_t fanout, uint64_t seed, uint64_t offset, const int32_t* out_rowptr, int32_t* out_col,
                             int32_t* out_eid, void* ws, size_t ws_bytes, void* stream) {
  if (m < 0 || nnz < 0 || n_seeds < 0 || fanout == 0) return GCN_ERR_INVALID_ARG;
  if (n_seeds == 0) return GCN_OK;
  if (!seeds || !out_rowptr) return GCN_ERR_INVALID_ARG;
  if (m == 0 || nnz == 0) return GCN_OK;                // (no seed is in range / every row is empty: nothing to write)
  if (!rowptr || !col || !out_col || !out_eid || !ws || ws_bytes < kSampleWsBytes) return GCN_ERR_INVALID_ARG;
  return launch_sample_neighbors(rowptr, col, m, nnz, seeds, n_seeds, fanout, seed, offset, out_rowptr, out_col, out_eid, ws,
                                 (hipStream_t)stream) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
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
  return launch_induced_subgraph_count(rowptr, col, m, nnz, nodes, n_nodes, vmap, out_len, ws, (hipStream_t)stream) == hipSuccess
             ? GCN_OK : GCN_ERR_HIP;
}

int gcn_induced_subgraph_fill_csr(const int32_t* rowptr, const int32_t* col, int32_t m, int32_t nnz, const int32_t* nodes,
                                  int32_t n_nodes, const int32_t* vmap, const int32_t* out_rowptr, int32_t* out_col,
                                  int32_t* out_eid, void* ws, size_t ws_bytes, void* stream) {
  int rc;
  if (subgraph_args(m, nnz, n_nodes, nodes, &rc)) return rc;
  if (!out_rowptr) return GCN_ERR_INVALID_ARG;
  if (m == 0 || nnz == 0) return GCN_OK;
  if (!rowptr || !col || !vmap || !out_col || !out_eid || !ws || ws_bytes < kSubgraphWsBytes) return GCN_ERR_INVALID_ARG;
  return launch_induced_subgraph_fill(rowptr, col, m, nnz, nodes, n_nodes, vmap, out_rowptr, out_col, out_eid, ws,
                                      (hipStream_t)stream) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
}

static_assert(kSubgraphWsBytes == GCN_SUBGRAPH_WS_BYTES, "include/gcn_spmm.h");

int gcn_random_walk_csr(const int32_t* rowptr, const int32_t* col, int32_t m, int32_t nnz, const int32_t* starts, int32_t n_walks,
                        int32_t length, uint64_t seed, uint64_t offset, int32_t* out_walks, void* stream) {
  if (m < 0 || nnz < 0 || n_walks < 0 || length < 0) return GCN_ERR_INVALID_ARG;
  if (n_walks == 0) return GCN_OK;
  if (!starts || !out_walks || (m > 0 && !rowptr) || (m > 0 && nnz > 0 && !col)) return GCN_ERR_INVALID_ARG;
  return launch_random_walk(rowptr, col, m, nnz, starts, n_walks, length, seed, offset, out_walks, (hipStream_t)stream) == hipSuccess
             ? GCN_OK : GCN_ERR_HIP;
}

int gcn_csr_find_entries(const int32_t* rowptr, const int32_t* col, int32_t m, int32_t nnz, const int32_t* q_rows,
                         const int32_t* q_cols, int32_t n_queries, int32_t* out_eid, void* stream) {
  if (m < 0 || nnz < 0 || n_queries < 0) return GCN_ERR_INVALID_ARG;
  if (n_queries == 0) return GCN_OK;
  if (!q_rows || !q_cols || !out_eid || (m > 0 && !rowptr) || (m > 0 && nnz > 0 && !col)) return GCN_ERR_INVALID_ARG;
  return launch_find_entries(rowptr, col, m, nnz, q_rows, q_cols, n_queries, out_eid, (hipStream_t)stream) == hipSuccess
             ? GCN_OK : GCN_ERR_HIP;
}

int gcn_negative_sample_csr(const int32_t* rowptr, const int32_t* col, int32_t m, int32_t n, int32_t nnz, const int32_t* q_rows,
                            int32_t n_queries, int32_t num_neg, int32_t max_tries, int32_t exclude_self, uint64_t seed,
                            uint64_t offset, int32_t* out_cols, void* stream) {
  if (m < 0 || n < 0 || nnz < 0 || n_queries < 0 || num_neg < 1 || max_tries < 1 || max_tries > 64) return GCN_ERR_INVALID_ARG;
  if ((long long)n_queries * num_neg >= (1ll << 31)) return GCN_ERR_INVALID_ARG;
  if (n_queries == 0) return GCN_OK;
  if (n < 1 || !q_rows || !out_cols || (m > 0 && !rowptr) || (m > 0 && nnz > 0 && !col)) return GCN_ERR_INVALID_ARG;
  return launch_negative_sample(rowptr, col, m, n, nnz, q_rows, n_queries * num_neg, num_neg, max_tries, exclude_self != 0, seed,
                                offset, out_cols, (hipStream_t)stream) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
}

static_assert(kBucketWaveMax == GCN_BUCKET_WAVE_MAX && kBucketBlockMax == GCN_BUCKET_BLOCK_MAX, "include/gcn_spmm.h");

int gcn_bucket_count_i32(const int32_t* keys, int32_t count, int32_t nbuckets, int32_t* offsets, void* stream) {
  if (count < 0 || nbuckets < 0 || !offsets || (count > 0 && nbuckets > 0 && !keys)) return GCN_ERR_INVALID_ARG;
  return launch_bucket_count(keys, count, nbuckets, offsets, (hipStream_t)stream) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
}

int gcn_bucket_fill_i32(const int32_t* keys, int32_t count, int32_t nbuckets, const int32_t* offsets, int32_t* perm, void* ws,
                        size_t ws_bytes, void* stream) {
  if (count < 0 || nbuckets < 0) return GCN_ERR_INVALID_ARG;
  if (count == 0 || nbuckets == 0) return GCN_OK;
  if (!keys || !offsets || !perm || !ws || ws_bytes < bucket_workspace_bytes(count, nbuckets)) return GCN_ERR_INVALID_ARG;
  return launch_bucket_fill(keys, count, nbuckets, offsets, perm, ws, (hipStream_t)stream) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
}

int gcn_csr_transpose_gather(const int32_t* rowptr, int32_t m, int32_t nnz, const int32_t* perm, const float* val, int32_t* trow,
                             float* tval, void* stream) {
  if (m < 0 || nnz < 0 || (val == nullptr) != (tval == nullptr)) return GCN_ERR_INVALID_ARG;
  if (nnz == 0) return GCN_OK;
  if (m == 0 || !rowptr || !perm || !trow) return GCN_ERR_INVALID_ARG;
  return launch_transpose_gather(rowptr, m, nnz, perm, val, trow, tval, (hipStream_t)stream) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
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
  return launch_csr_coalesce_count(rowptr, col, m, n, nnz, diagonal, out_len, ws, (hipStream_t)stream) == hipSuccess
             ? GCN_OK : GCN_ERR_HIP;
}

int gcn_csr_coalesce_fill(const int32_t* rowptr, const int32_t* col, const float* val, int32_t m, int32_t n, int32_t nnz,
                          int32_t reduce, int32_t diagonal, float diag_value, const int32_t* out_rowptr, int32_t* out_col,
                          float* out_val, int32_t* out_first, int32_t* seg, void* ws, size_t ws_bytes, void* stream) {
  if (m < 0 || n < 0 || nnz < 0 || reduce < GCN_COALESCE_SUM || reduce > GCN_COALESCE_FIRST || diagonal < GCN_DIAG_KEEP ||
      diagonal > GCN_DIAG_ADD || (val == nullptr) != (out_val == nullptr))
    return GCN_ERR_INVALID_ARG;
  if (m == 0) return GCN_OK;
  if (!rowptr || (nnz > 0 && !col) || !out_rowptr || !out_col || !ws || ws_bytes < kCoalesceWsBytes) return GCN_ERR_INVALID_ARG;
  return launch_csr_coalesce_fill(rowptr, col, val, m, n, nnz, reduce, diagonal, diag_value, out_rowptr, out_col, out_val,
                                  out_first, seg, ws, (hipStream_t)stream) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
}

int gcn_csr_degree_f64(const int32_t* rowptr, const float* val, int32_t m, int32_t nnz, double* deg, void* stream) {
  if (m < 0 || nnz < 0) return GCN_ERR_INVALID_ARG;
  if (m == 0) return GCN_OK;
  if (!rowptr || !deg) return GCN_ERR_INVALID_ARG;
  return launch_csr_degree(rowptr, val, m, nnz, deg, (hipStream_t)stream) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
}

int gcn_csr_normalize_f32(const int32_t* rowptr, const int32_t* col, const float* val, int32_t m, int32_t n, int32_t nnz,
                          const double* deg, int32_t mode, float* out_val, void* stream) {
  if (m < 0 || n < 0 || nnz < 0 || (mode != GCN_NORM_SYM && mode != GCN_NORM_ROW) || (mode == GCN_NORM_SYM && m != n))
    return GCN_ERR_INVALID_ARG;
  if (m == 0 || nnz == 0) return GCN_OK;
  if (!rowptr || !col || !deg || !out_val) return GCN_ERR_INVALID_ARG;
  return launch_csr_normalize(rowptr, col, val, m, n, nnz, deg, mode, out_val, (hipStream_t)stream) == hipSuccess ? GCN_OK
                                                                                                                  : GCN_ERR_HIP;
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
    return hipMemsetAsync(out_len, 0, (size_t)m * 4, (hipStream_t)stream) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
  if (!a_rowptr || !a_col || !b_rowptr || !b_col || !ws || ws_bytes < spgemm_workspace_bytes(m, n)) return GCN_ERR_INVALID_ARG;
  return launch_spgemm_count(a_rowptr, a_col, m, p, nnz_a, b_rowptr, b_col, n, nnz_b, out_len, ws, (hipStream_t)stream) == hipSuccess
             ? GCN_OK : GCN_ERR_HIP;
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
  return launch_spgemm_fill(a_rowptr, a_col, a_val, m, p, nnz_a, b_rowptr, b_col, b_val, n, nnz_b, out_rowptr, out_col, out_val,
                            ws, (hipStream_t)stream) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
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
  return launch_csr_sampled_dot(p_rowptr, p_col, mp, np, nnz_p, x_rowptr, x_col, x_val, nnz_x, y_rowptr, y_col, y_val, nnz_y, w,
                                x_by_col, out, ws, (hipStream_t)stream) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
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
  return launch_knn(x, ldx, y, ldy, q, n, d, k, self_offset, eff, out_idx, out_dist2, out_sum, ws, (hipStream_t)stream) == hipSuccess
             ? GCN_OK : GCN_ERR_HIP;
}

int gcn_spmm_plan_sddmm_kernel(const gcn_spmm_plan_t* p, int32_t k, char* buf, int32_t buflen) {
  if (!p || k <= 0 || !buf || buflen <= 0) return GCN_ERR_INVALID_ARG;
  snprintf(buf, (size_t)buflen, "gcn::sddmm_kernel<%s, %s>", sddmm_sliced(p, k) ? "true" : "false",
           k % 4 == 0 ? "true" : "false");
  return GCN_OK;
}

int gcn_spmm_csr_f32_epilogue(gcn_spmm_plan_t* p, const int32_t* rowptr, const int32_t* col, const float* val,
                              const float* B, float* C, const float* bias, int32_t relu, float dropout_p,
                              uint64_t seed, uint64_t offset, int32_t k, void* stream) {
  if (!p || k < 0 || !(dropout_p >= 0.f && dropout_p < 1.f)) return GCN_ERR_INVALID_ARG;
  if (p->m == 0 || k == 0) return GCN_OK;
  if (!C || !rowptr || (p->nnz > 0 && (!col || !val || !B))) return GCN_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const SpmmRoute r = spmm_route(p, k, /*build=*/true, rowptr, col, val, st);
  Epilogue epi;
  epi.bias = bias; epi.relu = relu ? 1 : 0;
  epi.drop.p = dropout_p; epi.drop.seed = seed; epi.drop.offset = offset;
  int rc;
  const float* Bg = B;
  if (r.copy != BCopy::none) {
    if ((rc = relay_B(p, r, B, k, st)) != GCN_OK) return rc;
    Bg = p->bpad;
  }
  if (r.odd) {                                         // into a k_run-wide scratch result, compacted with bias / ReLU into C
    if (grow(p->cpad, (size_t)p->m * (size_t)r.k_run) != GCN_OK) return GCN_ERR_ALLOC;
    if ((rc = spmm_impl(p, r, rowptr, col, val, B, Bg, p->cpad, Epilogue{}, st)) != GCN_OK) return rc;
    if (launch_unpad_rows(C, p->cpad, bias, epi.relu, p->m, k, r.k_run, st) != hipSuccess) return GCN_ERR_HIP;
  } else if ((rc = spmm_impl(p, r, rowptr, col, val, B, Bg, C, epi, st)) != GCN_OK) return rc;
  if (epi.drop.on() && !r.reduce_epilogue)             // no epilogue pass carried the mask: one pass in place
    return launch_dropout(C, C, (long long)p->m * k, epi.drop, st) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
  return GCN_OK;
}

// Everything a k-wide call builds lazily, built NOW (the narrow slice set of k <= 32: device allocations and stream
// synchronisation that a stream capture would refuse): afterwards the first k-wide call only grows workspaces.
int gcn_spmm_plan_prepare_width(gcn_spmm_plan_t* p, const int32_t* rowptr, const int32_t* col, const float* val, int32_t k,
                                void* stream) {
  if (!p || k <= 0) return GCN_ERR_INVALID_ARG;
  if (p->nnz > 0 && (!rowptr || !col || !val)) return GCN_ERR_INVALID_ARG;
  (void)spmm_route(p, k, /*build=*/true, rowptr, col, val, (hipStream_t)stream);
  if (sddmm_sliced(p, k)) return ensure_value_map(p, rowptr, (hipStream_t)stream);   // (the output map of a k-wide SDDMM)
  return GCN_OK;
}

int gcn_spmm_csr_f32_bias_relu(gcn_spmm_plan_t* p, const int32_t* rowptr, const int32_t* col,
                               const float* val, const float* B, float* C, const float* bias,
                               int32_t relu, int32_t k, void* stream) {
  return gcn_spmm_csr_f32_epilogue(p, rowptr, col, val, B, C, bias, relu, 0.f, 0, 0, k, stream);
}

int gcn_spmm_csr_f32(gcn_spmm_plan_t* p, const int32_t* rowptr, const int32_t* col,
                     const float* val, const float* B, float* C, int32_t k, void* stream) {
  return gcn_spmm_csr_f32_epilogue(p, rowptr, col, val, B, C, nullptr, 0, 0.f, 0, 0, k, stream);
}

int gcn_spmm_csr_f32_prelaid(gcn_spmm_plan_t* p, const int32_t* rowptr, const int32_t* col, const float* val,
                             const float* Bp, float* out, const float* out_scale, int32_t out_gap, int32_t k,
                             void* stream) {
  if (!p || k <= 0 || out_gap < 0) return GCN_ERR_INVALID_ARG;
  if (p->m == 0) return GCN_OK;
  if (!Bp || !out || !rowptr || !col || !val) return GCN_ERR_INVALID_ARG;
  SpmmRoute r;
  if (const int rc = spmm_route_prelaid(p, k, &r); rc != GCN_OK) return rc;
  if ((((uintptr_t)Bp | (uintptr_t)out) & 15) != 0) return GCN_ERR_INVALID_ARG;
  Epilogue epi;
  epi.outscale = out_scale;
  epi.gap_w = out_gap;
  return spmm_impl(p, r, rowptr, col, val, Bp, Bp, out, epi, (hipStream_t)stream);
}

int gcn_dropout_f32(float* dst, const float* src, int64_t count, float dropout_p, uint64_t seed, uint64_t offset,
                    void* stream) {
  if (count < 0 || !(dropout_p >= 0.f && dropout_p < 1.f)) return GCN_ERR_INVALID_ARG;
  if (count == 0) return GCN_OK;
  if (!dst || !src) return GCN_ERR_INVALID_ARG;
  DropoutSpec d;
  d.p = dropout_p; d.seed = seed; d.offset = offset;
  if (!d.on()) {
    if (dst == src) return GCN_OK;
    return hipMemcpyAsync(dst, src, sizeof(float) * (size_t)count, hipMemcpyDeviceToDevice, (hipStream_t)stream) == hipSuccess
               ? GCN_OK : GCN_ERR_HIP;
  }
  return launch_dropout(dst, src, (long long)count, d, (hipStream_t)stream) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
}

// bf16 operands: B is bf16, C fp32 or bf16 (c_dtype), every sum fp32.  The hot path (bf16_route, plan_policy.cpp) re-lays B
// as a bf16 table in the group kernels' slice layout, walks it with the bf16 group kernel into the fp32 partial rows and
// reduces them with the whole epilogue, rounding once when C is bf16.  Every other plan and width takes the fallback: B
// widened to fp32, the fp32 entry above with its whole epilogue (into C itself when C is fp32), the result narrowed.
// Correct everywhere, fast only on the hot path.
int gcn_spmm_csr_bf16_epilogue(gcn_spmm_plan_t* p, const int32_t* rowptr, const int32_t* col, const float* val,
                               const void* B, void* C, int32_t c_dtype, const float* bias, int32_t relu,
                               float dropout_p, uint64_t seed, uint64_t offset, int32_t k, void* stream) {
  if (!p || k < 0 || !(dropout_p >= 0.f && dropout_p < 1.f)) return GCN_ERR_INVALID_ARG;
  if (c_dtype != GCN_DTYPE_F32 && c_dtype != GCN_DTYPE_BF16) return GCN_ERR_INVALID_ARG;
  if (p->m == 0 || k == 0) return GCN_OK;
  if (!C || !rowptr || (p->nnz > 0 && (!col || !val || !B))) return GCN_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const unsigned short* Bh = static_cast<const unsigned short*>(B);
  const Bf16Route rt = bf16_route(p, k, /*build=*/true, rowptr, col, val, st);
  if (!rt.group) {
    float* Cf = static_cast<float*>(C);
    if (c_dtype == GCN_DTYPE_BF16) {
      if (grow(p->cwide, (size_t)p->m * (size_t)k) != GCN_OK) return GCN_ERR_ALLOC;
      Cf = p->cwide;
    }
    const float* Bf = nullptr;
    if (p->nnz > 0) {
      if (grow(p->bwide, (size_t)p->n * (size_t)k) != GCN_OK) return GCN_ERR_ALLOC;
      if (launch_bf16_to_f32(p->bwide, Bh, (long long)p->n * k, st) != hipSuccess) return GCN_ERR_HIP;
      Bf = p->bwide;
    }
    const int rc = gcn_spmm_csr_f32_epilogue(p, rowptr, col, val, Bf, Cf, bias, relu, dropout_p, seed, offset, k, stream);
    if (rc != GCN_OK || c_dtype == GCN_DTYPE_F32) return rc;
    return launch_f32_to_bf16(static_cast<unsigned short*>(C), Cf, (long long)p->m * k, st) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
  }
  // hot path: the bf16 table reuses the bytes of the plan's fp32 copy of B
  const SliceSet& ss = rt.ss;
  const GroupStream& G = *ss.g;
  const size_t table_elems = (size_t)ss.table_rows() * (size_t)rt.ldh;      // bf16 entries
  if (grow(p->bpad, (table_elems + 1) / 2) != GCN_OK) return GCN_ERR_ALLOC;
  unsigned short* table = reinterpret_cast<unsigned short*>(p->bpad.get());
  if (launch_relay_bf16_sliced(table, Bh, rt.weighted ? nullptr : p->factors.u_col, p->n, k, rt.ldh, ss.S, G.w, st) != hipSuccess)
    return GCN_ERR_HIP;
  if (grow(p->ws, ws_elems(p, k)) != GCN_OK) return GCN_ERR_ALLOC;
  if (grow(p->cv, (size_t)ss.S * (size_t)p->m * (size_t)k) != GCN_OK) return GCN_ERR_ALLOC;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;             // live timing of the main kernel (gcn_spmm_profile_begin)
  if (p->prof.armed()) { const auto pr = p->prof.next(); ev0 = pr.first; ev1 = pr.second; }
  CutLists cuts;
  if (const int rc = run_group_walk(p, ss, rt.weighted, table, 2, rt.ldh, k, ev0, ev1, st, &cuts); rc != GCN_OK) return rc;
  DropoutSpec drop;
  drop.p = dropout_p; drop.seed = seed; drop.offset = offset;
  const float* rowscale = rt.weighted ? nullptr : p->factors.u_row.get();
  const hipError_t e = c_dtype == GCN_DTYPE_F32
      ? launch_slice_reduce(p->cv, static_cast<float*>(C), bias, relu ? 1 : 0, p->m, ss.S, k, st, 0, rowscale, drop, nullptr,
                            nullptr, 0, cuts)
      : launch_slice_reduce_bf16(p->cv, static_cast<unsigned short*>(C), bias, relu ? 1 : 0, p->m, ss.S, k, rowscale, drop, cuts, st);
  return e == hipSuccess ? GCN_OK : GCN_ERR_HIP;
}

int gcn_spmm_csr_bf16(gcn_spmm_plan_t* p, const int32_t* rowptr, const int32_t* col, const float* val, const void* B, void* C,
                      int32_t c_dtype, int32_t k, void* stream) {
  return gcn_spmm_csr_bf16_epilogue(p, rowptr, col, val, B, C, c_dtype, nullptr, 0, 0.f, 0, 0, k, stream);
}

int gcn_dropout_bf16(void* dst, const void* src, int64_t count, float dropout_p, uint64_t seed, uint64_t offset, void* stream) {
  if (count < 0 || !(dropout_p >= 0.f && dropout_p < 1.f)) return GCN_ERR_INVALID_ARG;
  if (count == 0) return GCN_OK;
  if (!dst || !src) return GCN_ERR_INVALID_ARG;
  DropoutSpec d;
  d.p = dropout_p; d.seed = seed; d.offset = offset;
  if (!d.on()) {
    if (dst == src) return GCN_OK;
    return hipMemcpyAsync(dst, src, 2 * (size_t)count, hipMemcpyDeviceToDevice, (hipStream_t)stream) == hipSuccess
               ? GCN_OK : GCN_ERR_HIP;
  }
  return launch_dropout_bf16(static_cast<unsigned short*>(dst), static_cast<const unsigned short*>(src), (long long)count, d,
                             (hipStream_t)stream) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
}

int gcn_spmm_profile_begin(gcn_spmm_plan_t* p, int32_t capacity) {
  if (!p || capacity <= 0 || p->prof.capacity() > 0) return GCN_ERR_INVALID_ARG;
  return p->prof.begin(capacity) == hipSuccess ? GCN_OK : GCN_ERR_HIP;   // (a failed create leaves no events behind)
}

int gcn_spmm_profile_end(gcn_spmm_plan_t* p, float* ms_out, int32_t* count_out) {
  if (!p || !count_out || p->prof.capacity() <= 0) return GCN_ERR_INVALID_ARG;
  int rc = GCN_OK;
  for (int i = 0; i < p->prof.recorded(); ++i) {
    float ms = 0.f;
    if (hipEventSynchronize(p->prof.stop(i)) != hipSuccess ||
        hipEventElapsedTime(&ms, p->prof.start(i), p->prof.stop(i)) != hipSuccess) rc = GCN_ERR_HIP;
    if (ms_out) ms_out[i] = ms;
  }
  *count_out = p->prof.recorded();
  p->prof.clear();
  return rc;
}

// One-shot: the schedule is recomputed on the device every call (a few µs: one binary search per
// chunk) into the scratch plan of this (device, stream), so there is no cache that could go stale when
// the caller reuses device addresses, and calls on different streams or devices never share buffers.
int gcn_spmm_csr_f32_oneshot(const int32_t* rowptr, const int32_t* col, const float* val,
                             const float* B, float* C, int32_t m, int32_t n, int32_t nnz,
                             int32_t k, void* stream) {
  if (m < 0 || n < 0 || nnz < 0 || k < 0) return GCN_ERR_INVALID_ARG;
  const int cu = cu_count_cached();
  if (cu <= 0) return GCN_ERR_NO_DEVICE;
  std::lock_guard<std::mutex> lk(g_plan_mu);
  gcn_spmm_plan* p = scratch_plan(stream);
  if (!p) return GCN_ERR_ALLOC;
  p->m = m; p->n = n; p->nnz = nnz; p->cu_count = cu;
  p->T = auto_chunk_nnz(nnz, cu);
  p->nchunks = (int)(((long long)nnz + p->T - 1) / p->T);
  if (p->chunk_row.grow((size_t)p->nchunks) != hipSuccess) return GCN_ERR_ALLOC;
  if (m == 0 || k == 0) return GCN_OK;
  if (launch_plan_chunk_rows(rowptr, m, p->T, p->nchunks, p->chunk_row, (hipStream_t)stream) != hipSuccess) return GCN_ERR_HIP;
  if (p->ws.grow(ws_elems(p, k)) != hipSuccess) return GCN_ERR_ALLOC;
  SpmmArgs a;
  a.rowptr = rowptr; a.col = col; a.val = val; a.B = B; a.C = C; a.P = p->ws;
  a.chunk_row = p->chunk_row; a.bias = nullptr; a.relu = 0;
  a.nchunks = p->nchunks; a.T = p->T; a.m = m; a.nnz = nnz; a.k = k; a.n = n;
  a.nnz_dev = nullptr; a.nchunks_grid = p->nchunks;
  a.tile_cols = auto_tile_cols(n, k);
  return launch_spmm(a, cu, (hipStream_t)stream) == hipSuccess ? GCN_OK : GCN_ERR_HIP;
}

int gcn_gather_rows_f32(float* dst, const float* src, const int32_t* idx, int32_t nrows, int32_t k,
                        void* stream) {
  if (nrows < 0 || k < 0) return GCN_ERR_INVALID_ARG;
  if (nrows == 0 || k == 0) return GCN_OK;
  if (!dst || !src || !idx || dst == src) return GCN_ERR_INVALID_ARG;
  return launch_gather_rows(dst, src, idx, nrows, k, (hipStream_t)stream) == hipSuccess
             ? GCN_OK : GCN_ERR_HIP;
}

}  // extern "C"
