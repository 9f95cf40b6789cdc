// api_spmm.cpp — the native C ABI of libgcnspmm.so: the entry points that read a plan or the fused epilogue — SpMM, SDDMM,
// dropout, live kernel timing (include/gcn_spmm.h has the contract and the reference interfaces each one replaces).  The plan
// is built in plan_build.cpp, the rules that pick kernel family, tile, stride and slice set are plan_policy.cpp; the plan-free
// units' entry points are api_units.cpp, the reorderers' api_reorder.cpp, the reference's own symbols api_dropin.cpp.
#include "plan_policy.h"

#include <cstdio>

#define GCN_VERSION_STR "0.4.0"

using namespace gcn;
static_assert(kDtypeF32 == GCN_DTYPE_F32 && kDtypeBf16 == GCN_DTYPE_BF16, "include/gcn_spmm.h");

namespace {

// The copy of B a call's route asks for (r.copy), rows r.ldb elements apart (>= k, padding columns zero), scaled by u_col
// on a value-free route: row-padded, with one all-zero row more than B has (16-bit stream), or in the group kernels' layout,
// slice s at rows [s*(w+1), (s+1)*(w+1)) with row w of every slice zero (the weighted pass: the same, rows not scaled) —
// of fp32, or the bf16 table of a bf16 call (B is bf16 then), which reuses the bytes of the plan's fp32 copy.
int relay_B(gcn_spmm_plan* p, const SpmmRoute& r, const void* B, int k, hipStream_t st) {
  if (r.copy == BCopy::none) return GCN_OK;            // (the caller's own rows are gathered)
  const float* scale = r.valless ? p->factors.u_col : nullptr;
  const size_t table_elems = (size_t)r.ss.table_rows() * (size_t)r.ldb;        // (of a group layout)
  if (r.copy == BCopy::group_layout_bf16) {
    if (const int rc = grow(p->bpad, (table_elems + 1) / 2); rc != GCN_OK) return rc;
    unsigned short* table = reinterpret_cast<unsigned short*>(p->bpad.get());
    return hip_status(launch_relay_bf16_sliced(table, static_cast<const unsigned short*>(B), scale, p->n, k, r.ldb, r.ss.S,
                                               r.ss.g->w, st));
  }
  const float* Bf = static_cast<const float*>(B);
  if (r.copy == BCopy::group_layout) {
    if (const int rc = grow(p->bpad, table_elems); rc != GCN_OK) return rc;
    return hip_status(launch_scale_rows_sliced(p->bpad, Bf, scale, p->n, k, r.ldb, r.ss.S, r.ss.g->w, st));
  }
  if (const int rc = grow(p->bpad, ((size_t)p->n + 1) * (size_t)r.ldb); rc != GCN_OK) return rc;
  if (launch_pad_rows(p->bpad, Bf, p->n, k, r.ldb, st, scale) != hipSuccess ||
      hipMemsetAsync(p->bpad + (size_t)p->n * r.ldb, 0, sizeof(float) * (size_t)r.ldb, st) != hipSuccess)
    return GCN_ERR_HIP;
  return GCN_OK;
}

struct Epilogue {                                      // C = dropout(act(A*B + bias))
  const float* bias = nullptr;
  int relu = 0;
  DropoutSpec drop;
  int c_dtype = GCN_DTYPE_F32;                         // bf16: the group family's reduction only (the bf16 hot path)
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

// One call along its route r (spmm_route / spmm_route_bf16) into Cout [m x r.k_run] of epi.c_dtype.  B: the caller's fp32
// features (the panel kernels alone read them); Bg: what the main kernels gather from, rows r.ldb elements of r.elem_bytes apart:
// B or the route's copy.  Where r.reduce_epilogue is set the slice reduction carries the whole epilogue, the mask included.
int spmm_impl(gcn_spmm_plan* p, const SpmmRoute& r, const int32_t* rowptr, const int32_t* col, const float* val, const float* B,
              const void* Bg, void* Cout, const Epilogue& epi, hipStream_t st) {
  const int k = r.k_run;
  if (grow(p->ws, ws_elems(p, k)) != GCN_OK) return GCN_ERR_ALLOC;
  if (r.S_run > 0 && grow(p->cv, (size_t)r.S_run * (size_t)p->m * (size_t)k) != GCN_OK) return GCN_ERR_ALLOC;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;             // live timing of the main kernel (gcn_spmm_profile_begin)
  if (p->prof.armed()) { const auto pr = p->prof.next(); ev0 = pr.first; ev1 = pr.second; }
  SliceReduce red;                                     // what both sliced families end with
  red.Cv = p->cv; red.C = Cout; red.c_dtype = epi.c_dtype; red.m = p->m; red.S = r.S_run; red.k = k;
  red.bias = epi.bias; red.relu = epi.relu; red.drop = epi.drop;
  if (r.family == SpmmFamily::group) {
    // four independent 16-lane row engines per wave on the 15-bit slice-major stream (spmm_group.hip), then the per-row
    // reduction over slices
    if (const int rc = run_group_walk(p, r.ss, r.weighted, Bg, r.elem_bytes, r.ldb, k, ev0, ev1, st, &red.cuts); rc != GCN_OK)
      return rc;
    red.rowscale = r.weighted ? nullptr : p->factors.u_row.get();
    red.outscale = epi.outscale; red.gap_w = epi.gap_w;
    return hip_status(launch_slice_reduce(red, st));
  }
  if (epi.c_dtype != GCN_DTYPE_F32) return GCN_ERR_INVALID_ARG;   // (no route but the group one writes bf16)
  float* const C = static_cast<float*>(Cout);
  SpmmArgs a = spmm_args(p, r, epi.relu != 0);
  a.B = static_cast<const float*>(Bg); a.P = p->ws; a.ev_start = ev0; a.ev_stop = ev1;
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
    return hip_status(launch_spmm(a, p->cu_count, st));
  }
  if (r.family == SpmmFamily::unsliced) {
    a.rowptr = rowptr; a.col = col; a.val = val; a.chunk_row = p->chunk_row;
    a.C = C; a.bias = epi.bias;
    return hip_status(launch_spmm(a, p->cu_count, st));
  }
  // sliced, four per gather: the slice-major virtual CSR (S*m rows) into the partial buffer, then the per-row reduction
  // over slices, which carries the whole epilogue (bias, ReLU, dropout mask, row factor)
  const Slicing& sl = p->slicing;
  const Col16Stream& c16 = p->col16;
  a.rowptr = sl.vrowptr; a.col = sl.vcol; a.val = r.valless ? nullptr : sl.vval.get(); a.chunk_row = sl.vchunk_row;
  if (r.col16) { a.rowptr = c16.vrowptr16; a.col = reinterpret_cast<const int*>(c16.vcol16.get()); a.chunk_row = c16.vchunk_row16; }
  a.C = p->cv;
  if (launch_spmm(a, p->cu_count, st) != hipSuccess) return GCN_ERR_HIP;
  red.rowscale = r.valless ? p->factors.u_row.get() : nullptr;
  return hip_status(launch_slice_reduce(red, st));
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
    return hip_status(hipMemsetAsync(out_val, 0, sizeof(float) * (size_t)p->nnz, st));
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
  return hip_status(launch_sddmm(s, st));
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
  if (!p || k < 0 || !dropout_p_ok(dropout_p)) return GCN_ERR_INVALID_ARG;
  if (p->m == 0 || k == 0) return GCN_OK;
  if (!C || !rowptr || (p->nnz > 0 && (!col || !val || !B))) return GCN_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  const SpmmRoute r = spmm_route(p, k, /*build=*/true, rowptr, col, val, st);
  Epilogue epi;
  epi.bias = bias; epi.relu = relu ? 1 : 0;
  epi.drop = dropout_spec(dropout_p, seed, offset);
  int rc;
  if ((rc = relay_B(p, r, B, k, st)) != GCN_OK) return rc;
  const float* Bg = r.copy == BCopy::none ? B : p->bpad.get();
  if (r.odd) {                                         // into a k_run-wide scratch result, compacted with bias / ReLU into C
    if (grow(p->cpad, (size_t)p->m * (size_t)r.k_run) != GCN_OK) return GCN_ERR_ALLOC;
    if ((rc = spmm_impl(p, r, rowptr, col, val, B, Bg, p->cpad, Epilogue{}, st)) != GCN_OK) return rc;
    if (launch_unpad_rows(C, p->cpad, bias, epi.relu, p->m, k, r.k_run, st) != hipSuccess) return GCN_ERR_HIP;
  } else if ((rc = spmm_impl(p, r, rowptr, col, val, B, Bg, C, epi, st)) != GCN_OK) return rc;
  if (epi.drop.on() && !r.reduce_epilogue)             // no epilogue pass carried the mask: one pass in place
    return hip_status(launch_dropout(C, C, (long long)p->m * k, epi.drop, st));
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
  if (count < 0 || !dropout_p_ok(dropout_p)) return GCN_ERR_INVALID_ARG;
  if (count == 0) return GCN_OK;
  if (!dst || !src) return GCN_ERR_INVALID_ARG;
  const DropoutSpec d = dropout_spec(dropout_p, seed, offset);
  if (!d.on()) {
    if (dst == src) return GCN_OK;
    return hip_status(hipMemcpyAsync(dst, src, sizeof(float) * (size_t)count, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  }
  return hip_status(launch_dropout(dst, src, (long long)count, d, (hipStream_t)stream));
}

// bf16 operands: B is bf16, C fp32 or bf16 (c_dtype), every sum fp32.  The hot path is a route of its own through the code
// above (spmm_route_bf16, plan_policy.cpp): relay_B re-lays B as a bf16 table in the group kernels' slice layout, spmm_impl
// walks it with the bf16 group kernel into the fp32 partial rows and reduces them with the whole epilogue, rounding once when
// C is bf16.  Every other plan and width takes the fallback: B widened to fp32, the fp32 entry above with its whole epilogue
// (into C itself when C is fp32), the result narrowed.  Correct everywhere, fast only on the hot path.
int gcn_spmm_csr_bf16_epilogue(gcn_spmm_plan_t* p, const int32_t* rowptr, const int32_t* col, const float* val,
                               const void* B, void* C, int32_t c_dtype, const float* bias, int32_t relu,
                               float dropout_p, uint64_t seed, uint64_t offset, int32_t k, void* stream) {
  if (!p || k < 0 || !dropout_p_ok(dropout_p)) return GCN_ERR_INVALID_ARG;
  if (c_dtype != GCN_DTYPE_F32 && c_dtype != GCN_DTYPE_BF16) return GCN_ERR_INVALID_ARG;
  if (p->m == 0 || k == 0) return GCN_OK;
  if (!C || !rowptr || (p->nnz > 0 && (!col || !val || !B))) return GCN_ERR_INVALID_ARG;
  hipStream_t st = (hipStream_t)stream;
  SpmmRoute r;
  if (!spmm_route_bf16(p, k, /*build=*/true, rowptr, col, val, st, &r)) {
    float* Cf = static_cast<float*>(C);
    if (c_dtype == GCN_DTYPE_BF16) {
      if (grow(p->cwide, (size_t)p->m * (size_t)k) != GCN_OK) return GCN_ERR_ALLOC;
      Cf = p->cwide;
    }
    const float* Bf = nullptr;
    if (p->nnz > 0) {
      if (grow(p->bwide, (size_t)p->n * (size_t)k) != GCN_OK) return GCN_ERR_ALLOC;
      if (launch_bf16_to_f32(p->bwide, static_cast<const unsigned short*>(B), (long long)p->n * k, st) != hipSuccess)
        return GCN_ERR_HIP;
      Bf = p->bwide;
    }
    const int rc = gcn_spmm_csr_f32_epilogue(p, rowptr, col, val, Bf, Cf, bias, relu, dropout_p, seed, offset, k, stream);
    if (rc != GCN_OK || c_dtype == GCN_DTYPE_F32) return rc;
    return hip_status(launch_f32_to_bf16(static_cast<unsigned short*>(C), Cf, (long long)p->m * k, st));
  }
  if (const int rc = relay_B(p, r, B, k, st); rc != GCN_OK) return rc;
  Epilogue epi;
  epi.bias = bias; epi.relu = relu ? 1 : 0; epi.c_dtype = c_dtype;
  epi.drop = dropout_spec(dropout_p, seed, offset);
  return spmm_impl(p, r, rowptr, col, val, nullptr, p->bpad.get(), C, epi, st);
}

int gcn_spmm_csr_bf16(gcn_spmm_plan_t* p, const int32_t* rowptr, const int32_t* col, const float* val, const void* B, void* C,
                      int32_t c_dtype, int32_t k, void* stream) {
  return gcn_spmm_csr_bf16_epilogue(p, rowptr, col, val, B, C, c_dtype, nullptr, 0, 0.f, 0, 0, k, stream);
}

int gcn_dropout_bf16(void* dst, const void* src, int64_t count, float dropout_p, uint64_t seed, uint64_t offset, void* stream) {
  if (count < 0 || !dropout_p_ok(dropout_p)) return GCN_ERR_INVALID_ARG;
  if (count == 0) return GCN_OK;
  if (!dst || !src) return GCN_ERR_INVALID_ARG;
  const DropoutSpec d = dropout_spec(dropout_p, seed, offset);
  if (!d.on()) {
    if (dst == src) return GCN_OK;
    return hip_status(hipMemcpyAsync(dst, src, 2 * (size_t)count, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  }
  return hip_status(launch_dropout_bf16(static_cast<unsigned short*>(dst), static_cast<const unsigned short*>(src),
                                        (long long)count, d, (hipStream_t)stream));
}

int gcn_spmm_profile_begin(gcn_spmm_plan_t* p, int32_t capacity) {
  if (!p || capacity <= 0 || p->prof.capacity() > 0) return GCN_ERR_INVALID_ARG;
  return hip_status(p->prof.begin(capacity));          // (a failed create leaves no events behind)
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
  return hip_status(launch_spmm(a, cu, (hipStream_t)stream));
}

}  // extern "C"
