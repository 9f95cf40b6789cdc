// plan_policy.h — what the translation units behind the native API share (internal):
//   plan_policy.cpp  the dispatch policy: which kernel family, tile, slice count and slice set a k-wide call takes
//   plan_build.cpp   plan construction: chunk table, column slicing, streams, value factors, panels
//   api_spmm.cpp     the C entry points of the SpMM, the SDDMM and dropout: the ones that read a plan or the epilogue
//   api_units.cpp    the C entry points of the plan-free units: argument checks in front of one launcher each
// The public contract is include/gcn_spmm.h.
#pragma once
#include "plan.h"

namespace gcn {

inline int hip_status(hipError_t e) { return e == hipSuccess ? GCN_OK : GCN_ERR_HIP; }   // a launcher's error as a status
// the dropout arguments of the four entry points that take them: the range each checks first (a NaN fails it), the kernels' spec
inline bool dropout_p_ok(float p) { return p >= 0.f && p < 1.f; }
inline DropoutSpec dropout_spec(float p, uint64_t seed, uint64_t offset) { return DropoutSpec{p, seed, offset}; }

// thresholds of the policy (measured; the experiments behind them are cited where they are used)
constexpr int kSliceMinK = 33;          // smallest k the sliced copy is used for on the four-per-gather kernel
constexpr int kGroupMinK = 12;          // ... when the group kernels walk it
constexpr int kVallessMinPerCol = 48;   // non-zeros per column from which the scaled copy of B (value-free pass) pays
constexpr double kPanelMfmaDensity = 0.25;   // window density from which a panel becomes a dense MFMA tile

// The slice set ONE call runs on — the plan's own, or the narrow set built for k <= 32 (plan.h: group_alt) — decided once
// per call and handed down as an argument (it used to be per-call state inside the plan: two streams sharing a plan at
// different widths raced on it).
struct SliceSet {
  const GroupStream* g = nullptr;
  int S = 0;
  int alt = -1;                         // width class of group_alt, -1: the plan's own set
  long long table_rows() const { return (long long)S * ((long long)(g ? g->w : 0) + 1); }
};
int alt_class(int k);                   // width class of the narrow slice sets (0: k <= 32), -1: none
// the shape of one call's group launch on ss (no table, no result buffers): what the launch and the report both decide from
GroupArgs group_shape(const SliceSet& ss, bool weighted, int elem_bytes, int ld, int k);

// development switches that select an alternate code path a TEST needs (read once per process)
bool group_fused_fixup();               // GCN_AMD_GROUP_FUSED_FIXUP=0: cut rows' pieces added by a pass of their own

int group_chunk(long long entries, int cu);
size_t ws_elems(const gcn_spmm_plan* p, int k);

bool value_free_plan(const gcn_spmm_plan* p);
bool group_plan(const gcn_spmm_plan* p);

// Widths that are not a multiple of 4 are computed at k4 = ceil(k / 4) * 4 on copies whose rows are ld floats apart (whole
// 128-byte lines); fits: that copy of an n-row table stays within the 768 MiB the re-laid tables are capped at.
struct OddShape { int k4, ld; bool fits; };
OddShape odd_width_shape(long long n, int k);

// How ONE k-wide call runs, fp32 (spmm_route) or on the bf16 hot path (spmm_route_bf16): decided once, consumed by the
// launch (api_spmm.cpp) and printed by the reports (gcn_spmm_plan_num_passes / _main_kernel / _main_kernel_bf16 /
// _prelaid_layout).  DESIGN.md §4.19 lists who reads what.
enum class SpmmFamily { panels, unsliced, sliced_quad, group };
enum class BCopy { none, row_padded, group_layout, group_layout_bf16 };   // the copy of B the call lays out first
struct SpmmRoute {
  SpmmFamily family = SpmmFamily::unsliced;
  bool odd = false;                     // computed at k_run = ceil(k / 4) * 4 into a padded result, compacted afterwards
  int k_run = 0;
  int elem_bytes = 4;                   // of the table the main kernels gather from: fp32, or 2 for a bf16 call's bf16 table
  int ldb = 0;                          // row stride B is gathered with, in table elements (k_run: the caller's own rows)
  BCopy copy = BCopy::none;             // (a value-free route's copy has its rows multiplied by u_col)
  bool valless = false, weighted = false, col16 = false;
  SliceSet ss;                          // the slice set a group launch walks
  int S_run = 0;                        // slices the partial rows are sized with (0: not sliced)
  int tile_cols = 0;
  bool reduce_epilogue = false;         // the slice reduction carries bias, ReLU and dropout (else the main kernel / a pass after it)
};
// `build`: build the narrow slice set (k <= 32) at first use, which needs the CSR; without it only what exists is chosen.
// `prelaid`: the caller hands B over in the plan's pre-laid layout (own slice set, rows already scaled, no detour).
SpmmRoute spmm_route(gcn_spmm_plan* p, int k, bool build, const int32_t* rowptr, const int32_t* col, const float* val,
                     hipStream_t st, bool prelaid = false);
// the launch of a non-group route without its pointers: what launch_spmm is handed and spmm_chunk_choice decides from
SpmmArgs spmm_args(const gcn_spmm_plan* p, const SpmmRoute& r, bool epilogue);
// the route of a call that hands B over pre-laid (k % 4 == 0), or GCN_ERR_INVALID_ARG: the plan has no such layout for k
int spmm_route_prelaid(const gcn_spmm_plan* p, int k, SpmmRoute* r);

// true, *r: the route of a bf16 call at width k on the bf16 group walk (the rule stands at the definition); false: the
// fallback (B widened to fp32, the fp32 entry, C narrowed)
bool spmm_route_bf16(gcn_spmm_plan* p, int k, bool build, const int32_t* rowptr, const int32_t* col, const float* val,
                     hipStream_t st, SpmmRoute* r);

// plan_build.cpp
int count_empty(const int* rowptr, int m, int* out, hipStream_t st);
void build_sliced_streams(gcn_spmm_plan* p, hipStream_t st);
void drop_streams(gcn_spmm_plan* p);
void maybe_build_alt(gcn_spmm_plan* p, int cls, const int32_t* rowptr, const int32_t* col, const float* val, hipStream_t st);

// grow-only scratch of a plan; plans may be shared between host threads, so growth is serialised
template <class T>
int grow(DevBuf<T>& buf, size_t count) {
  std::lock_guard<std::mutex> lk(g_plan_mu);
  return buf.grow(count) == hipSuccess ? GCN_OK : GCN_ERR_ALLOC;
}

}  // namespace gcn
