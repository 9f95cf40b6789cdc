// select_rule.h — the selection rule of the max / min units (aggregate.hip, aggregate_multi.hip, edge_message.hip), written
// once: numpy's argmax / argmin.  The first entry in CSR order among equals, -0.0 == +0.0; a NaN beats every number and
// the first NaN wins; +-inf are ordinary values.  No arithmetic touches a value: the bits kept are the winner's bits.
// Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>

namespace gcn {

constexpr int kNone = INT_MAX;                         // "no entry yet" (a stored entry index is below nnz <= INT_MAX)

// is (av, ae) the better candidate than (bv, be)?  A total order (kNone, "no entry", below everything): usable in any
// merge order.
template <bool MAX>
__device__ __forceinline__ bool better(float av, int ae, float bv, int be) {
  const bool an = av != av, bn = bv != bv;
  const bool gt = MAX ? av > bv : av < bv;             // (false when either is a NaN)
  const bool eq = av == bv || (an && bn);
  return ae != kNone && (be == kNone || (an && !bn) || gt || (eq && ae < be));
}

// entry t with the value v into the state (sv, se) of EARLIER entries (ok: the entry exists): a tie keeps the earlier one
template <bool MAX>
__device__ __forceinline__ void select_fold(float& sv, int& se, float v, int t, bool ok) {
  const float b = sv;
  const bool take = ok && (se == kNone || (MAX ? v > b : v < b) || (v != v && b == b));
  sv = take ? v : b;
  se = take ? t : se;
}

// the state (ov, oe) of a disjoint entry set into (sv, se), in any order
template <bool MAX>
__device__ __forceinline__ void select_merge(float& sv, int& se, float ov, int oe) {
  const bool take = better<MAX>(ov, oe, sv, se);
  sv = take ? ov : sv;
  se = take ? oe : se;
}

}  // namespace gcn
