// lookup.hip — the two device primitives of link prediction: "is (u, v) stored, and at which entry?" (DGL's has_edges_between /
// edge_ids) and columns that are NOT neighbours of a row (negative sampling), both on a CSR whose rows hold ascending columns.
// Plan-free like sample.hip and subgraph.hip: the caller's CSR, one kernel per call, no workspace, no allocation, no host
// read of device data, no atomics — every output element has one writer, so a call gives the same bits every time and is
// compared integer for integer with a host reference (tests/linkpred_ref.py).  Every access is a 4-byte one: no pointer
// needs more than its type's alignment.
//
// ---- the row search ----------------------------------------------------------------------------------------------------------------
// row_find is written once and serves both kernels: a lower bound over the entries [b, e) of a row, i.e. the lowest x with
// col[x] >= q, and the answer is x when col[x] == q, else -1.  Repeated columns are allowed (the lowest entry index is the
// answer).  The interval [lo, hi) only shrinks and every probe is at lo <= mid < hi, so on a row that does NOT ascend the
// search still ends after at most ceil(log2(e - b + 1)) probes and reads nothing outside [b, e); the answer is then
// unspecified (an entry of the row that holds q, or -1).
//
// ---- the launch ---------------------------------------------------------------------------------------------------------------------
// ONE LANE PER QUERY (find) / PER SLOT (negative sample), as random_walk_kernel has one lane per walk and for its reason: a
// query is a chain of about log2(row length) DEPENDENT 4-byte loads with nothing to share — two lanes of a wave rarely want
// the same row, and a wave per query would leave 63 lanes idle behind the same chain.  The kernels are latency-bound by
// design: what hides a probe's trip to memory is the other waves, not bandwidth, and no bandwidth figure is claimed for
// them.  The first probes of neighbouring queries of one row (the lookup of every stored entry, the slots of one query)
// fall on the same few lines and are served by the caches.
// The launch shape comes from the number of queries alone — the host never reads a row length: one-wave workgroups up to
// kLookupSmall queries (tens to hundreds of waves for 256 CUs x 4 SIMDs: the smallest workgroup spreads them over as many
// CUs as there are), 256-thread workgroups above (a quarter of the workgroups to dispatch when there are millions).  The
// kernels need few registers and no LDS; no occupancy is requested beyond __launch_bounds__.
//
// ---- negative sampling ------------------------------------------------------------------------------------------------------------
//   slot p = i * num_neg + s (64 bits) of query row r = q_rows[i]; try t = 0 .. max_tries - 1 uses j = p * T4 + t with
//   T4 = 4 * ceil(max_tries / 4); key = word (j & 3) of Philox4x32-10(counter = (j >> 2, offset), key = seed) — the
//   random walk's convention; c = (key * n) >> 32; the slot takes the first c that is not stored in row r (row_find) and,
//   with exclude_self, is not r; -1 when every try is refused or the row is unusable.  T4 is a multiple of 4, so
//   j >> 2 = p * (T4 / 4) + (t >> 2): one Philox call serves four consecutive tries and is made when the first of them is
//   needed (a slot that accepts its first candidate — the usual case on a sparse row — makes one call).
#include <hip/hip_runtime.h>

#include "philox.h"
#include "spmm_kernels.h"

namespace gcn {
namespace {

constexpr int kLookupSmall = 1 << 16;                  // up to here one-wave workgroups, above 256-thread ones

// lowest x in [b, e) with col[x] == q, or -1; col ascending over [b, e), 0 <= b <= e (see the file's header)
__device__ __forceinline__ int row_find(const int* __restrict__ col, int b, int e, int q) {
  int lo = b, hi = e;                                  // col[x] < q for x in [b, lo), col[x] >= q for x in [hi, e)
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (col[mid] < q) lo = mid + 1; else hi = mid;
  }
  return lo < e && col[lo] == q ? lo : -1;
}

// the row [b, e) of r, or false when r or its pointers are not usable
__device__ __forceinline__ bool usable_row(const int* __restrict__ rowptr, int m, int nnz, int r, int& b, int& e) {
  if (r < 0 || r >= m) return false;
  b = rowptr[r];
  e = rowptr[r + 1];
  return b >= 0 && e >= b && e <= nnz;
}

struct FindArgs {
  const int* rowptr;
  const int* col;
  const int* q_rows;
  const int* q_cols;
  int* out;
  int m, nnz, count;
};

template <int THREADS>
__global__ void __launch_bounds__(THREADS) find_entries_kernel(FindArgs a) {
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (i >= a.count) return;
  int b, e;
  a.out[i] = usable_row(a.rowptr, a.m, a.nnz, a.q_rows[i], b, e) ? row_find(a.col, b, e, a.q_cols[i]) : -1;
}

struct NegArgs {
  const int* rowptr;
  const int* col;
  const int* q_rows;
  int* out;
  int m, n, nnz, slots, num_neg, max_tries, exclude_self;
  unsigned long long seed, offset;
};

template <int THREADS>
__global__ void __launch_bounds__(THREADS) negative_sample_kernel(NegArgs a) {
  const long long p = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (p >= a.slots) return;
  const int r = a.q_rows[p / a.num_neg];
  int b, e, got = -1;
  if (usable_row(a.rowptr, a.m, a.nnz, r, b, e)) {
    const unsigned long long g0 = (unsigned long long)p * (unsigned long long)((a.max_tries + 3) >> 2);   // (p * T4) >> 2
    const uint2 key = make_uint2((uint32_t)a.seed, (uint32_t)(a.seed >> 32));
    uint32_t words[4] = {0u, 0u, 0u, 0u};
    for (int t = 0; t < a.max_tries; ++t) {
      if ((t & 3) == 0) {
        const unsigned long long g = g0 + (unsigned long long)(t >> 2);
        const uint4 w = philox4x32_10(make_uint4((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)a.offset, (uint32_t)(a.offset >> 32)), key);
        words[0] = w.x; words[1] = w.y; words[2] = w.z; words[3] = w.w;
      }
      const int c = (int)__umulhi(words[t & 3], (uint32_t)a.n);            // in [0, n)
      if (a.exclude_self && c == r) continue;
      if (row_find(a.col, b, e, c) < 0) { got = c; break; }
    }
  }
  a.out[p] = got;
}

}  // namespace

hipError_t launch_find_entries(const int* rowptr, const int* col, int m, int nnz, const int* q_rows, const int* q_cols,
                               int n_queries, int* out_eid, hipStream_t st) {
  const FindArgs a{rowptr, col, q_rows, q_cols, out_eid, m, nnz, n_queries};
  if (n_queries <= kLookupSmall)
    find_entries_kernel<64><<<(unsigned)((n_queries + 63) / 64), 64, 0, st>>>(a);
  else
    find_entries_kernel<256><<<(unsigned)(((long long)n_queries + 255) / 256), 256, 0, st>>>(a);
  return hipGetLastError();
}

hipError_t launch_negative_sample(const int* rowptr, const int* col, int m, int n, int nnz, const int* q_rows, int slots,
                                  int num_neg, int max_tries, int exclude_self, unsigned long long seed,
                                  unsigned long long offset, int* out_cols, hipStream_t st) {
  const NegArgs a{rowptr, col, q_rows, out_cols, m, n, nnz, slots, num_neg, max_tries, exclude_self, seed, offset};
  if (slots <= kLookupSmall)
    negative_sample_kernel<64><<<(unsigned)((slots + 63) / 64), 64, 0, st>>>(a);
  else
    negative_sample_kernel<256><<<(unsigned)(((long long)slots + 255) / 256), 256, 0, st>>>(a);
  return hipGetLastError();
}

}  // namespace gcn
