// subgraph.hip — the two device primitives of subgraph mini-batching (Cluster-GCN, GraphSAINT's random-walk sampler):
// the vertex-induced subgraph of a CSR matrix, and uniform random walks on it.  Plan-free like sample.hip: the caller's
// CSR, at most one memset node and kernels, no allocation, no host read of device data, no global atomics — every output
// element has one writer, so the result is the same bits at every call and is compared integer for integer with a host
// reference (tests/subgraph_ref.py).  Every access is a 4-byte one: no pointer needs more than its type's alignment.
//
// ---- induced subgraph ----------------------------------------------------------------------------------------------------------
//   row i of the output belongs to nodes[i] = v; its entries are the e in [rowptr[v], rowptr[v + 1]) with vmap[col[e]] >= 0,
//   in ascending e: out_col[out_rowptr[i] + t] = vmap[col[e_t]], out_eid[...] = e_t.  vmap [n]: position in nodes, or -1.
// Two calls, because the sizes of out_col / out_eid are the sum of the counts and the caller has to allocate them: COUNT
// writes out_len[i], the caller scans, FILL writes the entries.  Both run the same code (induce_row<THREADS, FILL>).
//
// The unit is sample.hip's: ONE ROW PER WORKGROUP, one wave (64 threads) for a row of at most kSampleLongRow entries and
// four waves (256 threads) for a longer one.  A wave per row because the rows this is for (Reddit: 490 entries on
// average) are a few wave-widths long and a row's output positions are a running count over the row: inside a wave that
// count is a ballot and a popcount, with no barrier and no atomic.  A pass covers THREADS consecutive entries, lane-major
// (coalesced reads of col; the gather from vmap is the scattered part), a lane keeps its entry iff vmap[col[e]] >= 0, and
// the output position is the count of the passes before + the counts of the lower waves of this pass (ordered_slots in
// row_dispatch.h: one barrier per pass) + the popcount of the ballot below the lane.
// FILL first counts the row again and compares the count with the length of the caller's slot (a slot of another length
// writes nothing: the contract), then writes.  The map values of the first kKeep passes stay in registers, so a row of at
// most kKeep * 64 = 256 entries on a wave reads col and vmap once; a longer row reads them a second time (from the caches).
//
// Long rows: the dispatch (the wave kernel, the flag, the long kernel's screening of the nodes) is row_dispatch.h's, shared
// with sample.hip and coalesce.hip; the row functions have nothing else in common with sample.hip's — no keys, no histogram,
// another scratch layout.
//
// A node outside [0, m), a row pointer outside [0, nnz] or (FILL) a slot whose length is not the row's count writes nothing.
//
// ---- random walk -----------------------------------------------------------------------------------------------------------------
//   out_walks [length + 1][n_walks], step-major; out_walks[0][i] = starts[i]; step t of walk i at vertex v with d entries:
//   d == 0 stays; else key = word (j & 3) of Philox4x32-10(counter = (j >> 2, offset), key = seed), j = i * L4 + t with
//   L4 = 4 * ceil(length / 4); pick = (key * d) >> 32; next = col[rowptr[v] + pick] (a column outside [0, m): stays).
// ONE LANE PER WALK.  A walk is a chain of dependent loads — rowptr[v], rowptr[v + 1], then col[...], then the next vertex's
// row pointer — with nothing to share inside it: no two lanes of a wave want the same row, and a wave per walk would leave
// 63 lanes idle behind the same chain.  The parallelism is the number of walks, and what hides the latency of a step (two
// dependent trips to memory, most of them misses on a graph larger than the caches) is other waves.  L4 is a multiple of 4,
// so j >> 2 = i * (L4 / 4) + (t >> 2): one Philox call serves four consecutive steps of a walk.  Stores are step-major, so
// the 64 lanes of a wave store 64 consecutive ints per step.
// Launch: one-wave workgroups (64 threads), ceil(n_walks / 64) of them.  Batches are thousands to tens of thousands of
// walks, i.e. tens to hundreds of waves for 256 CUs x 4 SIMDs: the grid is far below one wave per SIMD, so the smallest
// workgroup spreads the waves over as many CUs (address units, L1s) as there are, and nothing is shared inside a workgroup
// that a larger one would serve.  The kernel needs few registers and no LDS, so when n_walks is large enough to matter the
// hardware limit of 8 waves per SIMD is what is resident; no occupancy is requested beyond __launch_bounds__(64).
#include <hip/hip_runtime.h>

#include "philox.h"
#include "row_dispatch.h"
#include "spmm_kernels.h"

namespace gcn {
namespace {

constexpr int kKeep = 4;                               // passes whose map values stay in registers between count and fill

struct InduceArgs {
  const int* rowptr;
  const int* col;
  const int* nodes;
  const int* vmap;
  int* out_len;                                        // COUNT
  const int* out_rowptr;                               // FILL
  int* out_col;
  int* out_eid;
  int m, nnz, count;                                   // count: nodes
};

template <int THREADS>
struct InduceScratch {
  int wsum[THREADS / 64];                              // the waves' counts of a whole row
  int cnt[2][THREADS / 64];                            // per pass parity and wave: kept entries (ordered_slots)
};

struct NodeRow { int b, e; };

// the row [b, e) of node i, or false when the node or the row is not usable
__device__ __forceinline__ bool node_row(const InduceArgs& a, int i, NodeRow& r) {
  const int v = a.nodes[i];
  if (v < 0 || v >= a.m) return false;
  r.b = a.rowptr[v];
  r.e = a.rowptr[v + 1];
  return r.b >= 0 && r.e >= r.b && r.e <= a.nnz;
}

// one row on a workgroup of THREADS threads (every thread of the workgroup calls it with the same arguments)
template <int THREADS, bool FILL>
__device__ __forceinline__ void induce_row(const InduceArgs& a, int i, const NodeRow& r, InduceScratch<THREADS>& L) {
  constexpr int WAVES = THREADS / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = r.b, e = r.e;
  const int passes = (int)(((long long)e - b + THREADS - 1) / THREADS);
  auto local_of = [&](int p) {                         // the map value of this thread's entry of pass p, -1 past the row
    const long long x = (long long)b + (long long)p * THREADS + tid;
    return x < e ? a.vmap[a.col[x]] : -1;
  };

  // ---- the row's count -----------------------------------------------------------------------------------------------------
  int keep[kKeep];
  int mine = 0;                                        // kept entries of this wave (wave-uniform)
#pragma unroll
  for (int p = 0; p < kKeep; ++p) {
    keep[p] = p < passes ? local_of(p) : -1;
    mine += __popcll(__ballot(keep[p] >= 0));
  }
  for (int p = kKeep; p < passes; ++p) mine += __popcll(__ballot(local_of(p) >= 0));
  int total = mine;
  if constexpr (WAVES > 1) {
    if (lane == 0) L.wsum[wave] = mine;
    __syncthreads();
    total = 0;
    for (int w = 0; w < WAVES; ++w) total += L.wsum[w];
  }
  if constexpr (!FILL) {
    if (tid == 0) a.out_len[i] = total;
    return;
  } else {
    const int o = a.out_rowptr[i];
    if (o < 0 || a.out_rowptr[i + 1] - o != total) return;            // (workgroup-uniform)

    // ---- the kept entries, in entry order ----------------------------------------------------------------------------------
    const unsigned long long before = (1ull << lane) - 1ull;
    int run = 0;                                       // written by the passes so far
    auto pass = [&](int p, int loc) {
      const unsigned long long mask = __ballot(loc >= 0);
      const int pos = ordered_slots<WAVES>(mask, p, L.cnt, run) + __popcll(mask & before);
      if (loc >= 0 && pos < total) {                   // (pos < total always: exactly total entries are kept)
        a.out_col[o + pos] = loc;
        a.out_eid[o + pos] = b + p * THREADS + tid;
      }
    };
#pragma unroll
    for (int p = 0; p < kKeep; ++p)
      if (p < passes) pass(p, keep[p]);
    for (int p = kKeep; p < passes; ++p) pass(p, local_of(p));
  }
}

template <bool FILL>
struct InduceOp : InduceArgs {
  using Row = NodeRow;
  template <int THREADS>
  using Scratch = InduceScratch<THREADS>;
  __device__ bool locate(int i, Row& r) const { return node_row(*this, i, r); }
  template <int THREADS>
  __device__ __forceinline__ void row(int i, const Row& r, Scratch<THREADS>& L) const { induce_row<THREADS, FILL>(*this, i, r, L); }
};

struct WalkArgs {
  const int* rowptr;
  const int* col;
  const int* starts;
  int* out;
  int m, nnz, n_walks, length;
  unsigned long long seed, offset;
};

__global__ void __launch_bounds__(64) random_walk_kernel(WalkArgs a) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.n_walks) return;
  const size_t stride = (size_t)a.n_walks;
  int v = a.starts[i];
  if (v < 0 || v >= a.m) {
    for (int t = 0; t <= a.length; ++t) a.out[t * stride + i] = -1;
    return;
  }
  a.out[i] = v;
  const unsigned long long g0 = (unsigned long long)i * (unsigned long long)((a.length + 3) >> 2);    // (i * L4) >> 2
  const uint2 key = make_uint2((uint32_t)a.seed, (uint32_t)(a.seed >> 32));
  uint32_t words[4] = {0u, 0u, 0u, 0u};
  for (int t = 0; t < a.length; ++t) {
    if ((t & 3) == 0) {
      const unsigned long long g = g0 + (unsigned long long)(t >> 2);
      const uint4 w = philox4x32_10(make_uint4((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)a.offset, (uint32_t)(a.offset >> 32)), key);
      words[0] = w.x; words[1] = w.y; words[2] = w.z; words[3] = w.w;
    }
    const int b = a.rowptr[v], e = a.rowptr[v + 1];
    if (b >= 0 && e > b && e <= a.nnz) {               // (an empty row, or a row pointer outside [0, nnz]: the walk stays)
      const int c = a.col[b + (int)__umulhi(words[t & 3], (uint32_t)(e - b))];
      if (c >= 0 && c < a.m) v = c;
    }
    a.out[(size_t)(t + 1) * stride + i] = v;
  }
}

}  // namespace

hipError_t launch_induced_subgraph_count(const int* rowptr, const int* col, int m, int nnz, const int* nodes, int n_nodes,
                                         const int* vmap, int* out_len, void* ws, hipStream_t st) {
  const InduceOp<false> op{{rowptr, col, nodes, vmap, out_len, nullptr, nullptr, nullptr, m, nnz, n_nodes}};
  return launch_rows(op, static_cast<int*>(ws), st);
}

hipError_t launch_induced_subgraph_fill(const int* rowptr, const int* col, int m, int nnz, const int* nodes, int n_nodes,
                                        const int* vmap, const int* out_rowptr, int* out_col, int* out_eid, void* ws,
                                        hipStream_t st) {
  const InduceOp<true> op{{rowptr, col, nodes, vmap, nullptr, out_rowptr, out_col, out_eid, m, nnz, n_nodes}};
  return launch_rows(op, static_cast<int*>(ws), st);
}

hipError_t launch_random_walk(const int* rowptr, const int* col, int m, int nnz, const int* starts, int n_walks, int length,
                              unsigned long long seed, unsigned long long offset, int* out_walks, hipStream_t st) {
  const WalkArgs a{rowptr, col, starts, out_walks, m, nnz, n_walks, length, seed, offset};
  random_walk_kernel<<<(unsigned)((n_walks + 63) / 64), 64, 0, st>>>(a);
  return hipGetLastError();
}

}  // namespace gcn
