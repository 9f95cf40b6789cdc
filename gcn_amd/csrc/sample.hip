// sample.hip — uniform neighbour sampling without replacement from the rows of a CSR matrix (GraphSAGE's mini-batch
// sampler), as a pure function of (seed, offset, entry index).  Plan-free like aggregate.hip: the caller's CSR, one memset
// node and two kernels, no allocation, no host read of device data, no global atomics — every output element has one
// writer, so the result is the same bits at every call and can be compared integer for integer with a host reference.
//
//   row i of the output belongs to seeds[i] = v; its entries are e in [rowptr[v], rowptr[v + 1]), d of them, fanout f
//   f < 0 or d <= f: every entry is selected (a coalesced copy)
//   otherwise        key(e) = word e & 3 of Philox4x32-10(counter = (e >> 2, offset), key = seed) — the dropout mask's
//                    convention (philox.h) with the entry index in the place of the element index — and the f entries with
//                    the smallest (key(e), e) are selected
//   the selected entries are written in ascending e: out_col[out_rowptr[i] + t] = col[e_t], out_eid[...] = e_t
//
// The unit: ONE ROW PER WORKGROUP, and the workgroup is one wave (64 threads) for a row of at most kSampleLongRow entries
// and four waves (256 threads) for a longer one; both run the same code (sample_row<THREADS>).  A wave per row because the
// rows of the graphs this is for (Reddit: 490 entries on average, fanout 10-25) are a few wave-widths long and need the
// selection, not the copy; a one-wave workgroup makes every barrier below free and lets rows of different lengths finish
// independently (several rows per wave would serialise the four histogram rounds of each).
//
// Lane-to-entry map: thread t of pass p takes the aligned group of four entries 4g .. 4g + 3, g = (rowptr[v] >> 2) + p *
// THREADS + t, so ONE Philox call serves the thread's four keys and a wave's lanes cover 256 consecutive entries in entry
// order (lane-major).  Keys are never stored: a pass recomputes them (10 rounds of two multiplies), except that the keys
// of the first pass stay in registers — a row of at most 4 * THREADS - 3 entries computes each key once.
//
// Selection: an 8-bit radix select, four rounds from the top byte down.  A round counts the keys that match the prefix
// found so far into a 256-bin LDS histogram (LDS integer adds: order-free), scans it (a wave scan, plus the wave totals
// for the four-wave unit) and keeps the bin that holds the f-th smallest key.  After four rounds the threshold key T and
// the number of keys below it are known.  One more walk in entry order writes every entry with key < T and the first
// f - below entries with key == T (the lower entry index wins a tie); the output position is a prefix popcount of
// ballots, and the four waves of a long row exchange their per-pass counts through LDS.
//
// Long rows: the dispatch (the wave kernel, the flag, the long kernel's screening of the seeds) is row_dispatch.h's, shared
// with subgraph.hip and coalesce.hip; the rule looks at the row's length only, selection or copy.  A hub row of tens of
// thousands of entries is 5 sweeps of a few dozen passes on its workgroup.
//
// A seed outside [0, m), a row pointer outside [0, nnz] or an out_rowptr whose row length is not min(d, f) writes nothing.
#include <hip/hip_runtime.h>

#include <climits>

#include "philox.h"
#include "row_dispatch.h"
#include "spmm_kernels.h"

namespace gcn {
namespace {

struct SampleArgs {
  const int* rowptr;
  const int* col;
  const int* seeds;
  const int* out_rowptr;
  int* out_col;
  int* out_eid;
  int m, nnz, count, fanout;                           // count: seeds; fanout: INT_MAX = every entry
  unsigned long long seed, offset;
};

template <int THREADS>
struct SampleScratch {
  unsigned hist[256];                                  // the radix histogram of one round
  int wsum[THREADS / 64];                              // inclusive scan totals of the waves
  int res[2];                                          // the chosen bin and the count below it
  int cnt[2][THREADS / 64][2];                         // per pass parity and wave: (keys < T, keys == T)
};

__device__ __forceinline__ uint4 entry_keys(const SampleArgs& a, int g) {
  return philox4x32_10(make_uint4((uint32_t)g, 0u, (uint32_t)a.offset, (uint32_t)(a.offset >> 32)),
                       make_uint2((uint32_t)a.seed, (uint32_t)(a.seed >> 32)));
}

struct SeedRow { int b, e, o; };                       // the row's entries [b, e) and its output offset

// the row of seed i, or false when the seed, the row or the output slot is not usable
__device__ __forceinline__ bool seed_row(const SampleArgs& a, int i, SeedRow& r) {
  const int v = a.seeds[i];
  if (v < 0 || v >= a.m) return false;
  r.b = a.rowptr[v];
  r.e = a.rowptr[v + 1];
  if (r.b < 0 || r.e < r.b || r.e > a.nnz) return false;
  r.o = a.out_rowptr[i];
  const int d = r.e - r.b, want = d < a.fanout ? d : a.fanout;
  return r.o >= 0 && a.out_rowptr[i + 1] - r.o == want;
}

// one row on a workgroup of THREADS threads (every thread of the workgroup calls it with the same arguments)
template <int THREADS>
__device__ __forceinline__ void sample_row(const SampleArgs& a, const SeedRow& r, SampleScratch<THREADS>& L) {
  constexpr int WAVES = THREADS / 64, BPT = 256 / THREADS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = r.b, e = r.e, o = r.o;
  const int d = e - b, f = a.fanout;
  if (d <= f) {                                        // the whole row
    for (int t = tid; t < d; t += THREADS) {
      a.out_col[o + t] = a.col[b + t];
      a.out_eid[o + t] = b + t;
    }
    return;
  }
  const int g0 = b >> 2, gend = (int)(((long long)e + 3) >> 2);       // groups of four aligned entries that meet the row
  const int passes = (gend - g0 + THREADS - 1) / THREADS;
  const uint4 first = g0 + tid < gend ? entry_keys(a, g0 + tid) : make_uint4(0, 0, 0, 0);
  auto keys_of = [&](int p, int g, unsigned (&k)[4]) {
    const uint4 w = p == 0 ? first : (g < gend ? entry_keys(a, g) : make_uint4(0, 0, 0, 0));
    k[0] = w.x; k[1] = w.y; k[2] = w.z; k[3] = w.w;
  };

  // ---- the f-th smallest key T and the number of keys below it -------------------------------------------------------------
  unsigned prefix = 0, known = 0;
  int krem = f, below = 0;                             // the krem-th smallest among the keys that match the prefix
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int i = tid; i < 256; i += THREADS) L.hist[i] = 0;
    __syncthreads();
    for (int p = 0; p < passes; ++p) {
      const int g = g0 + p * THREADS + tid;
      unsigned k[4];
      keys_of(p, g, k);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long long x = 4ll * g + j;
        if (x >= b && x < e && (k[j] & known) == prefix) atomicAdd(&L.hist[(k[j] >> shift) & 255u], 1u);
      }
    }
    __syncthreads();
    int h[BPT], s = 0;
#pragma unroll
    for (int i = 0; i < BPT; ++i) { h[i] = (int)L.hist[tid * BPT + i]; s += h[i]; }
    int inc = s;
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) {
      const int t = __shfl_up(inc, w);
      if (lane >= w) inc += t;
    }
    if constexpr (WAVES > 1) {
      if (lane == 63) L.wsum[wave] = inc;
      __syncthreads();
      for (int w = 0; w < wave; ++w) inc += L.wsum[w];
    }
    int c = inc - s;                                   // keys in the bins before this thread's
    if (krem - 1 >= c && krem - 1 < inc) {             // (one thread: its bins hold the krem-th key)
      bool done = false;
#pragma unroll
      for (int i = 0; i < BPT; ++i) {
        if (!done && krem - 1 < c + h[i]) { L.res[0] = tid * BPT + i; L.res[1] = c; done = true; }
        if (!done) c += h[i];
      }
    }
    __syncthreads();
    prefix |= (unsigned)L.res[0] << shift;
    known |= 255u << shift;
    below += L.res[1];
    krem -= L.res[1];
  }
  const unsigned T = prefix;
  const int need = f - below;                          // entries with key == T to take, the first in entry order (>= 1)

  // ---- the selected entries, in entry order ----------------------------------------------------------------------------------
  // (not row_dispatch.h's ordered_slots: a wave's "taken" depends on the running count of ties over the waves before it)
  const unsigned long long before = (1ull << lane) - 1ull;
  int run_out = 0, run_eq = 0;                         // written so far / entries with key == T met so far
  for (int p = 0; p < passes; ++p) {
    const int g = g0 + p * THREADS + tid;
    unsigned k[4];
    keys_of(p, g, k);
    bool lt[4], eq[4];
    unsigned long long mlt[4], meq[4];
    int wlt = 0, weq = 0, my_eq = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long x = 4ll * g + j;
      const bool ok = x >= b && x < e;
      lt[j] = ok && k[j] < T;
      eq[j] = ok && k[j] == T;
      mlt[j] = __ballot(lt[j]);
      meq[j] = __ballot(eq[j]);
      wlt += __popcll(mlt[j]);
      weq += __popcll(meq[j]);
      my_eq += __popcll(meq[j] & before);
    }
    int eq_base = run_eq, out_base = run_out;
    if constexpr (WAVES > 1) {
      if (lane == 0) { L.cnt[p & 1][wave][0] = wlt; L.cnt[p & 1][wave][1] = weq; }
      __syncthreads();                                 // (the other parity is what a wave one pass ahead writes)
      int eqs = run_eq;
      for (int w = 0; w < WAVES; ++w) {
        const int clt = L.cnt[p & 1][w][0], ceq = L.cnt[p & 1][w][1];
        const int left = need - eqs;
        const int taken = clt + (left <= 0 ? 0 : (left < ceq ? left : ceq));
        if (w < wave) { out_base += taken; eq_base += ceq; }
        run_out += taken;
        eqs += ceq;
      }
      run_eq = eqs;
    } else {
      const int left = need - run_eq;
      run_out += wlt + (left <= 0 ? 0 : (left < weq ? left : weq));
      run_eq += weq;
    }
    bool sel[4];
    unsigned long long msel[4];
    int rank = eq_base + my_eq;                        // entries with key == T before this thread's, then before entry j
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sel[j] = lt[j] || (eq[j] && rank < need);
      rank += eq[j] ? 1 : 0;
      msel[j] = __ballot(sel[j]);
    }
    int pos = out_base;
#pragma unroll
    for (int j = 0; j < 4; ++j) pos += __popcll(msel[j] & before);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (sel[j] && pos < f) {                         // (pos < f always: exactly f entries are selected)
        const int x = 4 * g + j;
        a.out_col[o + pos] = a.col[x];
        a.out_eid[o + pos] = x;
      }
      pos += sel[j] ? 1 : 0;
    }
  }
}

struct SampleOp : SampleArgs {
  using Row = SeedRow;
  template <int THREADS>
  using Scratch = SampleScratch<THREADS>;
  __device__ bool locate(int i, Row& r) const { return seed_row(*this, i, r); }
  template <int THREADS>
  __device__ __forceinline__ void row(int, const Row& r, Scratch<THREADS>& L) const { sample_row<THREADS>(*this, r, L); }
};

}  // namespace

hipError_t launch_sample_neighbors(const int* rowptr, const int* col, int m, int nnz, const int* seeds, int n_seeds, int fanout,
                                   unsigned long long seed, unsigned long long offset, const int* out_rowptr, int* out_col,
                                   int* out_eid, void* ws, hipStream_t st) {
  const SampleOp op{{rowptr, col, seeds, out_rowptr, out_col, out_eid, m, nnz, n_seeds, fanout < 0 ? INT_MAX : fanout, seed, offset}};
  return launch_rows(op, static_cast<int*>(ws), st);
}

}  // namespace gcn
