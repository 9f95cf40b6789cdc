// spgemm.hip — C = A * B for two CSR matrices on the device (SpGEMM): row-wise Gustavson in two calls, COUNT (the length of
// every row of C), the caller's scan, FILL (the columns, ascending, and the values).  Plan-free like coalesce.hip: the
// caller's arrays and workspace, one memset node and three kernels per call, no allocation, no host read of device data,
// no floating-point atomic.  The contract (the pattern, the order of the products of an entry, what a bad operand does) is
// written out in include/gcn_spmm.h; tests/spgemm_ref.py is its numpy twin, bit for bit.
//
// ---- the fold order ------------------------------------------------------------------------------------------------------------
// A row of C belongs to one UNIT, a wave or a 256-thread workgroup.  The unit takes the entries (i, j) of A's row one after
// another; for each, its threads spread over row j of B, one product a * b per thread and step, and put it into the row's
// accumulator under the key c = the column of b.  B holds a column once per row, so inside one step no two threads meet in
// a slot: the value of a slot is written (first touch) or read, added to and written back by the one thread that holds its
// column in this step, never atomically.  Between two entries of A the unit synchronises (a barrier for a workgroup; a wave
// runs in step with itself and needs the compiler kept in order only), so the products of an output entry are added in A's
// entry order: the result is a pure function of the operands.  Every wave loads A's entries 64 at a time, a lane each, with
// the bounds of the B row they point at, and hands them round by lane broadcast: no dependent load chain per entry.
//
// ---- three accumulators, chosen by K_i = min(U_i, n) ---------------------------------------------------------------------------
// U_i = the number of products of row i (the lengths of the B rows its entries point at, added up, saturating at 2^31 - 1):
// an upper bound of the row's length that needs no hash table to compute.  The wave kernel computes it for every row, keeps
// it in the workspace and takes the row itself when K_i <= kSpgemmWaveMax; the other two kernels find their rows by
// screening that array (the screening loop of row_dispatch.h, with this file's predicate) and leave at once when the wave
// kernel has raised no flag for their class.  COUNT and FILL compute the same U_i, hence agree on every row's class.
//   K_i <= kSpgemmWaveMax (512)    a wave per row, four rows per workgroup, a table per wave in LDS
//   K_i <= kSpgemmBlockMax (8192)  a 256-thread workgroup per row, one table in LDS (dynamic: 64 KiB of keys, 64 KiB of values)
//   above                          a 256-thread workgroup per row, kSpgemmDenseBlocks (16) of them: an n-word stamp array and
//                                  n floats of the workspace each; stamp[c] == i + 1 says that row i has touched column c, so
//                                  the stamps are zeroed once per kernel and not between the rows of a workgroup
// The tables are open-addressed, linear probing from c & (slots - 1), slots = the power of two >= 2 K_i (at least 64): at
// most half full, and a short row neither clears nor sorts 1024 slots.  A key is claimed by an integer compare-and-swap in
// LDS; which thread wins decides where a key sits, never which keys there are.  COUNT needs keys only.
// The output order: the table is sorted in place by key, the empty key (INT_MAX) last — a bitonic network over the slots,
// values moving with their keys — and its first `count` slots are the row.  The dense rows come out ascending from a scan of
// their stamps, 256 columns a pass, with ballots and ordered_slots (row_dispatch.h).
#include <hip/hip_runtime.h>

#include <climits>

#include "row_dispatch.h"
#include "spmm_kernels.h"

// The contract rounds every product and every sum once.  HIP's __fmul_rn / __fadd_rn are a plain * and + defined in its
// headers, where the compiler's default (-ffp-contract=fast-honor-pragmas) lets it fuse them into one FMA once they are
// inlined — it did in the dense accumulator's read-add-write.  So the two operations are written here, as mul_rn / add_rn,
// with contraction off for everything this file defines.
#pragma clang fp contract(off)

namespace gcn {
namespace {

constexpr int kEmpty = INT_MAX;                        // no column: a column is < n <= INT_MAX
constexpr int kWaveSlots = 2 * kSpgemmWaveMax, kBlockSlots = 2 * kSpgemmBlockMax;

struct SpgemmArgs {
  const int* a_rowptr; const int* a_col; const float* a_val;
  const int* b_rowptr; const int* b_col; const float* b_val;
  int* out_len;                                        // COUNT
  const int* out_rowptr;                               // FILL
  int* out_col;
  float* out_val;
  int* flags;                                          // ws: [0] a row of the workgroup class exists, [1] a dense row exists
  int* u;                                              // ws: [m] the rows' product counts, saturated
  int* stamps;                                         // ws: [kSpgemmDenseBlocks][n]
  float* dvals;                                        // ws: [kSpgemmDenseBlocks][n]
  int m, p, n, nnz_a, nnz_b;
};

__device__ __forceinline__ int row_class(int u, int n) {
  const int K = u < n ? u : n;
  return K <= kSpgemmWaveMax ? 0 : K <= kSpgemmBlockMax ? 1 : 2;
}

__device__ __forceinline__ int table_slots(int K) {     // the power of two >= 2 K, at least 64
  int s = 64;
  while (s < 2 * K) s <<= 1;
  return s;
}

// the entries [b, e) of A's row i — none when its row pointer is not usable
__device__ __forceinline__ void a_row(const SpgemmArgs& a, int i, int& b, int& e) {
  b = a.a_rowptr[i];
  e = a.a_rowptr[i + 1];
  if (b < 0 || e < b || e > a.nnz_a) b = e = 0;
}

// the entries [s, t) of the B row that A's entry x points at — none when the column or the row pointer is not usable
__device__ __forceinline__ void b_row(const SpgemmArgs& a, long long x, int& s, int& t) {
  s = t = 0;
  const int j = a.a_col[x];
  if (j < 0 || j >= a.p) return;
  const int rb = a.b_rowptr[j], re = a.b_rowptr[j + 1];
  if (rb >= 0 && re >= rb && re <= a.nnz_b) { s = rb; t = re; }
}

// what orders the steps of a unit: a barrier for a workgroup; a wave only has to keep the compiler from moving LDS accesses
template <int THREADS>
__device__ __forceinline__ void unit_sync() {
  if constexpr (THREADS > 64) {
    __syncthreads();
  } else {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// the sum of v over the unit (wsum: the workgroup's exchange, free again on return)
template <int THREADS>
__device__ __forceinline__ int unit_sum(int v, int* wsum) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if constexpr (THREADS > 64) {
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    v = 0;
    for (int w = 0; w < THREADS / 64; ++w) v += wsum[w];
    __syncthreads();
  }
  return v;
}

// The products of A's row [b, e) in the contract's order: f(c, av, y) for every entry y of B (column c, inside [0, n)) under
// every entry of A (value av), A's entries one after another with unit_sync between them.  tid: the thread's number in the
// unit; every thread of the unit calls it with the same row.
template <int THREADS, class F>
__device__ __forceinline__ void for_products(const SpgemmArgs& a, int b, int e, int tid, F&& f) {
  const int lane = tid & 63;
  for (long long x0 = b; x0 < e; x0 += 64) {
    const long long x = x0 + lane;                     // this lane's entry of A: its B row and its value
    int s = 0, t = 0;
    float av = 1.0f;
    if (x < e) {
      b_row(a, x, s, t);
      if (a.a_val) av = a.a_val[x];
    }
    const int cnt = e - x0 < 64 ? (int)(e - x0) : 64;
    for (int q = 0; q < cnt; ++q) {
      const int ys = __shfl(s, q, 64), yt = __shfl(t, q, 64);
      const float v = __shfl(av, q, 64);
      if (ys == yt) continue;                          // (unit-uniform)
      for (long long y = (long long)ys + tid; y < yt; y += THREADS) {
        const int c = a.b_col[y];
        if (c >= 0 && c < a.n) f(c, v, y);
      }
      unit_sync<THREADS>();
    }
  }
}

__device__ __forceinline__ float mul_rn(float x, float y) { return x * y; }      // (one rounding each: contraction is off)
__device__ __forceinline__ float add_rn(float x, float y) { return x + y; }

__device__ __forceinline__ float product(const SpgemmArgs& a, float av, long long y) {
  return mul_rn(av, a.b_val ? a.b_val[y] : 1.0f);
}

// ---- the LDS table -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void table_add(int* keys, float* vals, int mask, int c, bool values, float prod) {
  int s = c & mask;
  for (int probes = 0; probes <= mask; ++probes) {     // (at most half full: the bound only rules out a spin)
    const int old = atomicCAS(&keys[s], kEmpty, c);
    if (old == kEmpty) {                               // first touch
      if (values) vals[s] = prod;
      return;
    }
    if (old == c) {                                    // this column belongs to this thread for the step
      if (values) vals[s] = add_rn(vals[s], prod);
      return;
    }
    s = (s + 1) & mask;
  }
}

// ascending by key, in place: a bitonic network over the slots (a power of two), the values with their keys
template <int THREADS>
__device__ __forceinline__ void sort_table(int* keys, float* vals, int slots, int tid, bool values) {
  for (int k = 2; k <= slots; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < slots / 2; t += THREADS) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const int kl = keys[lo], kh = keys[hi];
        if ((kl > kh) == ((lo & k) == 0)) {
          keys[lo] = kh;
          keys[hi] = kl;
          if (values) {
            const float v = vals[lo];
            vals[lo] = vals[hi];
            vals[hi] = v;
          }
        }
      }
      unit_sync<THREADS>();
    }
  }
}

// one row of at most kSpgemmWaveMax / kSpgemmBlockMax possible columns on a unit of THREADS threads and its table
template <int THREADS, bool FILL>
__device__ __forceinline__ void table_row(const SpgemmArgs& a, int i, int b, int e, int K, int* keys, float* vals, int tid,
                                          int* wsum) {
  const int slots = table_slots(K), mask = slots - 1;
  const bool values = FILL && a.out_val != nullptr;
  for (int s = tid; s < slots; s += THREADS) keys[s] = kEmpty;
  unit_sync<THREADS>();
  for_products<THREADS>(a, b, e, tid, [&](int c, float av, long long y) {
    table_add(keys, vals, mask, c, values, values ? product(a, av, y) : 0.0f);
  });
  int mine = 0;
  for (int s = tid; s < slots; s += THREADS) mine += keys[s] != kEmpty;
  const int total = unit_sum<THREADS>(mine, wsum);
  if constexpr (!FILL) {
    if (tid == 0) a.out_len[i] = total;
  } else {
    const int o = a.out_rowptr[i];
    if (o < 0 || a.out_rowptr[i + 1] - o != total) return;               // (unit-uniform)
    sort_table<THREADS>(keys, vals, slots, tid, values);
    for (int s = tid; s < total; s += THREADS) {
      a.out_col[(long long)o + s] = keys[s];
      if (values) a.out_val[(long long)o + s] = vals[s];
    }
  }
}

// ---- a wave per row ------------------------------------------------------------------------------------------------------------
template <bool FILL>
__global__ void __launch_bounds__(256) spgemm_wave_kernel(SpgemmArgs a) {
  __shared__ int keys[4][kWaveSlots];
  __shared__ float vals[FILL ? 4 : 1][FILL ? kWaveSlots : 1];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + wave;
  if (row >= a.m) return;                              // (a wave leaves as a whole; no barrier in this kernel)
  const int i = (int)row;
  int b, e;
  a_row(a, i, b, e);
  long long u = 0;
  for (long long x = (long long)b + lane; x < e; x += 64) {
    int s, t;
    b_row(a, x, s, t);
    u += t - s;
  }
  for (int off = 32; off > 0; off >>= 1) u += __shfl_xor(u, off, 64);
  const int ui = u > INT_MAX ? INT_MAX : (int)u;
  if (lane == 0) a.u[i] = ui;
  const int cls = row_class(ui, a.n);
  if (cls != 0) {
    if (lane == 0) a.flags[cls - 1] = 1;               // (every writer writes the same word)
    return;
  }
  const int K = ui < a.n ? ui : a.n;
  if (K == 0) {
    if constexpr (!FILL)
      if (lane == 0) a.out_len[i] = 0;
    return;
  }
  table_row<64, FILL>(a, i, b, e, K, keys[wave], vals[FILL ? wave : 0], lane, nullptr);
}

// ---- a workgroup per row: the LDS table and the dense accumulator ---------------------------------------------------------------
struct BlockScratch {
  int is_mine[256];
  int wsum[4];
  int cnt[2][4];
};

template <bool FILL>
__device__ __forceinline__ void dense_row(const SpgemmArgs& a, int i, int b, int e, int* stamp, float* dv, BlockScratch& L) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int mark = i + 1;
  const bool values = FILL && a.out_val != nullptr;
  for_products<256>(a, b, e, tid, [&](int c, float av, long long y) {
    if (stamp[c] != mark) {                            // first touch
      stamp[c] = mark;
      if (values) dv[c] = product(a, av, y);
    } else if (values) {
      dv[c] = add_rn(dv[c], product(a, av, y));
    }
  });
  int mine = 0;
  for (long long c = tid; c < a.n; c += 256) mine += stamp[c] == mark;
  const int total = unit_sum<256>(mine, L.wsum);
  if constexpr (!FILL) {
    if (tid == 0) a.out_len[i] = total;
  } else {
    const int o = a.out_rowptr[i];
    if (o < 0 || a.out_rowptr[i + 1] - o != total) return;               // (workgroup-uniform)
    const unsigned long long below = (1ull << lane) - 1ull;
    const int passes = (int)(((long long)a.n + 255) / 256);
    int run = 0;
    for (int p = 0; p < passes; ++p) {
      const long long c = (long long)p * 256 + tid;
      const bool hit = c < a.n && stamp[c] == mark;
      const unsigned long long mask = __ballot(hit);
      const int base = ordered_slots<4>(mask, p, L.cnt, run);
      if (!hit) continue;
      const int k = base + __popcll(mask & below);
      if (k >= total) continue;                        // (never: exactly `total` columns carry the mark)
      a.out_col[(long long)o + k] = (int)c;
      if (values) a.out_val[(long long)o + k] = dv[c];
    }
  }
}

// CLS 1: the rows of the workgroup class, table in dynamic LDS; CLS 2: the dense rows.  The grid is fixed; workgroup w owns
// the rows w, w + G, w + 2G, ... and screens their product counts 256 at a time (row_dispatch.h's loop).
template <bool FILL, int CLS>
__global__ void __launch_bounds__(256) spgemm_block_kernel(SpgemmArgs a) {
  extern __shared__ int table[];                       // CLS 1: kBlockSlots keys, then in the fill kBlockSlots values
  __shared__ BlockScratch L;
  if (a.flags[CLS - 1] == 0) return;
  const int tid = threadIdx.x;
  const int G = gridDim.x;
  int* stamp = nullptr;
  float* dv = nullptr;
  if constexpr (CLS == 2) {
    stamp = a.stamps + (size_t)blockIdx.x * (size_t)a.n;
    dv = a.dvals + (size_t)blockIdx.x * (size_t)a.n;
    for (long long c = tid; c < a.n; c += 256) stamp[c] = 0;
    __syncthreads();
  }
  const int mine = (int)(((long long)a.m - (long long)blockIdx.x + G - 1) / G);
  for (int q0 = 0; q0 < mine; q0 += 256) {
    const int q = q0 + tid;
    L.is_mine[tid] = q < mine && row_class(a.u[blockIdx.x + q * G], a.n) == CLS;
    __syncthreads();
    const int top = mine - q0 < 256 ? mine - q0 : 256;
    for (int t = 0; t < top; ++t) {
      if (!L.is_mine[t]) continue;                     // (workgroup-uniform)
      const int i = blockIdx.x + (q0 + t) * G;
      int b, e;
      a_row(a, i, b, e);
      if constexpr (CLS == 1) {
        const int ui = a.u[i];
        table_row<256, FILL>(a, i, b, e, ui < a.n ? ui : a.n, table, reinterpret_cast<float*>(table + kBlockSlots), tid, L.wsum);
      } else {
        dense_row<FILL>(a, i, b, e, stamp, dv, L);
      }
      __syncthreads();                                 // (the next row overwrites the table and the exchange words)
    }
    __syncthreads();                                   // (the next screening overwrites is_mine)
  }
}

template <bool FILL>
hipError_t launch(SpgemmArgs a, void* ws, hipStream_t st) {
  char* w = static_cast<char*>(ws);
  a.flags = reinterpret_cast<int*>(w);
  a.u = reinterpret_cast<int*>(w + 16);
  a.stamps = reinterpret_cast<int*>(w + 16 + ((size_t)a.m * 4 + 15) / 16 * 16);
  a.dvals = reinterpret_cast<float*>(a.stamps + (size_t)kSpgemmDenseBlocks * (size_t)a.n);
  if (hipError_t err = hipMemsetAsync(a.flags, 0, 16, st); err != hipSuccess) return err;
  spgemm_wave_kernel<FILL><<<(unsigned)(((long long)a.m + 3) / 4), 256, 0, st>>>(a);
  if (hipError_t err = hipGetLastError(); err != hipSuccess) return err;
  const size_t lds = (size_t)kBlockSlots * (FILL ? 8 : 4);
  if (hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(&spgemm_block_kernel<FILL, 1>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      err != hipSuccess)
    return err;
  spgemm_block_kernel<FILL, 1><<<(unsigned)(a.m < kLongBlocks ? a.m : kLongBlocks), 256, lds, st>>>(a);
  if (hipError_t err = hipGetLastError(); err != hipSuccess) return err;
  spgemm_block_kernel<FILL, 2><<<(unsigned)(a.m < kSpgemmDenseBlocks ? a.m : kSpgemmDenseBlocks), 256, 0, st>>>(a);
  return hipGetLastError();
}

}  // namespace

size_t spgemm_workspace_bytes(int m, int n) {
  return 16 + ((size_t)m * 4 + 15) / 16 * 16 + 8 * (size_t)n * (size_t)kSpgemmDenseBlocks;
}

hipError_t launch_spgemm_count(const int* a_rowptr, const int* a_col, int m, int p, int nnz_a, const int* b_rowptr,
                               const int* b_col, int n, int nnz_b, int* out_len, void* ws, hipStream_t st) {
  return launch<false>(SpgemmArgs{a_rowptr, a_col, nullptr, b_rowptr, b_col, nullptr, out_len, nullptr, nullptr, nullptr,
                                  nullptr, nullptr, nullptr, nullptr, m, p, n, nnz_a, nnz_b}, ws, st);
}

hipError_t launch_spgemm_fill(const int* a_rowptr, const int* a_col, const float* a_val, int m, int p, int nnz_a,
                              const int* b_rowptr, const int* b_col, const float* b_val, int n, int nnz_b,
                              const int* out_rowptr, int* out_col, float* out_val, void* ws, hipStream_t st) {
  return launch<true>(SpgemmArgs{a_rowptr, a_col, a_val, b_rowptr, b_col, b_val, nullptr, out_rowptr, out_col, out_val,
                                 nullptr, nullptr, nullptr, nullptr, m, p, n, nnz_a, nnz_b}, ws, st);
}

}  // namespace gcn
