// construct.hip — building and transposing CSR on the device.  Both reduce to one primitive, STABLE BUCKETING of the indices
// 0 .. count - 1 by an integer key:
//   perm[offsets[b] .. offsets[b + 1]) = the i with keys[i] == b, in ascending i       (np.argsort(keys, kind="stable"),
//   offsets = the exclusive prefix sum of the buckets' lengths                           np.bincount + cumsum)
// A CSR transpose is the bucketing of the entries by column, an edge list becomes CSR by bucketing by row (after a bucketing
// by column when the rows are to come out column-sorted: two stable passes are an LSD sort on (row, column)).
// Plan-free like subgraph.hip and in its shape — a COUNT call, the caller's scan, a FILL call — with the caller's arrays,
// memset / copy nodes and kernels, no allocation and no host read of device data.
//
// ---- count -----------------------------------------------------------------------------------------------------------------------
// offsets[0 .. nbuckets] is zeroed, then one lane per key adds to offsets[key + 1].  Integer adds commute, so the counts are
// the same bits whatever order the atomics land in.  The lanes of a wave that hold the same key are found first (wave_groups:
// a ballot per distinct key of the wave) and only the first of them issues the atomic, with the group's size: a hub column
// of 20 k entries is then a few hundred adds on its word instead of 20 k, which a single address would serialise at the
// memory side.
//
// ---- fill ------------------------------------------------------------------------------------------------------------------------
// 1. SCATTER.  cursor = a copy of the scanned offsets (workspace).  One lane per key, grouped as above: the group's first
//    lane draws base = atomicAdd(cursor[key], size), lane r of the group writes i to perm[base + r].  Every bucket now holds
//    exactly its indices, in an order that depends on how the atomics landed.
// 2. ORDER.  The indices of a bucket are distinct, so sorting the bucket ascending gives the one right answer and takes the
//    landing order out of the result.  A classification pass (a lane per bucket) puts the buckets that need sorting on one of
//    three lists in the workspace — ballot-compacted, one atomic per wave and list — and three kernels with fixed grids walk
//    the lists (a workgroup beyond its list's end leaves at once), so the host never learns a length:
//      length 0 or 1                    nothing: on no list, no per-bucket work (most buckets of a sampled block)
//      2 .. kBucketWaveMax              one wave, the bucket in 1 KiB of LDS, a bitonic network (barriers of a one-wave
//                                       workgroup are free)
//      .. kBucketBlockMax               a 256-thread workgroup, the bucket in 32 KiB of LDS, the same network
//      longer                           one 512-thread workgroup on the bucket in place in global memory (L2): LDS-sized
//                                       chunks are sorted in LDS, then the network's remaining merge levels run their
//                                       wide strides on global memory and their narrow ones in LDS again, chunk by chunk
//    The network is the bitonic sorter whose merges start with a mirrored step (partner i ^ (k - 1)) so that EVERY
//    compare-exchange puts the smaller value at the lower index.  A bucket whose length is not a power of two is then
//    sorted as if padded with +infinity: a pair whose upper index is past the end is skipped, and nothing is padded.
//    The order of a list does not matter (buckets are independent), so the result does not depend on any atomic's order.
// Out-of-contract input writes nothing out of bounds: a key outside [0, nbuckets), a cursor position outside [0, count) or
// a bucket range outside perm is skipped.
//
// ---- transpose gather ------------------------------------------------------------------------------------------------------------
// One lane per transposed entry t: e = perm[t], trow[t] = the row r with rowptr[r] <= e < rowptr[r + 1] by binary search
// (rowptr is (m + 1) * 4 bytes and stays in L2: 0.9 MB for Reddit), tval[t] = val[e].  No nnz-sized 64-bit temporaries.
#include <hip/hip_runtime.h>

#include "spmm_kernels.h"

namespace gcn {
namespace {

constexpr int kWaveMax = kBucketWaveMax;
constexpr int kBlockMax = kBucketBlockMax;
constexpr int kWaveGrid = 8192, kBlockGrid = 2048, kLongGrid = 1024;      // workgroups of the three list walkers
constexpr int kBlockThreads = 256, kLongThreads = 512;

struct Caps {                                          // the capacities of the three lists (in buckets)
  int wave, block, lng;
};

__host__ __device__ inline int min_int(long long a, long long b) { return (int)(a < b ? a : b); }

// how many buckets can be longer than `above` entries: no more than there are, and no more than count / (above + 1)
inline Caps list_caps(int count, int nbuckets) {
  return Caps{min_int(nbuckets, count / 2), min_int(nbuckets, count / (kWaveMax + 1)), min_int(nbuckets, count / (kBlockMax + 1))};
}

// workspace, in ints: 4 counters (1..3: the lists' lengths) | cursor [nbuckets] | wave list | block list | long list
struct Ws {
  int* counters;
  int* cursor;
  int* wave_list;
  int* block_list;
  int* long_list;
};

inline Ws carve(void* ws, int nbuckets, const Caps& c) {
  int* p = static_cast<int*>(ws);
  return Ws{p, p + 4, p + 4 + (size_t)nbuckets, p + 4 + (size_t)nbuckets + c.wave, p + 4 + (size_t)nbuckets + c.wave + c.block};
}

// The lanes of the wave that hold the same key as this one (inactive lanes belong to no group): the group's first lane,
// this lane's rank in the group in lane order, and the group's size.  One iteration per distinct key of the wave.
__device__ __forceinline__ void wave_groups(int key, bool active, int& leader, int& rank, int& size) {
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned long long todo = __ballot(active);
  leader = lane; rank = 0; size = 0;
  while (todo) {                                       // (wave-uniform)
    const int first = __ffsll((long long)todo) - 1;
    const int k = __shfl(key, first);
    const bool mine = active && key == k;
    const unsigned long long same = __ballot(mine);
    if (mine) {
      leader = first;
      rank = __popcll(same & below);
      size = __popcll(same);
    }
    todo &= ~same;
  }
}

__global__ void __launch_bounds__(256) bucket_count_kernel(const int* __restrict__ keys, int count, int nbuckets,
                                                           int* __restrict__ offsets) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int key = i < count ? keys[i] : -1;
  const bool active = i < count && key >= 0 && key < nbuckets;
  int leader, rank, size;
  wave_groups(key, active, leader, rank, size);
  if (active && rank == 0) atomicAdd(&offsets[key + 1], size);
}

__global__ void __launch_bounds__(256) bucket_scatter_kernel(const int* __restrict__ keys, int count, int nbuckets,
                                                             int* __restrict__ cursor, int* __restrict__ perm) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const int key = i < count ? keys[i] : -1;
  const bool active = i < count && key >= 0 && key < nbuckets;
  int leader, rank, size;
  wave_groups(key, active, leader, rank, size);
  int base = 0;
  if (active && rank == 0) base = atomicAdd(&cursor[key], size);
  base = __shfl(base, leader);
  const long long pos = (long long)base + rank;
  if (active && base >= 0 && pos < count) perm[pos] = (int)i;
}

// a lane per bucket: the buckets of two or more entries onto the list of their tier
__global__ void __launch_bounds__(256) bucket_classify_kernel(const int* __restrict__ offsets, int nbuckets, Ws w, Caps caps) {
  const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  int tier = 0;
  if (b < nbuckets) {
    const int len = offsets[b + 1] - offsets[b];
    tier = len < 2 ? 0 : len <= kWaveMax ? 1 : len <= kBlockMax ? 2 : 3;
  }
  for (int t = 1; t <= 3; ++t) {
    const unsigned long long mask = __ballot(tier == t);
    if (mask == 0) continue;                           // (wave-uniform)
    const int first = __ffsll((long long)mask) - 1;
    int base = 0;
    if (lane == first) base = atomicAdd(&w.counters[t], __popcll(mask));
    base = __shfl(base, first);
    const int pos = base + __popcll(mask & below);
    int* list = t == 1 ? w.wave_list : t == 2 ? w.block_list : w.long_list;
    const int cap = t == 1 ? caps.wave : t == 2 ? caps.block : caps.lng;
    if (tier == t && pos >= 0 && pos < cap) list[pos] = (int)b;
  }
}

// One step of the network on a[0, n): pair p is (i, i + j), or with FLIP (i, i ^ (2j - 1)), the mirrored first step of a
// merge of blocks of 2j; the smaller value goes to the lower index, a pair that reaches past n is left alone.
template <int THREADS, bool FLIP>
__device__ __forceinline__ void cex_step(int* a, unsigned n, unsigned pairs, unsigned j) {
  for (unsigned p = threadIdx.x; p < pairs; p += THREADS) {
    const unsigned i = ((p & ~(j - 1u)) << 1) | (p & (j - 1u));
    const unsigned q = FLIP ? (i ^ (2u * j - 1u)) : (i + j);
    if (q < n) {
      const int x = a[i], y = a[q];
      if (x > y) {
        a[i] = y;
        a[q] = x;
      }
    }
  }
}

__device__ __forceinline__ unsigned pow2_ceil(unsigned n) {
  unsigned p = 1;
  while (p < n) p <<= 1;
  return p;
}

// a[0, n) ascending, a in LDS; every thread of the workgroup calls it after a barrier, and it ends with one
template <int THREADS>
__device__ __forceinline__ void sort_lds(int* a, unsigned n) {
  const unsigned n2 = pow2_ceil(n), pairs = n2 >> 1;
  for (unsigned k = 2; k <= n2; k <<= 1) {
    cex_step<THREADS, true>(a, n, pairs, k >> 1);
    __syncthreads();
    for (unsigned j = k >> 2; j >= 1; j >>= 1) {
      cex_step<THREADS, false>(a, n, pairs, j);
      __syncthreads();
    }
  }
}

// the range of bucket list[q] in perm, or false when it is not one this kernel may touch (workgroup-uniform)
__device__ __forceinline__ bool bucket_range(const int* offsets, int b, int nbuckets, int count, int least, int most, int& lo,
                                             int& len) {
  if (b < 0 || b >= nbuckets) return false;
  lo = offsets[b];
  len = offsets[b + 1] - lo;
  return lo >= 0 && len >= least && len <= most && lo <= count - len;
}

template <int THREADS, int CAP>
__global__ void __launch_bounds__(THREADS) sort_buckets_kernel(const int* __restrict__ offsets, int nbuckets, int count,
                                                               const int* __restrict__ list, const int* __restrict__ n_list,
                                                               int cap, int* __restrict__ perm) {
  __shared__ int a[CAP];
  const int n = *n_list < cap ? *n_list : cap;
  for (int q = blockIdx.x; q < n; q += gridDim.x) {
    int lo, len;
    if (!bucket_range(offsets, list[q], nbuckets, count, 2, CAP, lo, len)) continue;
    for (int t = threadIdx.x; t < len; t += THREADS) a[t] = perm[lo + t];
    __syncthreads();
    sort_lds<THREADS>(a, (unsigned)len);
    for (int t = threadIdx.x; t < len; t += THREADS) perm[lo + t] = a[t];
    __syncthreads();                                   // (the next bucket overwrites a)
  }
}

// a bucket longer than LDS holds, in place: one workgroup, barriers order its own global accesses
template <int THREADS, int CAP>
__global__ void __launch_bounds__(THREADS) sort_long_kernel(const int* __restrict__ offsets, int nbuckets, int count,
                                                            const int* __restrict__ list, const int* __restrict__ n_list, int cap,
                                                            int* perm) {
  __shared__ int a[CAP];
  const int nl = *n_list < cap ? *n_list : cap;
  for (int q = blockIdx.x; q < nl; q += gridDim.x) {
    int lo, len;
    if (!bucket_range(offsets, list[q], nbuckets, count, CAP + 1, count, lo, len)) continue;
    int* g = perm + lo;
    const unsigned n = (unsigned)len;
    // every aligned chunk of CAP entries through LDS: sorted (full), or the last log2(CAP) steps of a merge level
    auto sweep = [&](bool full) {
      for (unsigned c = 0; c < n; c += CAP) {
        const unsigned m = n - c < (unsigned)CAP ? n - c : (unsigned)CAP;
        for (unsigned t = threadIdx.x; t < m; t += THREADS) a[t] = g[c + t];
        __syncthreads();
        if (full) {
          sort_lds<THREADS>(a, m);
        } else {
          for (unsigned j = CAP / 2; j >= 1; j >>= 1) {
            cex_step<THREADS, false>(a, m, CAP / 2, j);
            __syncthreads();
          }
        }
        for (unsigned t = threadIdx.x; t < m; t += THREADS) g[c + t] = a[t];
        __syncthreads();
      }
    };
    sweep(true);
    const unsigned n2 = pow2_ceil(n), pairs = n2 >> 1;
    for (unsigned k = 2u * CAP; k <= n2 && k != 0; k <<= 1) {
      cex_step<THREADS, true>(g, n, pairs, k >> 1);
      __syncthreads();
      for (unsigned j = k >> 2; j >= (unsigned)CAP; j >>= 1) {
        cex_step<THREADS, false>(g, n, pairs, j);
        __syncthreads();
      }
      sweep(false);
    }
  }
}

__global__ void __launch_bounds__(256) transpose_gather_kernel(const int* __restrict__ rowptr, int m, int nnz,
                                                               const int* __restrict__ perm, const float* __restrict__ val,
                                                               int* __restrict__ trow, float* __restrict__ tval) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= nnz) return;
  const int e = perm[t];
  if (e < 0 || e >= nnz) {                             // (not a permutation of the entries: no row, and val is not read)
    trow[t] = -1;
    if (val) tval[t] = 0.f;
    return;
  }
  int lo = 0, hi = m - 1;                              // the last row r with rowptr[r] <= e
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if (rowptr[mid] <= e) lo = mid; else hi = mid - 1;
  }
  trow[t] = lo;
  if (val) tval[t] = val[e];
}

inline unsigned blocks_of(long long items, int per) { return (unsigned)((items + per - 1) / per); }

}  // namespace

size_t bucket_workspace_bytes(int count, int nbuckets) {
  const Caps c = list_caps(count, nbuckets);
  const size_t ints = 4 + (size_t)nbuckets + (size_t)c.wave + (size_t)c.block + (size_t)c.lng;
  return (ints * 4 + 15) / 16 * 16;
}

hipError_t launch_bucket_count(const int* keys, int count, int nbuckets, int* offsets, hipStream_t st) {
  if (hipError_t err = hipMemsetAsync(offsets, 0, ((size_t)nbuckets + 1) * sizeof(int), st); err != hipSuccess) return err;
  if (count == 0 || nbuckets == 0) return hipSuccess;
  bucket_count_kernel<<<blocks_of(count, 256), 256, 0, st>>>(keys, count, nbuckets, offsets);
  return hipGetLastError();
}

hipError_t launch_bucket_fill(const int* keys, int count, int nbuckets, const int* offsets, int* perm, void* ws, hipStream_t st) {
  const Caps caps = list_caps(count, nbuckets);
  const Ws w = carve(ws, nbuckets, caps);
  if (hipError_t err = hipMemsetAsync(w.counters, 0, 4 * sizeof(int), st); err != hipSuccess) return err;
  if (hipError_t err = hipMemcpyAsync(w.cursor, offsets, (size_t)nbuckets * sizeof(int), hipMemcpyDeviceToDevice, st);
      err != hipSuccess)
    return err;
  bucket_scatter_kernel<<<blocks_of(count, 256), 256, 0, st>>>(keys, count, nbuckets, w.cursor, perm);
  if (hipError_t err = hipGetLastError(); err != hipSuccess) return err;
  if (caps.wave == 0) return hipSuccess;               // (no bucket can hold two entries)
  bucket_classify_kernel<<<blocks_of(nbuckets, 256), 256, 0, st>>>(offsets, nbuckets, w, caps);
  if (hipError_t err = hipGetLastError(); err != hipSuccess) return err;
  sort_buckets_kernel<64, kWaveMax><<<(unsigned)(caps.wave < kWaveGrid ? caps.wave : kWaveGrid), 64, 0, st>>>(
      offsets, nbuckets, count, w.wave_list, w.counters + 1, caps.wave, perm);
  if (hipError_t err = hipGetLastError(); err != hipSuccess) return err;
  if (caps.block == 0) return hipSuccess;
  sort_buckets_kernel<kBlockThreads, kBlockMax><<<(unsigned)(caps.block < kBlockGrid ? caps.block : kBlockGrid), kBlockThreads, 0, st>>>(
      offsets, nbuckets, count, w.block_list, w.counters + 2, caps.block, perm);
  if (hipError_t err = hipGetLastError(); err != hipSuccess) return err;
  if (caps.lng == 0) return hipSuccess;
  sort_long_kernel<kLongThreads, kBlockMax><<<(unsigned)(caps.lng < kLongGrid ? caps.lng : kLongGrid), kLongThreads, 0, st>>>(
      offsets, nbuckets, count, w.long_list, w.counters + 3, caps.lng, perm);
  return hipGetLastError();
}

hipError_t launch_transpose_gather(const int* rowptr, int m, int nnz, const int* perm, const float* val, int* trow, float* tval,
                                   hipStream_t st) {
  transpose_gather_kernel<<<blocks_of(nnz, 256), 256, 0, st>>>(rowptr, m, nnz, perm, val, trow, tval);
  return hipGetLastError();
}

}  // namespace gcn
