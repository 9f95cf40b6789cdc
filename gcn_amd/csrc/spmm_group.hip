// spmm_group.hip — the sliced main pass as FOUR independent 16-lane row engines per wave.
//
// Why (profiles/r02c_pmc_quad_kernel_reddit_k128_S8.txt, Reddit-shaped k = 128, 8 slices): the four-per-gather kernel
// of spmm_quad.hip keeps one row per WAVE — its four 16-lane groups hold four interleaved partial sums of
// the same row — so every row end costs a cross-lane reduction, a scalar walk over the 64-entry block with
// per-lane masks, and scalar row-pointer loads.  With 8 column slices a virtual row is 62 entries long, so
// nearly every 64-entry block takes that slow path: 236 scalar and 189 vector instructions per block
// against 17 vector-memory instructions, the texture addresser busy 58 % of the time, and every further
// slice (shorter virtual rows) made it slower although the L2 misses halved.
//
// Here each 16-lane group (lane = g*16 + f, f = which float4 of the 64-column tile) walks its OWN chunk
// of the slice-major stream, one entry per step, and owns the complete sum of its current row:
//   * one global_load_dwordx4 still fetches four feature rows (4 x 256 B), one per group;
//   * a row end is a bit in the stream (bit 15 of the 16-bit entry) and costs the group ONE 256-byte write
//     under an EXEC mask — into its LDS ring, from where four consecutive rows leave with one 64-lane store
//     (spmm_group_ring_kernel), or straight to memory — no cross-lane reduction, no row pointers in the kernel;
//   * entries are 16 bits: the column's offset inside its slice (slices <= 32 767 columns); every virtual
//     row has at least one entry (empty ones get a padding entry that gathers the slice's all-zero row),
//     so "next row" is pointer arithmetic; runs of 64 entries are stored lane-major, so a lane fetches its
//     entries of four blocks with one 8-byte load;
//   * the byte offset of the gathered row is computed once per entry at load time (one lane = one entry
//     of its group's 16-entry block) and reaches the group by a DPP row broadcast fused into the address
//     add: per step one VALU op for the address, one load, two packed adds.
// Chunks are T entries of ONE group; a wave owns four consecutive chunks, a block sixteen, and the blocks
// of an XCD take consecutive chunks in dispatch order, so an XCD walks its part of the stream front to
// back and slices meet its L2 one after the other (with more chunks per wave, as before, the second
// chunk of an early wave ran beside the first chunk of a late one: two slices in one L2).
// A row cut by chunk ends leaves its first piece in Cv[row] and the pieces of the following chunks in the slab P (one
// head piece per chunk); the slice reduction adds them behind the row's slices, in chunk order (cut lists, slicing.hip;
// group_fixup_kernel does the same as a pass of its own where the reduction cannot): results are bitwise reproducible.
//
// Value-free (spmm_group_ring_kernel: every stored entry counts 1; the caller gathers from a copy of B whose rows
// were scaled by u_col and scales finished rows by u_row, api_spmm.cpp) or, for values that do not factor,
// with one fp32 value per entry beside the stream (spmm_group_weighted_kernel).
//
// The walk itself is group_walk.h: one template for this file's fp32 tables (RowF32, 64-column tiles) and the bf16 tables
// of spmm_group_bf16.hip (RowBf16, 128-column tiles).  This file holds the fp32 instantiations, the eight- and five-engine
// walks for narrow widths — chunk loops of their own around group_walk.h's chunk start (and, eight engines, row sink) —, the one choice of
// kernel (spmm_group_choice: the launch and the reported name ask it) and the one launch rule (group_grid,
// launch_spmm_group).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "spmm_kernels.h"
#include "group_walk.h"

namespace gcn {

// (the value-free walk WITHOUT the LDS ring — every finished row stored by its own group at once — was the r02 kernel; with
//  the ring 2.929 -> 2.874 ms, profiles/r02zt_*: only the ring variant is instantiated.  The weighted walk has none: it
//  sits at 126 VGPRs already and the ring bought nothing there, 3.184 -> 3.176 ms.)
template <bool BIG>
__global__ void __launch_bounds__(256)
spmm_group_ring_kernel(const unsigned short* __restrict__ stream, const int2* __restrict__ chunk_meta,
                       const float* __restrict__ Bp, float* __restrict__ Cv, float* __restrict__ P,
                       int nchunks, int T, int k, int seg_blocks, int ldb, int stream_nt, int blocks_per_tile, const int* __restrict__ dyn) {
  group_walk<RowF32, false, (GCN_ABLATE & 128) == 0, BIG>(stream, nullptr, chunk_meta, Bp, Cv, P, nchunks, T, k, seg_blocks, ldb, stream_nt, blocks_per_tile, dyn);
}

// the same walk for matrices whose values do not factor: one fp32 value per entry beside the 16-bit stream,
// handed from the lane that loaded it to its group by the same DPP broadcast as the address (one more vector
// instruction and four FMAs instead of two packed adds per step); Bp is then a plain (unscaled) sliced copy of B
template <bool BIG>
__global__ void __launch_bounds__(256)
spmm_group_weighted_kernel(const unsigned short* __restrict__ stream, const float* __restrict__ vals,
                           const int2* __restrict__ chunk_meta, const float* __restrict__ Bp, float* __restrict__ Cv,
                           float* __restrict__ P, int nchunks, int T, int k, int seg_blocks, int ldb, int stream_nt, int blocks_per_tile,
                           const int* __restrict__ dyn) {
  group_walk<RowF32, true, (GCN_ABLATE & 256) != 0, BIG>(stream, vals, chunk_meta, Bp, Cv, P, nchunks, T, k, seg_blocks, ldb, stream_nt, blocks_per_tile, dyn);
}

// (the eight- and five-engine walks below hold their partial rows as float4)
__device__ __forceinline__ void store_row_piece(float* dst, const float4& v) { store_row_piece(dst, f32x4{v.x, v.y, v.z, v.w}); }
__device__ __forceinline__ RowPieces<RowF32> row_pieces(const float4& v) { return RowPieces<RowF32>{{f32x4{v.x, v.y, v.z, v.w}}}; }

// ------------------------------------------------------------------------------------------------------------
// k <= 32: EIGHT independent 8-lane row engines per wave (lane = g*8 + f, f = which float4 of the 32-column tile).
// A gather instruction then fetches eight feature rows of 128 bytes instead of four of 256, so a non-zero costs half
// the addresser time of the 64-column pass it would otherwise ride in with half its lanes idle.  Same stream, same
// lane-major runs of 64 entries (a lane of an 8-lane group reads its entries of the run's eight 8-entry blocks as two
// 8-byte words: u16 4f.. and 32+4f..), same chunk_meta / partial slab / fix list; a wave owns eight consecutive
// chunks.  The DPP broadcasts still work on rows of 16 lanes = two groups: the upper group of a row takes its
// entry from a copy rotated by eight lanes.  Two 8-entry blocks are in flight together (sixteen gathers).
// Non-temporal stores; value-free (with the LDS ring: rows of 128 bytes, eight of one group leave together) or weighted.
__device__ __forceinline__ int row_ror8(int v) { return __builtin_amdgcn_mov_dpp(v, 0x128, 0xf, 0xf, true); }   // lane l <- lane (l + 8) % 16 of its row
template <int UU>
__device__ __forceinline__ int row_ror8_bcast(int v, int vrot, bool upper) {   // entry UU of THIS lane's 8-lane group
  const int lo = row_bcast<UU>(v), hi = row_bcast<UU>(vrot);
  return upper ? hi : lo;
}

template <bool RING, bool VALS, bool BIG>
__device__ __forceinline__ void
group8_walk(const unsigned short* __restrict__ stream, const float* __restrict__ vals, const int2* __restrict__ chunk_meta,
            const float* __restrict__ Bp, float* __restrict__ Cv, float* __restrict__ P,
            int nchunks, int T, int k, int ldb, int stream_nt, const int* __restrict__ dyn) {
  GroupChunk<RowF32, 8, 8, BIG> ch(Bp, nchunks, dyn, (int)blockIdx.x, 0, k, (size_t)k, ldb);
  if (ch.none()) return;
  ch.open(chunk_meta, Cv, P);
  RowSink<RowF32, 8, 8, RING> sink(ch, block_ring<RowF32, 8, 8, RING>());
  const int f = ch.f, base = ch.base;
  const bool upper = (ch.lane & 8) != 0;                        // the upper group of its 16-lane DPP row
  const unsigned row_bytes = ch.row_bytes, foff = ch.foff;
  const char* Bb = ch.Bb;

  const u32x2* __restrict__ sp = reinterpret_cast<const u32x2*>(stream + (size_t)ch.c * T);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  // words of the current run: w0 = entries of the even 8-entry blocks (0, 2, 4, 6), w1 = of the odd ones
  u32x2 w0 = stream_load(sp + f, stream_nt), w1 = stream_load(sp + 8 + f, stream_nt);
  u32x2 w0_nx = w0, w1_nx = w1;
  // VALS: the values of the same entries (slicing.hip lays them out like the stream): two 16-byte words per run
  const f32x4* __restrict__ vp = VALS ? reinterpret_cast<const f32x4*>(vals + (size_t)ch.c * T) : nullptr;
  f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
  if constexpr (VALS) { v0 = stream_load(vp + f, stream_nt); v1 = stream_load(vp + 8 + f, stream_nt); }
  f32x4 v0_nx = v0, v1_nx = v1;
  unsigned fl1 = 0;
#pragma unroll 1
  for (int d = 0; d < T / 16; ++d) {                            // two 8-entry blocks (2d, 2d+1 of the chunk) per turn
    const int j = d & 3;                                        // ... the j-th pair of the current run
    if (j == 0 && d + 4 < T / 16) {                             // the next run, a whole run ahead of its use
      const u32x2* nx = sp + (d / 4 + 1) * 16;
      w0_nx = stream_load(nx + f, stream_nt);
      w1_nx = stream_load(nx + 8 + f, stream_nt);
      if constexpr (VALS) {
        const f32x4* vnx = vp + (d / 4 + 1) * 16;
        v0_nx = stream_load(vnx + f, stream_nt);
        v1_nx = stream_load(vnx + 8 + f, stream_nt);
      }
    }
    const unsigned e0 = ((j & 2 ? w0.y : w0.x) >> (16 * (j & 1))) & 0xFFFFu;
    const unsigned e1 = ((j & 2 ? w1.y : w1.x) >> (16 * (j & 1))) & 0xFFFFu;
    int vb0 = 0, vb1 = 0, vb0r = 0, vb1r = 0;                   // this lane's entries' values (bit patterns) and their rotated copies
    if constexpr (VALS) {
      vb0 = __builtin_bit_cast(int, j == 0 ? v0.x : j == 1 ? v0.y : j == 2 ? v0.z : v0.w);
      vb1 = __builtin_bit_cast(int, j == 0 ? v1.x : j == 1 ? v1.y : j == 2 ? v1.z : v1.w);
      vb0r = row_ror8(vb0); vb1r = row_ror8(vb1);
    }
    if (j == 3) { w0 = w0_nx; w1 = w1_nx; v0 = v0_nx; v1 = v1_nx; }
    const int ro0 = (int)(__umul24((e0 & 0x7FFFu) + (unsigned)base, row_bytes));
    const int ro1 = (int)(__umul24((e1 & 0x7FFFu) + (unsigned)base, row_bytes));
    const int ro0r = row_ror8(ro0), ro1r = row_ror8(ro1);
    const unsigned fl0 = e0 >> 15;
    fl1 = e1 >> 15;
    const int fl0r = row_ror8((int)fl0), fl1r = row_ror8((int)fl1);
    float4 b[16];
#define GCN_G8_ALL(M) M(0) M(1) M(2) M(3) M(4) M(5) M(6) M(7)
#define GCN_G8_GATHER0(UU) \
    b[UU] = *reinterpret_cast<const float4*>(Bb + (size_t)((unsigned)row_ror8_bcast<UU>(ro0, ro0r, upper) + foff));
#define GCN_G8_GATHER1(UU) \
    b[8 + UU] = *reinterpret_cast<const float4*>(Bb + (size_t)((unsigned)row_ror8_bcast<UU>(ro1, ro1r, upper) + foff));
    GCN_G8_ALL(GCN_G8_GATHER0)
    GCN_G8_ALL(GCN_G8_GATHER1)
#undef GCN_G8_GATHER0
#undef GCN_G8_GATHER1
    const unsigned long long ends0 = __ballot(fl0 != 0);        // bit g*8+u: entry u of group g (first block) ends a row
    const unsigned long long ends1 = __ballot(fl1 != 0);
#define GCN_G8_ADDV(UU, I, VB, VBR)                                                                 \
      if constexpr (VALS) {                                                                         \
        const float vu = __builtin_bit_cast(float, row_ror8_bcast<UU>(VB, VBR, upper));             \
        acc.x = fmaf(vu, b[I].x, acc.x); acc.y = fmaf(vu, b[I].y, acc.y);                           \
        acc.z = fmaf(vu, b[I].z, acc.z); acc.w = fmaf(vu, b[I].w, acc.w);                           \
      } else { acc.x += b[I].x; acc.y += b[I].y; acc.z += b[I].z; acc.w += b[I].w; }
#define GCN_G8_ADD0(UU) GCN_G8_ADDV(UU, UU, vb0, vb0r)
#define GCN_G8_ADD1(UU) GCN_G8_ADDV(UU, 8 + UU, vb1, vb1r)
    if ((ends0 | ends1) == 0ull) {
      GCN_G8_ALL(GCN_G8_ADD0)
      GCN_G8_ALL(GCN_G8_ADD1)
    } else {
#define GCN_G8_STEP(UU, I, ENDS, FL, FLR, VB, VBR)                                                  \
      GCN_G8_ADDV(UU, I, VB, VBR)                                                                   \
      if (ENDS & (group_bits<8, 8>() << UU)) {                   /* some group ends a row here */    \
        if (row_ror8_bcast<UU>((int)FL, FLR, upper)) { sink.finish(row_pieces(acc)); acc = make_float4(0.f, 0.f, 0.f, 0.f); } \
      }
#define GCN_G8_STEP0(UU) GCN_G8_STEP(UU, UU, ends0, fl0, fl0r, vb0, vb0r)
#define GCN_G8_STEP1(UU) GCN_G8_STEP(UU, 8 + UU, ends1, fl1, fl1r, vb1, vb1r)
      GCN_G8_ALL(GCN_G8_STEP0)
      GCN_G8_ALL(GCN_G8_STEP1)
#undef GCN_G8_STEP0
#undef GCN_G8_STEP1
#undef GCN_G8_STEP
      sink.drain_full();
    }
#undef GCN_G8_ADD1
#undef GCN_G8_ADD0
#undef GCN_G8_ADDV
#undef GCN_G8_ALL
  }
  sink.drain_rest();
  // (the chunk's last entry is entry 7 of its last block)
  sink.tail(!row_ror8_bcast<7>((int)fl1, row_ror8((int)fl1), upper), row_pieces(acc));
}

template <bool RING, bool BIG>
__global__ void __launch_bounds__(256)
spmm_group8_kernel(const unsigned short* __restrict__ stream, const int2* __restrict__ chunk_meta,
                   const float* __restrict__ Bp, float* __restrict__ Cv, float* __restrict__ P,
                   int nchunks, int T, int k, int ldb, int stream_nt, const int* __restrict__ dyn) {
  group8_walk<RING, false, BIG>(stream, nullptr, chunk_meta, Bp, Cv, P, nchunks, T, k, ldb, stream_nt, dyn);
}

// ... and with the values beside the stream (matrices whose values do not factor); no ring: 138 VGPRs without
template <bool BIG>
__global__ void __launch_bounds__(256)
spmm_group8_weighted_kernel(const unsigned short* __restrict__ stream, const float* __restrict__ vals,
                            const int2* __restrict__ chunk_meta, const float* __restrict__ Bp, float* __restrict__ Cv,
                            float* __restrict__ P, int nchunks, int T, int k, int ldb, int stream_nt, const int* __restrict__ dyn) {
  group8_walk<false, true, BIG>(stream, vals, chunk_meta, Bp, Cv, P, nchunks, T, k, ldb, stream_nt, dyn);
}

// ------------------------------------------------------------------------------------------------------------
// 33 <= k <= 48: FIVE 12-lane row engines per wave (lane = g*12 + f, f = which float4 of the 48-column row; lanes 60..63
// idle).  The addressers charge a gather instruction for its 64 lane addresses whatever they fetch (gather_x3_probe), so
// a row of 192 bytes occupies 12 lanes here, not 16 with four of them idle: five rows per instruction instead of four.
// (Worth 4-7 % of the whole SpMM, not the 20 % the instruction count suggests: a 192-byte row still arrives as two
// whole 128-byte lines, and at 64 B/clk per CU five rows of two lines cost the L2 -> L1 path 20 clocks where four cost
// 16 — with 16 lanes x 16 bytes the address rate and the line rate bind together)
// SAME stream as the 16-lane kernel (blocks of 16 entries, runs of 64 stored lane-major): lane f < 12 holds entry f of
// its group's block, lanes f < 4 hold entries 12..15 as well (a second 8-byte word per run); an entry reaches the
// group's lanes through ds_bpermute (a DPP row is 16 lanes wide and would straddle the groups).  Row ends: two ballots
// (entries 0..11 and 12..15).  Same chunk_meta, partial slab, cut lists and pieces; a wave owns five consecutive
// chunks, a block twenty (GroupChunk: the groups that are not live).  Value-free pass, 32-bit slice bases, LDS ring of
// five rows per group (one 60-lane store).
__device__ __forceinline__ int lane_bcast(int src_lane_bytes, int v) { return __builtin_amdgcn_ds_bpermute(src_lane_bytes, v); }

__device__ __forceinline__ void
group12_walk(const unsigned short* __restrict__ stream, const int2* __restrict__ chunk_meta,
             const float* __restrict__ Bp, float* __restrict__ Cv, float* __restrict__ P,
             int nchunks, int T, int k, int ldb, int stream_nt, const int* __restrict__ dyn) {
  GroupChunk<RowF32, 5, 12, false> ch(Bp, nchunks, dyn, (int)blockIdx.x, 0, k, (size_t)k, ldb);
  if (ch.none()) return;
  ch.open(chunk_meta, Cv, P);
  const int lane = ch.lane, wib = ch.wib, g = ch.g, f = ch.f, fcol = ch.fcol, base = ch.base, c = ch.c;
  const bool live = ch.live, fok = live && ch.col_ok, head = ch.head;
  const unsigned row_bytes = ch.row_bytes, foff = ch.foff;
  const char* Bb = ch.Bb;
  const size_t kk = ch.kk;
  float *ptr = ch.ptr, *nptr = ch.nptr;
  bool first = true;
  // The ring, its drains and the row ends stay this walk's own text, and the stream words are loaded and decoded in place:
  // on RowSink, or with stream_load, the compiler allocates this kernel differently (126 to 137 VGPRs
  // against 135, three or four waves) and its chunk loop is no longer the one that was measured — DESIGN §4.17.
  __shared__ f32x4 ring[4][5][5][12];                           // [wave][group][slot][float4 of the row]
  int ring_n = 0;
  float* ring_base = nullptr;
  const int row_l = lane / 12;                                  // which ring row this lane writes out in a drain (== g)
#define GCN_G12_DRAIN(G2, ROWS)                                                                     \
  {                                                                                                 \
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(uintptr_t)ring_base, 12 * G2);    \
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)((uintptr_t)ring_base >> 32), 12 * G2); \
    float* b0 = reinterpret_cast<float*>(((uintptr_t)hi << 32) | lo);                              \
    if (row_l < (ROWS) && fcol < k) {                                                               \
      const f32x4 rv = ring[wib][G2][row_l][f];                                                     \
      store_row_piece(b0 + (size_t)row_l * kk + fcol, make_float4(rv.x, rv.y, rv.z, rv.w));         \
    }                                                                                               \
    if (g == G2) ring_n = 0;                                                                        \
  }

  const u32x2* __restrict__ sp = reinterpret_cast<const u32x2*>(stream + (size_t)c * T);
  const int f2 = f < 4 ? 12 + f : f;                            // the second word of lanes 0..3: entries 12..15 (others: a copy)
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  u32x2 eq = stream_nt ? __builtin_nontemporal_load(sp + f) : sp[f], eq_nx = eq;
  u32x2 eq2 = stream_nt ? __builtin_nontemporal_load(sp + f2) : sp[f2], eq2_nx = eq2;
  const int srcA = g * 48;                                      // byte index of the group's lane 0 (ds_bpermute counts bytes)
  unsigned long long endsA = 0ull, endsB = 0ull;
#pragma unroll 1
  for (int blk = 0; blk < T / 16; ++blk) {
    const int j = blk & 3;
    if (j == 0 && blk + 4 < T / 16) {
      const int nx = (blk / 4 + 1) * 16;
      eq_nx = stream_nt ? __builtin_nontemporal_load(sp + nx + f) : sp[nx + f];
      eq2_nx = stream_nt ? __builtin_nontemporal_load(sp + nx + f2) : sp[nx + f2];
    }
    const unsigned e  = ((j & 2 ? eq.y : eq.x) >> (16 * (j & 1))) & 0xFFFFu;
    const unsigned e2 = ((j & 2 ? eq2.y : eq2.x) >> (16 * (j & 1))) & 0xFFFFu;
    if (j == 3) { eq = eq_nx; eq2 = eq2_nx; }
    const int rowoff  = (int)(__umul24((e & 0x7FFFu) + (unsigned)base, row_bytes));
    const int rowoff2 = (int)(__umul24((e2 & 0x7FFFu) + (unsigned)base, row_bytes));
    float4 b[16];
#define GCN_G12_ALL(M) M(0) M(1) M(2) M(3) M(4) M(5) M(6) M(7) M(8) M(9) M(10) M(11) M(12) M(13) M(14) M(15)
#define GCN_G12_GATHER(UU) \
    b[UU] = *reinterpret_cast<const float4*>(Bb + (size_t)((unsigned)lane_bcast(srcA + 4 * (UU < 12 ? UU : UU - 12), UU < 12 ? rowoff : rowoff2) + foff));
    GCN_G12_ALL(GCN_G12_GATHER)
#undef GCN_G12_GATHER
    endsA = __ballot((e >> 15) != 0);                           // bit g*12+u: entry u < 12 of group g ends a row
    endsB = __ballot((e2 >> 15) != 0 && f < 4);                 // bit g*12+u-12: entry u >= 12
    if ((endsA | endsB) == 0ull) {
#define GCN_G12_ADD(UU) acc.x += b[UU].x; acc.y += b[UU].y; acc.z += b[UU].z; acc.w += b[UU].w;
      GCN_G12_ALL(GCN_G12_ADD)
    } else {
      const unsigned long long mineA = endsA >> (g < 5 ? g * 12 : 60);    // this lane's group's bits at 0..11
      const unsigned long long mineB = endsB >> (g < 5 ? g * 12 : 60);    // ... entries 12..15 at 0..3
#define GCN_G12_STEP(UU)                                                                            \
      GCN_G12_ADD(UU)                                                                               \
      if ((UU < 12 ? endsA : endsB) & (group_bits<5, 12>() << (UU < 12 ? UU : UU - 12))) {        \
        if (((UU < 12 ? mineA : mineB) >> (UU < 12 ? UU : UU - 12)) & 1ull) {                       \
          if (!(first && head) && ring_n < 5) {                                                     \
            if (fok) ring[wib][g < 5 ? g : 0][ring_n][f] = f32x4{acc.x, acc.y, acc.z, acc.w};       \
            if (ring_n == 0) ring_base = ptr;                                                       \
            ++ring_n;                                                                               \
          } else if (fok) store_row_piece(ptr, acc);                                                \
          acc = make_float4(0.f, 0.f, 0.f, 0.f);                                                    \
          ptr = nptr; nptr += kk; first = false;                                                    \
        }                                                                                           \
      }
      GCN_G12_ALL(GCN_G12_STEP)
#undef GCN_G12_STEP
#undef GCN_G12_ADD
      const unsigned long long full = __ballot(ring_n == 5 && live);
      if (full) {
        if (full & (1ull << 0))  GCN_G12_DRAIN(0, 5)
        if (full & (1ull << 12)) GCN_G12_DRAIN(1, 5)
        if (full & (1ull << 24)) GCN_G12_DRAIN(2, 5)
        if (full & (1ull << 36)) GCN_G12_DRAIN(3, 5)
        if (full & (1ull << 48)) GCN_G12_DRAIN(4, 5)
      }
    }
#undef GCN_G12_ALL
  }
  {
    const unsigned long long some = __ballot(ring_n > 0 && live);
    if (some & (1ull << 0))  GCN_G12_DRAIN(0, __builtin_amdgcn_readlane(ring_n, 0))
    if (some & (1ull << 12)) GCN_G12_DRAIN(1, __builtin_amdgcn_readlane(ring_n, 12))
    if (some & (1ull << 24)) GCN_G12_DRAIN(2, __builtin_amdgcn_readlane(ring_n, 24))
    if (some & (1ull << 36)) GCN_G12_DRAIN(3, __builtin_amdgcn_readlane(ring_n, 36))
    if (some & (1ull << 48)) GCN_G12_DRAIN(4, __builtin_amdgcn_readlane(ring_n, 48))
  }
#undef GCN_G12_DRAIN
  // the row piece that sticks out of the chunk's end: the chunk's last entry is entry 15 of its last block (lane 3's second word)
  if (!((endsB >> (g < 5 ? g * 12 + 3 : 63)) & 1ull)) {
    if (fok) store_row_piece(ptr, acc);
  }
}

__global__ void __launch_bounds__(256)
spmm_group12_kernel(const unsigned short* __restrict__ stream, const int2* __restrict__ chunk_meta,
                    const float* __restrict__ Bp, float* __restrict__ Cv, float* __restrict__ P,
                    int nchunks, int T, int k, int ldb, int stream_nt, const int* __restrict__ dyn) {
  group12_walk(stream, chunk_meta, Bp, Cv, P, nchunks, T, k, ldb, stream_nt, dyn);
}

// 32-bit byte offsets (entry + slice base) * row_bytes reach every row of the sliced table?  (__umul24: both factors
// below 2^24, and the product below 2^32.)  Otherwise the BIG variants add the slice base in 64 bits.
bool spmm_group_needs_big(long long table_rows, long long row_bytes) {
  // GCN_AMD_GROUP_BIG=1 (development / tests): the 64-bit variants whatever the size
  static const bool forced = [] { const char* e = getenv("GCN_AMD_GROUP_BIG"); return e && e[0] == '1'; }();
  return forced || table_rows >= (1LL << 24) || table_rows * row_bytes >= (1LL << 32);
}

// table_rows = rows of the sliced copy the kernel gathers from, S * (w + 1) (0: unknown / not checked)
bool spmm_group_eligible(int k, int ldb, long long table_rows, const void* B, const void* C, const void* P) {
  const uintptr_t al = (uintptr_t)B | (uintptr_t)C | (uintptr_t)P;
  if (ldb <= 0) ldb = k;
  if (!(k % 4 == 0 && ldb % 4 == 0 && (al & 15) == 0 && ldb * 4 < (1 << 24))) return false;
  // BIG: the offset inside a slice (< 32 768 rows) must still fit 32 bits
  return !spmm_group_needs_big(table_rows, ldb * 4LL) || ldb * 4 < (1 << 17);
}

// development switches, each read once per process: GCN_AMD_GROUP8=0 keeps k <= 32, GCN_AMD_GROUP12=0 keeps 33..48 on the
// 64-column pass.  The first reaches the choice as GroupArgs::narrow8 (the drop-in flexspmm leaves the default).
static bool knob_on(const char* name) { const char* e = getenv(name); return !e || e[0] != '0'; }
static bool group12_enabled() { static const bool on = knob_on("GCN_AMD_GROUP12"); return on; }
bool group8_enabled() { static const bool on = knob_on("GCN_AMD_GROUP8"); return on; }

// THE rule for which kernel a launch runs (the launch switches on it, the plan API reports from it): eight engines for
// fp32, k <= 32 and whole waves of eight chunks per XCD; five for fp32, 33 <= k <= 48, value-free, 32-bit slice bases
GroupChoice spmm_group_choice(const GroupArgs& a) {
  const int ld = a.ldb > 0 ? a.ldb : a.k;
  GroupChoice c;
  c.bf16 = a.elem_bytes == 2;
  c.weighted = a.vals != nullptr;
  c.big = spmm_group_needs_big(a.table_rows, (long long)ld * a.elem_bytes);
  c.engine = GroupEngine::four16;
  if (!c.bf16 && a.k % 4 == 0) {
    if (a.narrow8 && a.k <= 32 && a.nchunks % 64 == 0) c.engine = GroupEngine::eight8;
    else if (group12_enabled() && a.narrow12 && !c.weighted && a.k > 32 && a.k <= 48 && !c.big) c.engine = GroupEngine::five12;
  }
  return c;
}

// the kernel's name as a profile shows it
void spmm_group_kernel_name(const GroupChoice& c, char* buf, size_t len) {
  const char* big = c.big ? "true" : "false";
  if (!c.bf16 && c.engine == GroupEngine::five12) { snprintf(buf, len, "gcn::spmm_group12_kernel"); return; }
  if (c.bf16) snprintf(buf, len, c.weighted ? "gcn::spmm_group_bf16_weighted_kernel<%s>" : "gcn::spmm_group_bf16_kernel<%s>", big);
  else if (c.engine == GroupEngine::eight8) snprintf(buf, len, c.weighted ? "gcn::spmm_group8_weighted_kernel<%s>" : "gcn::spmm_group8_kernel<true, %s>", big);
  else snprintf(buf, len, c.weighted ? "gcn::spmm_group_weighted_kernel<%s>" : "gcn::spmm_group_ring_kernel<%s>", big);
}

namespace {

// The launch rule of every group kernel: GROUPS engines per wave (a block walks 4 * GROUPS chunks) on column tiles of
// tile_cols (the eight- and five-engine kernels have one tile, and no order to pick).
hipError_t group_grid(const GroupArgs& a, int tile_cols, int groups, GroupGrid* g) {
  const int per_xcd = a.nchunks / 8, per_block = 4 * groups;
  g->blocks_per_tile = 8 * ((per_xcd + per_block - 1) / per_block);
  const int tiles = (a.k + tile_cols - 1) / tile_cols;
  // all tiles in ONE launch: tile t+1 starts on the CUs that tile t's last blocks leave idle (k = 128 / 256: 2.89 / 5.70 ->
  // 2.87 / 5.66 ms, profiles/r02zzb_merged_tile_launch.log)
  if ((long long)g->blocks_per_tile * tiles >= (1LL << 31)) return hipErrorInvalidValue;
  g->nblocks = g->blocks_per_tile * tiles;
  // streams (2 bytes per entry, 6 with values) beyond what the L2s and a good part of the Infinity Cache hold are read
  // non-temporally (group_walk.h has the measurement)
  const size_t stream_bytes = (size_t)a.nchunks * (size_t)a.T * (a.vals ? 6u : 2u);
  g->stream_nt = stream_bytes > ((size_t)64 << 20) ? 1 : 0;
  // Order of the (tile, block) pairs inside the launch (r04).  Tile-major — all of tile 0, then all of tile 1 — reads the
  // whole stream once per tile from HBM: by the time tile 1 starts, tile 0's stream has long left the 256 MiB Infinity
  // Cache.  In SEGMENTS — every XCD's blocks cut into nseg runs, run 0 for tile 0, run 0 for tile 1, ..., then run 1 — a
  // run's stream is read again while it still sits there.  The price is a switch of the XCD's L2-resident table slice at
  // every run, so as few runs as keep one run's stream (all XCDs together) near half the cache:
  // nseg = ceil(stream bytes / 120 MB); measured (profiles/r04k_*, r04l_*; Reddit-shaped, whole fp32 SpMM): value-free (230 MB)
  // k = 128: 2.845 -> 2.680 ms at 2 runs (3 / 5 / 8 / 12 runs: 2.73 / 2.75 / 2.82 / 2.92), k = 512: 11.52 -> 10.89;
  // weighted (689 MB) k = 128: 3.135 -> 3.043 at 6 runs (2 / 8: 3.19 / 3.08); half-size graph: value-free (57 MB) stays
  // tile-major, weighted (172 MB) 1.452 -> 1.382 at 2.  GCN_AMD_GROUP_SEGMENTS (development) overrides nseg; 1 = tile-major.
  static const int forced_seg = [] { const char* e = getenv("GCN_AMD_GROUP_SEGMENTS"); return e ? atoi(e) : 0; }();
  const size_t seg_bytes = (size_t)120 << 20;
  const int nseg = forced_seg > 0 ? forced_seg : (int)((stream_bytes + seg_bytes - 1) / seg_bytes);
  const int nbx = g->blocks_per_tile / 8;
  g->seg_blocks = (nseg > 1 && tiles > 1 && nbx > 1) ? (nbx + nseg - 1) / nseg : 0;                // 0: tile-major
  return hipSuccess;
}

template <bool BIG>
hipError_t launch_group_f32(const GroupArgs& a, const GroupChoice& c, int ldb, const GroupGrid& g, hipStream_t s) {
  const int2* meta = reinterpret_cast<const int2*>(a.chunk_meta);
  const float* Bp = static_cast<const float*>(a.Bp);
  const dim3 grid(g.nblocks), block(256);
  if (c.engine == GroupEngine::five12) {
    if constexpr (BIG) return hipErrorInvalidValue;             // (spmm_group_choice: 32-bit slice bases only)
    else spmm_group12_kernel<<<grid, block, 0, s>>>(a.stream, meta, Bp, a.Cv, a.P, a.nchunks, a.T, a.k, ldb, g.stream_nt, a.dyn);
  } else if (c.engine == GroupEngine::eight8) {
    if (c.weighted) spmm_group8_weighted_kernel<BIG><<<grid, block, 0, s>>>(a.stream, a.vals, meta, Bp, a.Cv, a.P, a.nchunks, a.T, a.k, ldb, g.stream_nt, a.dyn);
    else            spmm_group8_kernel<true, BIG><<<grid, block, 0, s>>>(a.stream, meta, Bp, a.Cv, a.P, a.nchunks, a.T, a.k, ldb, g.stream_nt, a.dyn);
  } else {
    if (c.weighted) spmm_group_weighted_kernel<BIG><<<grid, block, 0, s>>>(a.stream, a.vals, meta, Bp, a.Cv, a.P, a.nchunks, a.T, a.k, g.seg_blocks, ldb, g.stream_nt, g.blocks_per_tile, a.dyn);
    else            spmm_group_ring_kernel<BIG><<<grid, block, 0, s>>>(a.stream, meta, Bp, a.Cv, a.P, a.nchunks, a.T, a.k, g.seg_blocks, ldb, g.stream_nt, g.blocks_per_tile, a.dyn);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_spmm_group(const GroupArgs& a, hipStream_t s) {
  if (a.nchunks <= 0 || a.k <= 0) return hipSuccess;
  if (a.elem_bytes != 4 && a.elem_bytes != 2) return hipErrorInvalidValue;
  const int lane_cols = 16 / a.elem_bytes;                            // columns in the 16 bytes a lane gathers
  if (a.nchunks % 32 != 0 || a.k % lane_cols != 0 || a.T < 64 || a.T % 64 != 0) return hipErrorInvalidValue;
  const int ld = a.ldb > 0 ? a.ldb : a.k;
  if (ld % lane_cols != 0 || ld < a.k || ((uintptr_t)a.Bp & 15) != 0) return hipErrorInvalidValue;
  if (a.table_rows <= 0) return hipErrorInvalidValue;                 // (the addressing mode depends on it)
  const GroupChoice c = spmm_group_choice(a);
  if (c.big && (long long)ld * a.elem_bytes >= (1 << 17)) return hipErrorInvalidValue;   // (the offset inside a slice must still fit 32 bits)
  const int groups    = c.engine == GroupEngine::eight8 ? 8 : c.engine == GroupEngine::five12 ? 5 : 4;
  const int tile_cols = c.engine == GroupEngine::eight8 ? 32 : c.engine == GroupEngine::five12 ? 48 : c.bf16 ? 128 : 64;
  GroupGrid g;
  if (const hipError_t e = group_grid(a, tile_cols, groups, &g); e != hipSuccess) return e;
  if (c.bf16) return a.dyn ? hipErrorInvalidValue : launch_group_walk_bf16(a, ld, g, c.big, s);   // (no bf16 drop-in path)
  return c.big ? launch_group_f32<true>(a, c, ld, g, s) : launch_group_f32<false>(a, c, ld, g, s);
}

}  // namespace gcn
