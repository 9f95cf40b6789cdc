// group_walk.h — the walk of the group kernels (four independent 16-lane row engines per wave on the 15-bit slice-major
// stream; spmm_group.hip says why and how), written once for both table formats.  A row format says what the 16 bytes one
// lane gathers mean — RowF32: 4 fp32 columns of a 64-column tile; RowBf16: 8 bf16 columns of a 128-column tile, widened by
// shift / mask (a bf16 is the top half of an fp32) — everything else is the same code: the (tile, block) order inside the
// merged launch, the lane-major stream with the value words a run ahead, the DPP broadcast of the row offset, the row-end
// ballot.  What stands around the chunk loop — the chunk assignment per XCD, the chunk_meta decode and BIG (GroupChunk),
// the LDS ring with its drains and the piece that sticks out of a chunk (RowSink) — is written for an engine geometry:
// GroupChunk serves the eight- and five-engine walks of spmm_group.hip as well, RowSink the eight-engine one.  Every sum
// is fp32; partial rows go to the fp32 slab Cv / P whatever the table holds.
// Device code only: included by spmm_group.hip (fp32 instantiations) and spmm_group_bf16.hip (bf16 instantiations).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gcn {

// value held by lane UU of this lane's 16-lane row (DPP row_newbcast)
template <int UU>
__device__ __forceinline__ int row_bcast(int v) {
  return __builtin_amdgcn_mov_dpp(v, 0x150 + UU, 0xf, 0xf, true);
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// Partial-row store, GCN_STORE_POLICY: 0 plain, 1 sc1 (write-through), 2 nt (streaming; the default and the only one a
// release build holds).  The slab of partial rows is read back only by the reduction that follows; left in L2 its lines
// push out feature rows the gathers are about to reuse.  Measured (profiles/r02z2_row_end_store_ablation.log,
// r02z4_store_policy.log, Reddit-shaped k = 128): with the store instruction alone removed the main passes run 2.69 ms at
// 8 slices and 2.22 ms at 16 — the whole cost of a row end is its store; sc1 stores cost 2.86 / 2.74 / 2.76 ms (8 / 12 /
// 16 slices), plain ones 2.86 / 2.75 / 2.71, nt ones 2.82 / 2.66 / 2.53.  tools/probes/store_probe.hip shows why: beside
// L2-served gathers an sc1 store holds the vector-memory path ~30 cycles per instruction, a plain or nt one ~5, and only
// sc1 and nt keep the written lines from displacing the table.  (There is no builtin for a 16-byte sc1 store; the
// trailing s_nop keeps the compiler's next instruction off the data registers until the store has read them,
// cdna_hip_programming.md §5.7.)
// GCN_ABLATE (development builds only, tools/ablate_group.sh: wrong results, exact costs): bit 0 no partial-row stores,
// bit 1 no row-end handling, bit 2 no stream loads after the first run (value-free: every load reads the chunk's first
// run), bit 3 partial rows at a stride of one tile;
// weighted walk (r04): bit 4 the value stream read from its first 4 KiB only (cache-resident: its bytes without its
// traffic), bit 5 no value broadcast (every lane multiplies by its OWN entry's value), bit 6 adds instead of FMAs — these
// seven act on both row formats; bit 7 the value-free walk WITHOUT the LDS ring, bit 8 the weighted walk WITH it (these
// two give right results) are read where the fp32 kernels name their walk: fp32 only.
#ifndef GCN_ABLATE
#define GCN_ABLATE 0
#endif
#ifndef GCN_STORE_POLICY
#define GCN_STORE_POLICY 2
#endif
__device__ __forceinline__ void store_row_piece(float* dst, const f32x4& t) {
  if constexpr ((GCN_ABLATE & 1) != 0) { asm volatile("" : : "v"(t.x), "v"(t.y), "v"(t.z), "v"(t.w)); return; }
  if constexpr (GCN_STORE_POLICY == 1) {
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(dst), "v"(t) : "memory");
  } else if constexpr (GCN_STORE_POLICY == 2) {
    __builtin_nontemporal_store(t, reinterpret_cast<f32x4*>(dst));
  } else {
    *reinterpret_cast<f32x4*>(dst) = t;
  }
}

// A lane's share of a row is four accumulator units (Unit: what one add handles — an fp32, or a pair for the packed
// instructions) and leaves as kPieces 16-byte pieces (piece i: columns 4i .. 4i + 3 of the share).
// kStage: runs of 64 entries whose stream words the value-free walk fetches together (group_walk below).  fp32: 8, a whole
// chunk at the default T = 512 (124 VGPRs against 112 with the next run alone, four waves per SIMD either way).  bf16: 8
// would take 136 VGPRs and the fourth wave, 4 takes 128 and keeps it — Reddit-shaped, whole SpMM, k = 128 / 256: fp32
// 2.68 -> 2.51 / 5.47 -> 5.17 ms at 8 (2.54 / 5.22 at 4); bf16 1.80 -> 1.67 / 3.50 -> 3.37 at 4 (1.68 / 3.42 at 8):
// profiles/stream_stage_measure.log, registers in profiles/stream_stage_registers.log.  (GCN_GROUP_STAGE, development
// builds: one length for both.)
#ifdef GCN_GROUP_STAGE
#define GCN_ROW_STAGE(N) GCN_GROUP_STAGE
#else
#define GCN_ROW_STAGE(N) N
#endif
struct RowF32 {
  typedef float Unit;
  static constexpr int kLaneCols = 4, kTileCols = 64, kElemBytes = 4, kPieces = 1, kStage = GCN_ROW_STAGE(8);
  static __device__ __forceinline__ void widen(const uint4& raw, Unit (&w)[4]) {
    w[0] = __uint_as_float(raw.x); w[1] = __uint_as_float(raw.y); w[2] = __uint_as_float(raw.z); w[3] = __uint_as_float(raw.w);
  }
  static __device__ __forceinline__ f32x4 piece(const Unit (&a)[4], int) { return f32x4{a[0], a[1], a[2], a[3]}; }
};
struct RowBf16 {
  typedef f32x2 Unit;
  static constexpr int kLaneCols = 8, kTileCols = 128, kElemBytes = 2, kPieces = 2, kStage = GCN_ROW_STAGE(4);
  static __device__ __forceinline__ Unit pair(unsigned word) {    // columns 2i and 2i + 1 of a word
    return Unit{__uint_as_float(word << 16), __uint_as_float(word & 0xFFFF0000u)};
  }
  static __device__ __forceinline__ void widen(const uint4& raw, Unit (&w)[4]) {
    w[0] = pair(raw.x); w[1] = pair(raw.y); w[2] = pair(raw.z); w[3] = pair(raw.w);
  }
  static __device__ __forceinline__ f32x4 piece(const Unit (&a)[4], int i) {
    return f32x4{a[2 * i].x, a[2 * i].y, a[2 * i + 1].x, a[2 * i + 1].y};
  }
};
template <class Row> struct RowPieces { f32x4 p[Row::kPieces]; };   // what a store or a ring slot takes

template <class Row>
__device__ __forceinline__ RowPieces<Row> row_pieces(const typename Row::Unit (&acc)[4]) {
  RowPieces<Row> r;
#pragma unroll
  for (int i = 0; i < Row::kPieces; ++i) r.p[i] = Row::piece(acc, i);
  return r;
}

template <class Row>
__device__ __forceinline__ void store_row_pieces(float* dst, const RowPieces<Row>& r) {
#pragma unroll
  for (int i = 0; i < Row::kPieces; ++i) store_row_piece(dst + 4 * i, r.p[i]);
}

// One launch covers every column tile: blocks [t*blocks_per_tile, (t+1)*blocks_per_tile) walk the whole stream for tile
// t.  Blocks are dispatched in index order, so the next tile starts on the CUs the previous one's last blocks leave idle
// (blocks_per_tile % 8 == 0: a block's XCD is blockIdx % 8 either way).  Order of the (tile, block) pairs (group_grid,
// spmm_group.hip, says why).  seg_blocks == 0: tile-major.  seg_blocks = Q > 0: every XCD's blocks in runs of Q — run 0
// for tile 0, run 0 for tile 1, ..., then run 1.  Placement only: the result is the same.
struct TileBlock { int col_tile, bx; };
template <int TILE_COLS>
__device__ __forceinline__ TileBlock group_tile_block(int block, int blocks_per_tile, int seg_blocks, int k) {
  TileBlock tb;
  if (seg_blocks > 0) {
    const int Q = seg_blocks, nbx = blocks_per_tile >> 3, tiles = (k + TILE_COLS - 1) >> __builtin_ctz(TILE_COLS);
    const int x = block & 7, i = block >> 3;
    const int nseg = (nbx + Q - 1) / Q, full = (nseg - 1) * tiles * Q;
    int j;
    if (i < full) { const int seg = i / (tiles * Q), r = i - seg * tiles * Q; tb.col_tile = r / Q; j = seg * Q + (r - tb.col_tile * Q); }
    else { const int last = nbx - (nseg - 1) * Q, r = i - full; tb.col_tile = r / last; j = (nseg - 1) * Q + (r - tb.col_tile * last); }
    tb.bx = j * 8 + x;
  } else {
    tb.col_tile = block / blocks_per_tile;
    tb.bx = block - tb.col_tile * blocks_per_tile;
  }
  return tb;
}

// stream  [nchunks*T] u16: bits 0..14 column offset inside the slice (== slice width: the all-zero row),
//                          bit 15 = last entry of its virtual row; every run of 64 entries stored lane-major (group_phys)
// chunk_meta [nchunks]: {2 * (virtual row holding entry c*T) + (that row began in an earlier chunk), first row of
// the chunk's slice in the table}
// table: slice s at rows [s*(w+1), (s+1)*(w+1)), row w of every slice all zero, rows ld elements apart (fp32: the copy
// of B scaled by u_col; bf16: bf16(u_col[c] * B[c, :]), one RNE rounding; weighted passes: B itself)
// Cv / P: fp32, rows k floats apart.  k % Row::kLaneCols == 0: a lane's columns are all in or all out.
// nchunks % 32 == 0 (the stream is padded), so every XCD owns whole waves.
// vals (VALS only) [nchunks*T]: the matrix values in stream order, 0 at padding entries
// BIG: the table is 4 GiB or more (or has 2^24 rows or more): the slice's first row is added to the table pointer in 64
// bits, per lane, and only the offset INSIDE the slice (< 32 768 rows x < 128 KiB) stays in 32 bits — one more vector
// instruction per gather (add + carry instead of one add).  Without it the 32-bit byte offset (entry + base) * row_bytes
// would wrap silently.

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// bit u of every group's LANES bits of a ballot, at u = 0
template <int GROUPS, int LANES>
constexpr unsigned long long group_bits() {
  unsigned long long m = 0;
  for (int g = 0; g < GROUPS; ++g) m |= 1ull << (g * LANES);
  return m;
}
// stream_nt (streams too large to stay cached from one SpMM to the next, group_grid): non-temporal loads
// keep them from displacing the table — 2.94 -> 2.87 ms per SpMM on the 232 MB stream of the Reddit-shaped
// graph (profiles/r02zn_*); a stream that fits the caches is better left there (profiles/r02zo_*)
template <class V>
__device__ __forceinline__ V stream_load(const V* p, int stream_nt) { return stream_nt ? __builtin_nontemporal_load(p) : *p; }
// Where this lane's group starts: its chunk, the lane's columns, what the chunk's meta word says.  A wave owns GROUPS
// consecutive chunks of its XCD's range, a block 4 * GROUPS.  GROUPS * LANES == 64: the range is whole waves (the stream's
// padding; spmm_group_choice for eight).  Fewer lanes: the groups past the range and the spare lanes walk the wave's
// first chunk along (loads only) and store nothing — live says which.  Use: construct (arithmetic only), leave if none(),
// then open() reads the meta word — two steps, because behind a returned flag the compiler closes the divergent region and
// opens it again, and the stream's first loads wait for the meta word.
template <class Row, int GROUPS, int LANES, bool BIG>
struct GroupChunk {
  static constexpr bool kWholeWaves = GROUPS * LANES == 64;
  int lane, wib, g, f;            // f: which 16 bytes of the tile's row this lane gathers
  int per_xcd, c_w, c, fcol;      // chunks of an XCD; the wave's first chunk inside that range; the chunk; the lane's first column
  bool live, col_ok, head;        // col_ok: the lane's columns exist; head: the chunk's first row began in an earlier chunk
  unsigned row_bytes, foff;       // foff: byte offset of the lane's columns in a table row
  int base;                       // first row of the chunk's slice in the table (BIG: 0, it is in Bb)
  const char* Bb;
  size_t kk;                      // floats between rows of Cv / P
  float *ptr, *nptr;              // where the current row goes, and the next one

  // dyn (drop-in flexspmm only; else nullptr): {buffers recognised, chunk count} written by dropin_guard_kernel — the grid
  // was sized from an upper bound, and buffers this library did not pack are not walked (no chunks: every wave leaves)
  __device__ __forceinline__ GroupChunk(const void* __restrict__ table, int nchunks, const int* __restrict__ dyn, int bx,
                                        int col_tile, int k, size_t kk_, int ld) {
    if (dyn) nchunks = dyn[0] ? dyn[1] : 0;
    lane = threadIdx.x & 63;
    wib  = threadIdx.x >> 6;
    g    = lane / LANES;
    f    = lane - g * LANES;
    per_xcd = nchunks >> 3;
    c_w = ((bx >> 3) * 4 + wib) * GROUPS;
    live = kWholeWaves || (g < GROUPS && c_w + g < per_xcd);
    c = (bx & 7) * per_xcd + (live ? c_w + g : c_w);
    fcol = col_tile * Row::kTileCols + f * Row::kLaneCols;
    col_ok = fcol < k;
    row_bytes = (unsigned)ld * (unsigned)Row::kElemBytes;
    foff = (unsigned)(col_ok ? fcol : col_tile * Row::kTileCols) * (unsigned)Row::kElemBytes;
    Bb = reinterpret_cast<const char*>(table);
    kk = kk_;
  }
  __device__ __forceinline__ bool none() const { return c_w >= per_xcd; }
  __device__ __forceinline__ void open(const int2* __restrict__ chunk_meta, float* __restrict__ Cv, float* __restrict__ P) {
    const int2 meta = chunk_meta[c];                              // one load: nothing else stands before the first gather
    const int vrow = meta.x >> 1;                                 // virtual row holding the chunk's first entry
    head = meta.x & 1;
    base = BIG ? 0 : meta.y;
    if constexpr (BIG) Bb += (size_t)meta.y * (size_t)row_bytes;  // (per lane: the groups of a wave can sit in different slices)
    ptr  = head ? P + (size_t)(2 * c) * kk + fcol : Cv + (size_t)vrow * kk + fcol;
    nptr = Cv + (size_t)(vrow + 1) * kk + fcol;
  }
};

// RING: finished rows wait in LDS, GROUPS slots per group, and leave GROUPS at a time — consecutive rows of ONE group,
// written by the whole wave with one 64-lane pass (a store occupies the addressers like a gather whatever its width).
// 16 or 32 KiB per block.  Indexed [wave][group][slot][lane] in place: through a reference to the wave's part the
// address arithmetic of a drain comes out differently.
template <class Row, int GROUPS, int LANES, bool RING>
__device__ __forceinline__ auto& block_ring() {
  __shared__ RowPieces<Row> ring[RING ? 4 : 1][GROUPS][GROUPS][LANES];
  return ring;
}

// Where the rows of this lane's group go (GROUPS * LANES == 64; the five-engine walk keeps its own text).
// A row that ends goes into the ring — unless it is the chunk's head piece or the ring is full, then straight to memory;
// full rings are drained after every block that ended a row, the rest after the loop.
template <class Row, int GROUPS, int LANES, bool RING>
struct RowSink {
  typedef RowPieces<Row> Ring[RING ? 4 : 1][GROUPS][GROUPS][LANES];
  Ring& ring;
  const int wib;
  float *ptr, *nptr;
  float* ring_base = nullptr;     // the first row waiting in the ring goes here (the next ones kk further each)
  const size_t kk;
  int ring_n = 0;                 // rows of this lane's group waiting in the ring
  const int g, f;
  bool first = true;              // no row of this chunk has ended yet
  const bool head, col_ok;

  template <bool BIG>
  __device__ __forceinline__ RowSink(const GroupChunk<Row, GROUPS, LANES, BIG>& ch, Ring& r)
      : ring(r), wib(ch.wib), ptr(ch.ptr), nptr(ch.nptr), kk(ch.kk), g(ch.g), f(ch.f), head(ch.head), col_ok(ch.col_ok) {}

  // the current row of this lane's group has ended with the sum r
  __device__ __forceinline__ void finish(const RowPieces<Row>& r) {
    if (RING && !(first && head) && ring_n < GROUPS) {
      if (col_ok) ring[wib][g][ring_n][f] = r;
      if (ring_n == 0) ring_base = ptr;
      ++ring_n;
    } else if (col_ok) store_row_pieces<Row>(ptr, r);
    ptr = nptr; nptr += kk; first = false;
  }
  // the rows waiting in group G2's ring (ALL: it is full): lane l writes the piece of lane l % LANES of row l / LANES.
  // The LDS read stands in front of the test: inside it the bf16 kernel ran 2-3 % slower (profiles/r14_drain_read_variants.json)
  template <bool ALL>
  __device__ __forceinline__ void drain(int G2) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(uintptr_t)ring_base, LANES * G2);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)((uintptr_t)ring_base >> 32), LANES * G2);
    float* b0 = reinterpret_cast<float*>(((uintptr_t)hi << 32) | lo);
    const RowPieces<Row> rv = ring[wib][G2][g][f];
    if (col_ok && g < (ALL ? GROUPS : __builtin_amdgcn_readlane(ring_n, LANES * G2)))
      store_row_pieces<Row>(b0 + (size_t)g * kk + f * Row::kLaneCols, rv);
    if (g == G2) ring_n = 0;
  }
  template <bool ALL>
  __device__ __forceinline__ void drain_flagged(unsigned long long flags) {   // bit LANES * G2: group G2's ring
#pragma unroll
    for (int G2 = 0; G2 < GROUPS; ++G2)
      if (flags & (1ull << (LANES * G2))) drain<ALL>(G2);
  }
  __device__ __forceinline__ void drain_full() {
    if constexpr (RING) { const unsigned long long full = __ballot(ring_n == GROUPS); if (full) drain_flagged<true>(full); }
  }
  __device__ __forceinline__ void drain_rest() { if constexpr (RING) drain_flagged<false>(__ballot(ring_n > 0)); }
  // the row piece that sticks out of the chunk's end (the last entry did not end its row): it is the FIRST piece of its
  // row — unless the whole chunk lies inside one row, then it is this chunk's head piece — and goes where the row's
  // partial sum lives, Cv[row]; the pieces of the chunks the row runs on into (their head pieces, P[2c]) are added by
  // the slice reduction (cut lists) or by group_fixup_kernel
  __device__ __forceinline__ void tail(bool row_open, const RowPieces<Row>& r) {
    if (row_open) {
      if (col_ok) store_row_pieces<Row>(ptr, r);
    }
  }
};

template <class Row, bool VALS, bool RING, bool BIG, int STAGE = Row::kStage>
__device__ __forceinline__ void
group_walk(const unsigned short* __restrict__ stream, const float* __restrict__ vals, const int2* __restrict__ chunk_meta,
           const void* __restrict__ table, float* __restrict__ Cv, float* __restrict__ P,
           int nchunks, int T, int k, int seg_blocks, int ld, int stream_nt, int blocks_per_tile, const int* __restrict__ dyn) {
  // T: entries per chunk of ONE group, a multiple of 64 (a chunk is whole runs of four blocks) — a run-time value: the
  // plan picks it so that the blocks fill whole rounds of the chip on small matrices (group_chunk, plan_policy.cpp)
  constexpr int TC = Row::kTileCols;
  const TileBlock tb = group_tile_block<TC>((int)blockIdx.x, blocks_per_tile, seg_blocks, k);
  // (GCN_ABLATE bit 3: partial rows of a tile contiguous — a layout experiment)
  GroupChunk<Row, 4, 16, BIG> ch(table, nchunks, dyn, tb.bx, tb.col_tile, k, (GCN_ABLATE & 8) ? (size_t)TC : (size_t)k, ld);
  if (ch.none()) return;
  // the stream is stored in runs of 64 entries, lane-major (slicing.hip, group_phys): lane f reads its entries of
  // four consecutive blocks with one 8-byte load (16 bytes for the values)
  const u32x2* __restrict__ sp = reinterpret_cast<const u32x2*>(stream + (size_t)ch.c * T) + ch.f;
  // The stream words of the runs ahead, w[0] the current run's; a run's end shifts them down by one (static indices:
  // registers).  Value-free: a STAGE of runs, fetched back to back at the chunk's start and again where a stage ends
  // inside the chunk (T > 64 * STAGE).  Vector-memory results return in order, and with one load per run — issued in
  // front of that run's first gathers, from HBM for a large stream — the compiler's wait in front of the gathers was
  // vmcnt(0): every run began by sitting out a stream load, eight times per chunk.  Fetched together the loads of a stage
  // overlap into ONE such wait: main kernel, Reddit-shaped k = 128, 2.30 -> 2.14 ms, and tile-major order, which reads
  // the whole stream from HBM once per tile, 2.44 -> 2.18 (profiles/stream_stage_gate.log).  Runs past the chunk's end
  // read its last run again (nothing is read beyond the chunk; the last chunk ends the buffer).  Weighted: the next run
  // only, a whole run ahead of its use, beside its values (126 VGPRs: no room for a stage of 16-byte value words).
  constexpr int NW = VALS ? 2 : STAGE;
  static_assert(NW >= 2 && (NW & (NW - 1)) == 0, "a stage is a power of two of runs, at least two");
  const int last_run = (GCN_ABLATE & 4) ? 0 : T / 64 - 1;
  u32x2 w[NW];
  auto load_stage = [&](int r0) {
#pragma unroll
    for (int i = 0; i < NW; ++i) w[i] = stream_load(sp + 16 * (r0 + i < last_run ? r0 + i : last_run), stream_nt);
  };
  ch.open(chunk_meta, Cv, P);
  RowSink<Row, 4, 16, RING> sink(ch, block_ring<Row, 4, 16, RING>());
  const int f = ch.f, base = ch.base;
  const unsigned row_bytes = ch.row_bytes, foff = ch.foff;
  const char* Bb = ch.Bb;

  // (GCN_ABLATE bit 4: every chunk reads the values of the first one, 1 KiB)
  const f32x4* __restrict__ vp = VALS ? reinterpret_cast<const f32x4*>(vals + ((GCN_ABLATE & 16) ? 0 : (size_t)ch.c * T)) + f : nullptr;
  typename Row::Unit acc[4] = {};
  if constexpr (VALS) { w[0] = stream_load(sp, stream_nt); w[1] = w[0]; }
  else load_stage(0);
  f32x4 vq = {0.f, 0.f, 0.f, 0.f}, vq_nx = vq;
  if constexpr (VALS) { vq = (GCN_ABLATE & 16) ? vp[0] : stream_load(vp, stream_nt); vq_nx = vq; }
  unsigned fl = 0;
#pragma unroll 1
  for (int blk = 0; blk < T / 16; ++blk) {
    const int j = blk & 3;
    if constexpr (VALS) {
      if (j == 0 && blk + 4 < T / 16 && !(GCN_ABLATE & 4)) {    // the next run, a whole run ahead of its use
        const int nx = (blk / 4 + 1) * 16;
        w[1] = stream_load(sp + nx, stream_nt);
        vq_nx = (GCN_ABLATE & 16) ? vp[nx & 63] : stream_load(vp + nx, stream_nt);
      }
    } else {
      if (blk != 0 && (blk & (4 * NW - 1)) == 0) {              // a stage ends: the next one
        load_stage(blk >> 2);
      }
    }
    const unsigned e = ((j & 2 ? w[0].y : w[0].x) >> (16 * (j & 1))) & 0xFFFFu;
    int vbits = 0;                                              // this lane's entry's value; step u takes lane u's
    if constexpr (VALS) vbits = __builtin_bit_cast(int, j == 0 ? vq.x : j == 1 ? vq.y : j == 2 ? vq.z : vq.w);
    if (j == 3) {
#pragma unroll
      for (int i = 0; i + 1 < NW; ++i) w[i] = w[i + 1];
      vq = vq_nx;
    }
    const int rowoff = (int)(__umul24((e & 0x7FFFu) + (unsigned)base, row_bytes));
    fl = e >> 15;
    uint4 b[16];
#define GCN_G_ALL(M) M(0) M(1) M(2) M(3) M(4) M(5) M(6) M(7) M(8) M(9) M(10) M(11) M(12) M(13) M(14) M(15)
#define GCN_G_GATHER(UU) \
    b[UU] = *reinterpret_cast<const uint4*>(Bb + (size_t)((unsigned)row_bcast<UU>(rowoff) + foff));
    GCN_G_ALL(GCN_G_GATHER)
#undef GCN_G_GATHER
    const unsigned long long ends = (GCN_ABLATE & 2) ? 0ull : __ballot(fl != 0);   // bit g*16+u: entry u of group g ends a row
#define GCN_G_ADD(UU)                                                                               \
    {                                                                                               \
      typename Row::Unit w[4];                                                                      \
      Row::widen(b[UU], w);                                                                         \
      if constexpr (VALS && (GCN_ABLATE & 64) == 0) {                                               \
        const float vu = __builtin_bit_cast(float, (GCN_ABLATE & 32) ? vbits : row_bcast<UU>(vbits)); \
        _Pragma("unroll") for (int i = 0; i < 4; ++i)                                               \
          acc[i] = __builtin_elementwise_fma((typename Row::Unit)vu, w[i], acc[i]);             \
      } else {                                                                                      \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) acc[i] += w[i];                             \
        if constexpr (VALS) asm volatile("" : : "v"(vbits));                                        \
      }                                                                                             \
    }
    if (ends == 0ull) {
      GCN_G_ALL(GCN_G_ADD)
    } else {
#define GCN_G_STEP(UU)                                                                              \
      GCN_G_ADD(UU)                                                                                 \
      if (ends & (group_bits<4, 16>() << UU)) {                  /* some group ends a row here */    \
        if (row_bcast<UU>((int)fl)) {                                                               \
          sink.finish(row_pieces<Row>(acc));                                                        \
          _Pragma("unroll") for (int i = 0; i < 4; ++i) acc[i] = typename Row::Unit{};              \
        }                                                                                           \
      }
      GCN_G_ALL(GCN_G_STEP)
#undef GCN_G_STEP
      sink.drain_full();
    }
#undef GCN_G_ADD
#undef GCN_G_ALL
  }
  sink.drain_rest();
  sink.tail(!row_bcast<15>((int)fl), row_pieces<Row>(acc));
}

}  // namespace gcn
