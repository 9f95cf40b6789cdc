// plan_policy.cpp — the dispatch policy of libgcnspmm's SpMM plan: chunk size, column tile, slice count, row stride of
// the re-laid feature table, and which kernel family / slice set a k-wide call takes.  Every threshold here is a measured
// one (the experiment is cited beside it); the alternate paths those experiments decided against are gone — what remains
// switchable is what a test needs (plan_policy.h).  Plan construction is plan_build.cpp, the launches api_spmm.cpp.
#include "plan_policy.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>

namespace gcn {

std::mutex g_plan_mu;

int cu_count_cached() {
  static int cached[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return -1;
  if (dev < 0 || dev >= 64) return -1;
  if (cached[dev] > 0) return cached[dev];
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return -1;
  cached[dev] = prop.multiProcessorCount;
  return cached[dev];
}

// chunk size: the largest power of two <= nnz / resident waves (8 blocks x 4 waves per CU), within
// [64, 2048].  Measured (profiles/r01_sweep_chunk_size.txt): every chunk boundary costs a partial
// row (slab write + fix-up read) and a row-pointer restart, and that outweighs the load imbalance of
// having only one or two chunks per wave — Reddit-shaped 1 GPU: T = 512 / 1024 / 2048 / 4096 ->
// 4.12 / 4.03 / 3.94 / 4.04 ms; rank of an 8-way partition: T = 64 / 512 / 2048 / 4096 ->
// 0.68 / 0.56 / 0.556 / 0.67 ms.
int auto_chunk_nnz(long long nnz, int cu) {
  if (cu <= 0) cu = 256;
  const long long waves = (long long)cu * 32;
  const long long per_wave = nnz / waves;
  long long t = 64;
  while (t * 2 <= per_wave && t < 2048) t *= 2;
  return (int)t;
}

// Feature-column tile per pass.  Measured on MI355X (profiles/r01_sweep_tiles_*.txt): when one
// 64-column slice of B (n x 256 B) sits well inside the 256 MiB Infinity Cache, k/64 narrow
// passes beat one wide pass by 3-6 % (Reddit-shaped, n = 233 k); when it does not (products-
// shaped, n = 2.4 M) the widest tile wins by 6-7 %.
int auto_tile_cols(long long n, int k) {
  if (k <= 64) return 0;
  const long long budget = 128LL << 20;          // half of the Infinity Cache
  if (n * 256 <= budget) return 64;
  if (n * 512 <= budget && k > 128) return 128;
  return 0;                                      // widest tile k allows (<= 256 columns)
}

// Parts of the candidate range per query block of gcn_knn_f32 when the caller passes splits = 0.  NOT MEASURED: the aim is two
// workgroups per CU (a workgroup at k = 64 takes 99 KiB of LDS, so one is resident per CU and the second fills the tail),
// with at least 8 candidate tiles per part so that a part's k keys and its merge stay small beside its distances.
int knn_auto_splits(int q, int n, int cus) {
  if (cus <= 0) cus = 256;
  const long long blocks = ((long long)q + kKnnTileQ - 1) / kKnnTileQ;
  const long long tiles = ((long long)n + kKnnTileC - 1) / kKnnTileC;
  if (blocks <= 0) return 1;
  long long s = (2LL * cus + blocks - 1) / blocks;
  if (s > tiles / 8) s = tiles / 8;
  return s < 1 ? 1 : (int)s;
}

namespace {
bool env_on(const char* name) { const char* e = std::getenv(name); return !e || e[0] != '0'; }
}  // namespace

bool group_fused_fixup() { static const bool v = env_on("GCN_AMD_GROUP_FUSED_FIXUP"); return v; }

// Entries per chunk of one 16-lane group.  A block walks 16 chunks and 4 blocks are resident per CU (114 VGPRs), so the
// chip holds cu*4 blocks per "round".  Large matrices run many rounds and 512 is the measured optimum
// (profiles/r02zg_chunk_length_slices.log); a matrix of a few rounds — a rank's row block of an 8-way partition: 1.7
// rounds at 512 — leaves the last round partly empty, so the length is picked from the multiples of 64 in [256, 1024]
// that fill whole rounds best (ties: the one closest to 512).
// GCN_AMD_GROUP_T (development / tests, read once per process): that length for every plan — a multiple of 64 in
// [64, 1024], anything else is ignored — so that small graphs reach the stage boundaries of the walk (group_walk.h).
int group_chunk(long long entries, int cu) {
  static const int forced = [] {
    const char* e = std::getenv("GCN_AMD_GROUP_T");
    const int t = e ? std::atoi(e) : 0;
    return t >= 64 && t <= 1024 && t % 64 == 0 ? t : 0;
  }();
  if (forced) return forced;
  if (cu <= 0) cu = 256;
  const double round = (double)cu * 4.0;
  if ((double)entries / (16.0 * 512.0) >= 6.0 * round) return 512;
  double fills[13], top = 0.0;                         // t = 256 + 64*i
  for (int i = 0; i < 13; ++i) {
    const double blocks = (double)entries / (16.0 * (256 + 64 * i));
    const double rounds = std::ceil(blocks / round);
    fills[i] = rounds > 0 ? blocks / (rounds * round) : 0.0;
    if (fills[i] > top) top = fills[i];
  }
  int best = 512;
  bool have = false;
  for (int i = 0; i < 13; ++i) {                       // among the lengths within 2 % of the best fill: the one closest to 512
    const int t = 256 + 64 * i;
    if (fills[i] >= top - 0.02 && (!have || std::abs(t - 512) < std::abs(best - 512))) { best = t; have = true; }
  }
  return best;
}

namespace {
// Expected 128-byte cache lines one gathered feature row costs, summed over its 64-column tiles, when B's
// rows are `ld` floats apart (the row start offsets cycle through the multiples of gcd(4*ld, 128)).
double lines_per_row(int k, int ld) {
  const long long row_bytes = 4LL * ld;
  long long g = row_bytes % 128;
  for (long long a = 128; g != 0;) { const long long t = a % g; a = g; g = t; if (g == 0) { g = a; break; } }
  if (g == 0) g = 128;                                // row_bytes % 128 == 0: every row starts on a line
  const int period = (int)(128 / g);
  double total = 0;
  for (int r = 0; r < period; ++r) {
    const long long off = (r * row_bytes) % 128;
    for (long long t0 = 0; t0 < 4LL * k; t0 += 256) {
      const long long w = (4LL * k - t0) < 256 ? (4LL * k - t0) : 256;
      const long long start = (off + t0) % 128;
      total += (double)((start + w - 1) / 128 + 1);
    }
  }
  return total / period;
}
}  // namespace

// Row stride (floats) B is gathered with: k itself, or k rounded up to whole 128-byte lines when that
// saves >= 15 % of the cache lines per gathered row and the re-laid table stays <= 768 MiB.  Measured
// (profiles/r01f_sweep_padded_feature_rows.log, whole SpMM, unpadded -> padded): Reddit-shaped k = 20:
// 2.19 -> 1.60 ms, 24: 2.26 -> 1.60, 47: 2.11 -> 2.00, 100: 4.43 -> 3.84, 172: 7.56 -> 5.73; no saving
// by the model and none measured for k = 40, 48 (rows of 160 / 192 B never straddle more lines than
// padded ones); products-shaped k = 47 (627 MB padded): 5.41 -> 4.86 ms, k = 100 (1.25 GB): 8.95 ->
// 9.73 ms — past the Infinity Cache the larger table and the copy cost more than the lines save.
int padded_ldb(long long n, int k) {
  if (k <= 16 || k % 32 == 0) return k;
  const int ld = (k + 31) / 32 * 32;
  if ((long long)sizeof(float) * n * ld > (768LL << 20)) return k;
  return lines_per_row(k, k) >= 1.15 * lines_per_row(k, ld) ? ld : k;
}

// Number of column slices for the XCD-aware slicing (slicing.hip), 0 = do not slice.
// Measured on MI355X with the r01f kernels (profiles/r01f_sweep_slices_scales.log; Reddit-shaped graphs
// of 14.5 k .. 1.86 M vertices, mean degree 493; whole SpMM, k = 128, best S in brackets):
//   n = 14.5 k (64-column table 3.7 MB): slicing buys nothing;  29 k (7.5 MB): [2] 0.352 vs 0.394 ms
//   unsliced;  58 k: [4] 0.84 vs 1.18;  116 k: [4/8] 1.76-1.80 vs 3.13;  233 k: [8] 3.62 vs 7.3;
//   466 k: [8] 9.20 vs 15.7 (16: 9.84);  932 k: [8] 24.4 vs 32.3;  1.86 M: [8] 56.5 vs 62.5.
// So, for matrices with a value stream on the four-per-gather kernel: as many slices as bring one slice of
// the table (n/S x 256 B) down to the 4 MiB of an XCD's L2, but never more than the 8 XCDs — beyond 8 every
// XCD walks several slices and the extra partial rows (S*m*k floats written and re-read) cost more than the
// higher hit rate returns.
// `value_free` (the group kernels of spmm_group.hip run, with or without the value stream): a partial row costs
// one non-temporal 256-byte store and no cross-lane work, so the count follows the table alone — one slice per
// 4 MiB of it (n = 233 k: 15), XCDs walking two slices each one after the other.  Measured
// (profiles/r02z5_nt_stores_slices.log, whole SpMM k = 128): S = 8 / 14 / 16 / 18 / 20 / 24 / 32:
// 3.19 / 3.08 / 3.09 / 3.13 / 3.19 / 3.36 / 3.68 ms — flat from 14 to 16, then the slab of partial rows
// (S*m*k floats, written and re-read by the reduction) takes over.
// Both need >= 16 non-zeros per virtual row; at mean degree 51 (products-shaped) slicing loses and stays off.
int auto_slices(long long m, long long n, long long nnz, bool value_free) {
  if (m <= 0 || nnz <= 0) return 0;
  if (nnz / m < 128) return 0;                        // low degree: partial rows outweigh the hits
  const long long table = n * 256;                    // bytes of one 64-column tile of B
  const long long l2 = 4LL << 20;
  if (table <= l2) return 0;                          // fits every L2 as it is
  if (value_free) {
    long long S = (table + l2 - 1) / l2;
    const long long narrow = (n + 32766) / 32767;     // the group kernel's 15-bit entries: slices <= 32 767 columns
    if (S < narrow) S = narrow;
    if (S > 8) {                                      // (up to 8 the rule below gives the same or better)
      if (S > nnz / m / 16) S = nnz / m / 16;         // keep >= 16 non-zeros per virtual row
      if (S > 8 && S <= 1024 && S >= narrow && table / S <= 2 * l2) return (int)S;
    }
  }
  int S = 2;
  while (S < 8 && table / S > l2) S *= 2;
  while (S > 1 && nnz / m / S < 16) S /= 2;           // keep >= 16 non-zeros per virtual row
  if (S < 2) return 0;
  // slices far larger than any cache (huge n): the partial rows cost traffic and buy no hits
  if (table / S > (64LL << 20)) return 0;
  return S;
}

void die(const char* what, hipError_t e) {
  std::fprintf(stderr, "libgcnspmm: %s failed: %s\n", what, hipGetErrorString(e));
  std::abort();
}

bool verbose() {
  const char* v = std::getenv("GCN_AMD_VERBOSE");
  return v && v[0] && v[0] != '0';
}

// The stateless entry points (oneshot / cuspmm / flexspmm) keep their partial slab and chunk rows in a
// scratch plan per (device, stream): two calls that can run concurrently never share buffers.  The plans
// are never freed (a static destructor would call hipFree after the runtime has shut down).
gcn_spmm_plan* scratch_plan(void* stream) {
  static auto* plans = new std::map<std::pair<int, void*>, gcn_spmm_plan*>();
  int dev = 0;
  (void)hipGetDevice(&dev);
  auto& slot = (*plans)[{dev, stream}];
  if (!slot) { slot = new (std::nothrow) gcn_spmm_plan(); if (slot) slot->device = dev; }
  return slot;
}

size_t ws_elems(const gcn_spmm_plan* p, int k) {
  int chunks = std::max(p->nchunks, p->panels.out_nchunks);
  chunks = std::max(chunks, p->col16.nchunks16);
  chunks = std::max(chunks, p->group.nchunks);
  chunks = std::max(chunks, p->group_alt[0].nchunks);   // (whichever slice set a call picks: room for the larger)
  return 2 * (size_t)(chunks > 0 ? chunks : 1) * (size_t)k;
}

namespace {

SliceSet own_slice_set(const gcn_spmm_plan* p) {
  SliceSet s;
  s.g = &p->group; s.S = p->slicing.S; s.alt = -1;
  return s;
}

// Widths that are not a multiple of 4 can take a detour over k4 = k rounded up to 4 (OddShape) to reach the
// 16-byte-per-lane kernels: never from a panel plan or one kept on one non-zero per gather, and only while the padded
// table fits its cap
bool detour_possible(const gcn_spmm_plan* p, int k, const OddShape& o) {
  return k > 16 && k % 4 != 0 && p->nnz > 0 && p->panels.R == 0 && p->gather_width != 1 && o.fits;
}

// Is a k-wide SpMM of this plan launched on the sliced copy?  The four-per-gather kernel pays from k = 33 (narrower
// rows gather 128 B or less per non-zero: the partial rows cost more than the L2 hits buy, 2.12 vs 2.02 ms at
// k = 32).  The group kernels pay from k = 12: their 64-column pass costs the same whatever k is, and beats the
// unsliced kernels there (Reddit-shaped, whole SpMM, profiles/r02zzg_narrow_widths_sliced.log: k = 12 / 16 / 20 /
// 32: 1.49 / 1.36 / 1.60 / 1.58 -> 1.23 / 1.02 / 1.23 / 1.10 ms; k = 8 a tie, k = 4 loses) — provided the width
// reaches them (lanes16): a multiple of 4, or one the detour is possible for.
bool sliced_for(const gcn_spmm_plan* p, int k, bool lanes16) {
  if (p->slicing.S <= 0 || p->nnz <= 0) return false;
  if (k >= kSliceMinK) return true;
  return p->group.ready() && p->panels.R == 0 && k >= kGroupMinK && lanes16;
}

// ... and is the detour taken?  It follows the rule of the kernels it reaches: the four-per-gather kernel only pays from
// ~48 non-zeros per (virtual) row up, the group kernels do not mind short rows
bool odd_width_detour(const gcn_spmm_plan* p, bool sliced) {
  if (p->gather_width == 4) return true;
  if (sliced && p->group.ready() && (p->group.vals || value_free_plan(p))) return true;
  const long long rows = sliced ? (long long)p->slicing.S * p->m : (long long)p->m;
  return rows > 0 && p->nnz / rows >= 48;
}

// What the sliced launch of a k-wide pass (B gathered with stride ld) runs.  valless: a value-free kernel, on a copy of
// B scaled by u_col.  (That copy costs 2*n*k*4 bytes of traffic whatever the matrix; the value stream it saves is
// 4 bytes per non-zero plus instructions.  With the group kernel the rank-0 share of an 8-way partition of the
// Reddit-shaped graph, 61 non-zeros per column of the block, still gains: 0.460 against 0.511 ms,
// profiles/r02z7_rank_share_value_free.log; below 48 per column nothing has been measured, so it stays off — and a plan
// whose group stream carries values was built for the weighted pass: value-free did not pay.)  weighted: the group
// kernel with the values beside its stream.  group: either way B is gathered from the slice-by-slice copy.
struct PassKind { bool valless = false, weighted = false, group = false; };
PassKind pass_kind(const gcn_spmm_plan* p, int k, int ld, bool sliced, int tile_cols) {
  PassKind pk;
  if (!sliced || p->panels.R != 0) return pk;
  const bool walks = p->group.ready() && spmm_group_eligible(k, ld, own_slice_set(p).table_rows(), nullptr, nullptr, nullptr);
  if (p->group.vals) { pk.weighted = pk.group = walks; return pk; }
  if (!value_free_plan(p)) return pk;
  if (walks) { pk.valless = pk.group = true; return pk; }
  SpmmRoute r;                                         // without the group stream: the four-per-gather kernel, all 16 lanes
  r.family = SpmmFamily::sliced_quad; r.k_run = k; r.ldb = ld; r.copy = BCopy::row_padded; r.tile_cols = tile_cols;
  const ChunkChoice c = spmm_chunk_choice(spmm_args(p, r, false));
  pk.valless = c.family == ChunkFamily::quad && c.lanes == 16;
  pk.group = pk.valless && p->group.ready();        // (a stream that exists is walked: the width it cannot serve is refused there)
  return pk;
}

// The narrow slice set (k <= 32: plan_build.cpp, maybe_build_alt) when the plan has or can have one, else its own
SliceSet narrow_slice_set(gcn_spmm_plan* p, int k, bool build, const int32_t* rowptr, const int32_t* col, const float* val,
                          hipStream_t st) {
  const int cls = alt_class(k);
  if (cls < 0) return own_slice_set(p);
  if (build) maybe_build_alt(p, cls, rowptr, col, val, st);
  if (!p->group_alt[cls].ready()) return own_slice_set(p);
  SliceSet s;
  s.g = &p->group_alt[cls]; s.S = p->alt_S[cls]; s.alt = cls;
  return s;
}

}  // namespace

OddShape odd_width_shape(long long n, int k) {
  OddShape o;
  o.k4 = (k + 3) / 4 * 4;
  o.ld = (o.k4 + 31) / 32 * 32;
  o.fits = (long long)sizeof(float) * n * o.ld <= (768LL << 20);
  return o;
}

// will a sliced plan of this matrix run the group kernel value-free (known before the slicing exists)
bool value_free_plan(const gcn_spmm_plan* p) {
  return p->factors.ready() && p->panels.R == 0 && p->nnz / p->n >= kVallessMinPerCol;
}
// ... or the group kernel at all (value-free or weighted): it decides the automatic slice count
bool group_plan(const gcn_spmm_plan* p) { return p->panels.R == 0; }

int alt_class(int k) { return k <= 32 ? 0 : -1; }

// the shape of one call's group launch on ss: what the launch (run_group_walk adds the buffers) and the report decide from
GroupArgs group_shape(const SliceSet& ss, bool weighted, int elem_bytes, int ld, int k) {
  const GroupStream& G = *ss.g;
  GroupArgs ga{};
  ga.stream = G.stream; ga.chunk_meta = G.chunk_meta;
  ga.vals = weighted ? G.vals.get() : nullptr;
  ga.elem_bytes = elem_bytes;
  ga.nchunks = G.nchunks; ga.T = G.T; ga.k = k; ga.ldb = ld;
  ga.table_rows = ss.table_rows();
  ga.narrow8 = group8_enabled() ? 1 : 0;
  return ga;
}

// The route of a k-wide fp32 call.
// Feature rows that are not a whole number of 128-byte cache lines straddle lines: where that matters (padded_ldb) B is
// first re-laid with its rows padded to the next multiple of 32 floats (one streaming copy, ~45 us for 233 k x 100) and
// gathered from there.  The same copy carries the row scaling of the value-free pass (values u[r]*u[c]: B' = diag(u) B)
// and, for the group kernels, the slice-by-slice layout.  Widths that are not a multiple of 4 (class counts: 41, 47, ...)
// cannot use the 16-byte-per-lane kernels on the caller's layout: where the detour pays they are computed at k4 on such
// copies, B re-laid with zero columns and the product compacted into C afterwards (Reddit-shaped k = 41: 2.13 -> 1.87 ms).
// The slice set of a value-free group launch: k <= 32 the narrow set; widths 33..48 stay on the plan's own slices, and
// where the stride would have been padded to 64 floats (k = 44 and the detour's k4) the five-engine kernel gathers from
// rows of 48 instead (192 bytes: always two lines, a quarter less table and copy; k = 41 / 47: 1.39 / 1.36 -> 1.34 /
// 1.30 ms; 36 / 40 keep their dense rows).  (A slice set of their own — 11..13 slices instead of 15 — was built and
// measured: +-1 %, profiles/r03ba_*; not kept.)
SpmmRoute spmm_route(gcn_spmm_plan* p, int k, bool build, const int32_t* rowptr, const int32_t* col, const float* val,
                     hipStream_t st, bool prelaid) {
  SpmmRoute r;
  r.ss = own_slice_set(p);
  const OddShape o = odd_width_shape(p->n, k);
  const bool may_detour = !prelaid && detour_possible(p, k, o);
  const bool sliced = sliced_for(p, k, k % 4 == 0 || may_detour);
  r.odd = may_detour && odd_width_detour(p, sliced);
  r.k_run = r.odd ? o.k4 : k;
  r.ldb = r.odd ? o.ld : padded_ldb(p->n, k);
  if (p->panels.R > 0 && p->nnz > 0 && k > 32) {
    r.family = SpmmFamily::panels;
    r.tile_cols = p->tile_cols ? p->tile_cols : auto_tile_cols(p->n, k);
  } else {
    r.tile_cols = p->tile_cols ? p->tile_cols : (sliced ? 64 : auto_tile_cols(p->n, k));
    const PassKind pk = pass_kind(p, r.k_run, r.ldb, sliced, r.tile_cols);
    r.valless = pk.valless; r.weighted = pk.weighted;
    r.family = pk.group ? SpmmFamily::group : sliced ? SpmmFamily::sliced_quad : SpmmFamily::unsliced;
    r.col16 = r.family == SpmmFamily::sliced_quad && r.valless && p->col16.ready();
    if (pk.group && r.valless && !prelaid) {
      if (r.k_run <= 32) r.ss = narrow_slice_set(p, r.k_run, build, rowptr, col, val, st);
      else if (r.k_run <= 48 && r.ldb > 48 &&
               spmm_group_choice(group_shape(r.ss, false, 4, 48, r.k_run)).engine == GroupEngine::five12) r.ldb = 48;
    }
    r.S_run = pk.group ? r.ss.S : sliced ? p->slicing.S : 0;
    r.reduce_epilogue = sliced && !r.odd;
  }
  if (prelaid) return r;                               // (B comes in the group layout, rows r.ldb apart)
  if (p->nnz > 0 && r.family == SpmmFamily::group) r.copy = BCopy::group_layout;
  else if (p->nnz > 0 && (r.odd || r.ldb != k || r.valless)) r.copy = BCopy::row_padded;
  else r.ldb = k;                                      // the caller's own rows
  return r;
}

// The launch of a non-group route as launch_spmm takes it, without the operand pointers (panels: of the pass over the
// entries outside the windows)
SpmmArgs spmm_args(const gcn_spmm_plan* p, const SpmmRoute& r, bool epilogue) {
  SpmmArgs a{};
  a.relu = epilogue && !r.reduce_epilogue && !r.odd ? 1 : 0;
  a.nchunks = a.nchunks_grid = p->nchunks; a.T = p->T; a.m = p->m; a.nnz = p->nnz; a.k = r.k_run; a.n = p->n;
  a.ldb = r.ldb != r.k_run ? r.ldb : 0;
  a.empty_rows = p->empty_rows;
  a.tile_cols = r.tile_cols;
  a.blocks_per_cu = p->blocks_per_cu;
  a.gather_width = p->gather_width;
  if (r.family == SpmmFamily::panels) {
    const Panels& pn = p->panels;
    a.nchunks = a.nchunks_grid = pn.out_nchunks; a.T = pn.out_T; a.nnz = pn.out_nnz;
    a.empty_rows = -1;                                 // (rows whose entries all sit inside their window: not counted)
    a.accumulate = 1;
  } else if (r.family == SpmmFamily::sliced_quad) {
    const Slicing& sl = p->slicing;
    a.m = sl.S * p->m;
    a.empty_rows = sl.empty_vrows;
    a.stream_rows = 1;                                 // partial rows leave with non-temporal stores (3.667 -> 3.646 ms, profiles/r02zi_*)
    a.valless = r.valless ? 1 : 0;
    if (r.col16) {                                     // 16-bit column stream, slice-aligned chunks
      const Col16Stream& c16 = p->col16;
      a.nnz = c16.nnz16; a.nchunks = a.nchunks_grid = c16.nchunks16;
      a.col16 = 1; a.col16_S = sl.S; a.col16_w = (p->n + sl.S - 1) / sl.S;
      a.empty_rows = -1;                               // (its own row pointer: not counted)
      for (int i = 0; i < 9; ++i) a.col16_start[i] = c16.start16[i];
    }
  }
  return a;
}

// bf16 operands (spmm_group_bf16.hip): widths k >= 64 with k % 8 == 0 on a plan that runs a group kernel.  The slice set
// follows the table's row BYTES, not k: a bf16 call at k takes the set of an fp32 call at k / 2 (k = 64: the narrow set
// of 128-byte rows, built here at first use like the fp32 k <= 32 one; the five-engine kernel's 48-float rows are an fp32
// matter only).  Rows of the bf16 table are padded to whole 128-byte lines.  Anything else — unsliced plans, panels,
// narrow / odd widths — takes the fallback.
bool spmm_route_bf16(gcn_spmm_plan* p, int k, bool build, const int32_t* rowptr, const int32_t* col, const float* val,
                     hipStream_t st, SpmmRoute* r) {
  if (k < 64 || k % 8 != 0 || p->nnz <= 0 || p->panels.R != 0 || !p->group.ready()) return false;
  const int ldh = (k + 63) / 64 * 64;
  const int kw = k / 2, ldw = ldh / 2;                 // the fp32 width and stride with the same row bytes
  const PassKind pk = pass_kind(p, kw, ldw, sliced_for(p, kw, true), p->tile_cols ? p->tile_cols : 64);
  if (!pk.group) return false;
  const SliceSet ss = pk.valless ? narrow_slice_set(p, kw, build, rowptr, col, val, st) : own_slice_set(p);
  const GroupStream* g = ss.g;
  if (!g || !g->ready() || g->nchunks % 32 != 0 || g->T < 64 || g->T % 64 != 0) return false;
  if (spmm_group_needs_big(ss.table_rows(), ldh * 2LL) && ldh * 2 >= (1 << 17)) return false;
  *r = SpmmRoute{};
  r->family = SpmmFamily::group; r->k_run = k; r->elem_bytes = 2; r->ldb = ldh; r->copy = BCopy::group_layout_bf16;
  r->valless = pk.valless; r->weighted = pk.weighted; r->ss = ss; r->S_run = ss.S; r->reduce_epilogue = true;
  return true;
}

// the route as it stands: the reports build nothing
static SpmmRoute report_route(const gcn_spmm_plan* p, int k, bool prelaid = false) {
  return spmm_route(const_cast<gcn_spmm_plan*>(p), k, /*build=*/false, nullptr, nullptr, nullptr, nullptr, prelaid);
}

// the kernel a group route's walk runs, fp32 or bf16: the shape run_group_walk (api_spmm.cpp) launches with
static void group_route_kernel_name(const SpmmRoute& r, char* buf, int buflen) {
  spmm_group_kernel_name(spmm_group_choice(group_shape(r.ss, r.weighted, r.elem_bytes, r.ldb, r.k_run)), buf, (size_t)buflen);
}

// only the value-free group pass gathers from a scaled, slice-by-slice copy of B; the layout is that of the plan's OWN
// slice set whatever the width
int spmm_route_prelaid(const gcn_spmm_plan* p, int k, SpmmRoute* r) {
  if (k <= 0 || k % 4 != 0) return GCN_ERR_INVALID_ARG;
  *r = report_route(p, k, /*prelaid=*/true);
  return r->family == SpmmFamily::group && r->valless ? GCN_OK : GCN_ERR_INVALID_ARG;
}

}  // namespace gcn

using namespace gcn;

extern "C" {

int32_t gcn_spmm_plan_num_passes(const gcn_spmm_plan_t* p, int32_t k) {
  if (!p || k <= 0) return -1;
  const SpmmRoute r = report_route(p, k);
  if (r.family == SpmmFamily::panels) return (k + 63) / 64;
  if (r.family == SpmmFamily::group) return 1;         // the group kernels take every tile in one launch
  const int vec = pick_vec(r.k_run, r.tile_cols, nullptr, nullptr, nullptr);   // 16-B aligned operands
  return (r.k_run + 64 * vec - 1) / (64 * vec);
}

int gcn_spmm_plan_main_kernel(const gcn_spmm_plan_t* p, int32_t k, int32_t epilogue, char* buf, int32_t buflen) {
  if (!p || k <= 0 || !buf || buflen <= 0) return GCN_ERR_INVALID_ARG;
  const SpmmRoute r = report_route(p, k);
  if (r.family == SpmmFamily::panels) snprintf(buf, (size_t)buflen, "gcn::spmm_panel_in_kernel");
  else if (r.family == SpmmFamily::group) group_route_kernel_name(r, buf, buflen);
  else spmm_chunk_kernel_name(spmm_chunk_choice(spmm_args(p, r, epilogue != 0)), buf, (size_t)buflen);
  return GCN_OK;
}

int gcn_spmm_plan_main_kernel_bf16(const gcn_spmm_plan_t* p, int32_t k, int32_t epilogue, char* buf, int32_t buflen) {
  if (!p || k <= 0 || !buf || buflen <= 0) return GCN_ERR_INVALID_ARG;
  SpmmRoute r;                                         // (the slice set only as it exists: nothing is built here)
  if (!spmm_route_bf16(const_cast<gcn_spmm_plan*>(p), k, /*build=*/false, nullptr, nullptr, nullptr, nullptr, &r))
    return gcn_spmm_plan_main_kernel(p, k, epilogue, buf, buflen);                 // the fallback runs the fp32 entry
  group_route_kernel_name(r, buf, buflen);
  return GCN_OK;
}

int gcn_spmm_plan_prelaid_layout(const gcn_spmm_plan_t* p, int32_t k, int32_t* slices, int32_t* slice_cols,
                                 int64_t* table_rows, int32_t* ld) {
  SpmmRoute r;
  if (!p) return GCN_ERR_INVALID_ARG;
  if (const int rc = spmm_route_prelaid(p, k, &r); rc != GCN_OK) return rc;
  if (slices) *slices = r.ss.S;
  if (slice_cols) *slice_cols = r.ss.g->w;
  if (table_rows) *table_rows = r.ss.table_rows();
  if (ld) *ld = r.ldb;
  return GCN_OK;
}

int32_t gcn_spmm_auto_slices(int64_t m, int64_t n, int64_t nnz, int32_t value_free) {
  return auto_slices(m, n, nnz, value_free != 0);
}

int32_t gcn_spmm_group_addressing(int64_t table_rows, int32_t ld_floats) {
  if (table_rows <= 0 || ld_floats <= 0) return -1;
  if (!spmm_group_eligible(ld_floats, ld_floats, table_rows, nullptr, nullptr, nullptr)) return -1;
  return spmm_group_needs_big(table_rows, ld_floats * 4LL) ? 1 : 0;
}

}  // extern "C"
