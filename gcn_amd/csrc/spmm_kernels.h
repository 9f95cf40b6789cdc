// Internal interface between the C-ABI layer (plan_policy.cpp, plan_build.cpp, api_spmm.cpp, api_units.cpp, api_dropin.cpp)
// and the device code (spmm_kernels.hip).  Not installed; the public contract is include/gcn_spmm.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "philox.h"

namespace gcn {

// The ReLU of every fused epilogue: max(x, 0) on every number and on +-Inf, NaN kept (fmaxf alone answers 0 to a NaN, and
// torch.relu, which the fused path stands for, answers NaN).  Same bits as fmaxf(x, 0.f) for every x that is not a NaN.
__device__ __forceinline__ float relu_keep_nan(float x) { return x != x ? x : fmaxf(x, 0.f); }

struct SpmmArgs {
  const int*   rowptr;     // [m+1] device
  const int*   col;        // [nnz] device
  const float* val;        // [nnz] device
  const float* B;          // [n x k] device, row-major, ld = k
  float*       C;          // [m x k] device, row-major, ld = k
  float*       P;          // partial slab [2*nchunks x k] device
  const int*   chunk_row;  // [nchunks] device
  const float* bias;       // [k] or nullptr
  int relu;
  int nchunks, T, m, nnz, k;
  int n = 0x7fffffff;      // rows of B (columns of A); decides 32-bit buffer addressing
  int ldb = 0;             // row stride of B in floats, 0 = k (api_spmm.cpp pads rows to 128-byte lines for odd k)
  // drop-in mode (flexspmm symbol): nnz is only known on the device (nnz_dev =
  // &rowptr[m]); the kernels then derive nchunks and the value pointer themselves
  // and the host sizes its grids with the upper bound nchunks_grid.
  const int* nnz_dev;
  int nchunks_grid;
  // optional HIP events recorded on the launch stream right before / after the MAIN
  // kernel (not the fix-up) — the live kernel timing bench.py reports (null = off)
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;
  int tile_cols = 0;       // feature-column tile per pass: 0 auto, else 64 / 128 / 256
  int accumulate = 0;      // 1: C += A*B (C already holds another part of the product); epilogue after the add
  int col16 = 0;           // 1 (value-free pass only): a.col is a 16-bit stream of offsets inside the slice, see spmm_quad.hip
  int col16_S = 0, col16_w = 0, col16_start[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  int valless = 0;         // 1: ignore val (every entry counts 1): the caller pre-scaled B and post-scales the rows
  int stream_rows = 0;     // 1: finished rows are written with non-temporal stores (partial rows of a sliced pass: read back
                           // only by the slice reduction; spmm_quad_kernel)
  int gather_width = 0;    // 64-column tile: non-zeros per gather instruction, 0 auto (4 when eligible), 1, 4
  // Empty rows are never written by the main kernels (a run of them would be walked by ONE wave, row by row: the
  // 6.5 s of profiles/r03d_hub_split_probe_rmat24.log) — they skip whole runs (next_nonempty_row) and a pass of its own
  // writes every empty row in parallel (launch_fill_empty_rows).  empty_rows: how many the matrix has when the caller
  // knows (0: the pass is skipped), -1: unknown (the pass always runs).
  int empty_rows = -1;
  int blocks_per_cu = 32;  // grid size in 256-thread blocks per CU (1..64).  Up to 8 (4 for the 108-VGPR
                           // quad kernel) are resident; more = later blocks start as earlier ones end, i.e.
                           // the hardware dispatcher balances the load (Reddit-shaped, k=128: 3.96 ms at 8,
                           // 3.68 ms at 32).  Less than the resident count leaves wave slots and registers
                           // free for a concurrent kernel (the RCCL all-gather).
};

hipError_t launch_plan_chunk_rows(const int* rowptr, int m, int T, int nchunks,
                                  int* chunk_row, hipStream_t s);
// rows r with rowptr[r] == rowptr[r+1]: *count_dev += their number (count_dev zeroed by the caller)
hipError_t launch_count_empty_rows(const int* rowptr, int m, int* count_dev, hipStream_t s);
// C[r, :] = act((accumulate ? C[r, :] : 0) + bias) for every EMPTY row r — what the main kernels leave out
hipError_t launch_fill_empty_rows(const int* rowptr, float* C, const float* bias, int relu, int accumulate, int m, int k,
                                  hipStream_t s);

hipError_t launch_spmm(const SpmmArgs& a, int cu_count, hipStream_t s);
hipError_t launch_gather_rows(float* dst, const float* src, const int* idx, int nrows, int k,
                              hipStream_t s);
// dst[r, 0:k] = src[r, 0:k], dst[r, k:ld] = 0 for r < rows (dst row stride ld >= k)
hipError_t launch_pad_rows(float* dst, const float* src, long long rows, int k, int ld, hipStream_t s,
                           const float* rowscale = nullptr);   // dst[r, :] = rowscale[r] * src[r, :] when given
// dst[r, 0:k] = act(src[r, 0:k] + bias), src row stride ld >= k
hipError_t launch_unpad_rows(float* dst, const float* src, const float* bias, int relu, long long rows, int k,
                             int ld, hipStream_t s, const int* guard = nullptr);   // guard: skip when *guard == 0
int pick_vec(int k, int tile_cols, const void* B, const void* C, const void* P);

// which main kernel a launch_spmm with these arguments runs (the one rule: the launch switches on it, the plan API's
// reports ask it), and its name.  refused: what launch_spmm answers with hipErrorInvalidValue — a value-free or 16-bit
// column stream handed to a kernel that is not built for it.
enum class ChunkFamily { empty, quad, narrow, narrow16_dpp, chunk, refused };
struct ChunkChoice {
  ChunkFamily family;
  int lanes;                             // lanes per non-zero: quad 4 / 16, narrow G = 4 / 8 / 16, chunk 64
  int vec, U;                            // floats per lane and gather; gather instructions per batch
  bool epi, buf, valless, col16;         // template flags: fused epilogue, buffer addressing, no values, 16-bit columns
};
ChunkChoice spmm_chunk_choice(const SpmmArgs& a);
void spmm_chunk_kernel_name(const ChunkChoice& c, char* buf, size_t len);
// the fifteen leading arguments of every chunk-schedule main kernel
#define GCN_CHUNK_ARGS(a) (a).rowptr, (a).col, (a).val, (a).B, (a).C, (a).P, (a).chunk_row, (a).bias, (a).nnz_dev, \
                          (a).relu, (a).nchunks, (a).T, (a).m, (a).nnz, (a).k

// spmm_narrow.hip — k <= 16: several non-zeros per gather instruction (c: a narrow or narrow16_dpp choice)
hipError_t launch_spmm_narrow(const SpmmArgs& a, const ChunkChoice& c, int nblocks, hipStream_t s);

// spmm_quad.hip — 64-column tile, four non-zeros per 16-byte-per-lane gather instruction (c: a quad choice)
bool spmm_quad_eligible(const SpmmArgs& a);
hipError_t launch_spmm_quad(const SpmmArgs& a, const ChunkChoice& c, int nblocks, hipStream_t s);

// spmm_group.hip — sliced main pass, four independent 16-lane row engines per wave (the walk itself: group_walk.h)
struct GroupArgs {
  const unsigned short* stream;  // [nchunks*T]: bits 0..14 column offset inside the slice, bit 15 = row end
  const float* vals = nullptr;   // [nchunks*T] matrix values in stream order (0 at padding entries); nullptr: every entry counts 1
  const int* chunk_meta;         // int2 [nchunks]: {2 * (virtual row holding entry c*T) + (it began in an earlier chunk),
                                 //                  first row of the chunk's slice in Bp}
  const void* Bp;                // the table: scaled copy of B, slice s at rows [s*(w+1), (s+1)*(w+1)), row w all zero
  int elem_bytes = 4;            // ... of fp32 (4) or bf16 (2: k % 8 == 0, ldb % 8 == 0, no dyn; walked 128 columns per tile)
  float* Cv;                     // partial outputs [S*m x k]
  float* P;                      // partial slab [2*nchunks x k]
  int nchunks, T, k, ldb;        // T = entries per chunk (of ONE 16-lane group), ldb = row stride of Bp in elements (0 = k)
  const int* dyn = nullptr;      // drop-in flexspmm: device words {buffers recognised, chunk count, cut rows}; nchunks is then an
                                 // upper bound that sizes the grid (dropin_guard_kernel, api_dropin.cpp)
  long long table_rows = 0;      // rows of Bp, S * (w + 1): decides 32-bit or 64-bit (BIG) slice-base addressing
  int narrow8 = 1;               // k <= 32 on the eight-engine kernel (spmm_group8_kernel) when nchunks % 64 == 0
  int narrow12 = 1;              // 33 <= k <= 48, value-free: the five-engine kernel (spmm_group12_kernel)
  // (partial rows leave with non-temporal stores, finished rows of the value-free pass through the LDS ring, every
  //  64-column tile in one launch: the alternatives were measured in round 2 and are no longer built)
};
bool spmm_group_eligible(int k, int ldb, long long table_rows, const void* B, const void* C, const void* P);
bool spmm_group_needs_big(long long table_rows, long long row_bytes);
hipError_t launch_spmm_group(const GroupArgs& a, hipStream_t s);      // the single entry: every format, every kernel
// grid and order of one group launch (group_grid, spmm_group.hip)
struct GroupGrid { int blocks_per_tile, nblocks, stream_nt, seg_blocks; };
// spmm_group_bf16.hip holds the bf16 instantiations of the walk; launch_spmm_group has checked the arguments
hipError_t launch_group_walk_bf16(const GroupArgs& a, int ld, const GroupGrid& g, bool big, hipStream_t s);
// which kernel a launch with this shape runs (the one rule: the launch and the plan API's report ask it), and its name
enum class GroupEngine { four16, eight8, five12 };                   // engines x lanes of a wave
struct GroupChoice { GroupEngine engine; bool weighted, big, bf16; };
GroupChoice spmm_group_choice(const GroupArgs& a);
void spmm_group_kernel_name(const GroupChoice& c, char* buf, size_t len);
bool group8_enabled();                  // GCN_AMD_GROUP8=0: k <= 32 on the 64-column group pass (what GroupArgs::narrow8 is set from)
// the slice-major 15-bit stream the group kernel walks (S slices of width w = ceil(n/S) <= 32767): every virtual
// row gets >= 1 entry, every slice is padded to whole chunks and the total to a multiple of 32 chunks with
// entries that gather the slice's zero row.  Outputs: vrowptr_g [S*m+1] (caller-allocated; the fix-up pass needs
// it), *stream_out, *chunk_row_out [nchunks] and *chunk_meta_out (int2 [nchunks], see GroupArgs) — allocated here,
// the caller frees —, *nchunks_host.
// *fix_out (int4 [*nfix_host], allocated here): the rows whose pieces lie in the partial slab, see launch_group_fixup.
// vval + vals_out (optional): the slice-major values are laid out beside the stream (*vals_out [nchunks*T], 0 at padding).
hipError_t build_group_stream(const int* vrowptr, const int* vcol, int m, int n, int S, int T, int* vrowptr_g,
                              unsigned short** stream_out, int** chunk_row_out, int** chunk_meta_out,
                              int* nchunks_host, int** fix_out, int* nfix_host, hipStream_t st,
                              const float* vval = nullptr, float** vals_out = nullptr,
                              int** cutptr_out = nullptr, int** cutchunk_out = nullptr, int* ncut_host = nullptr);
// cutptr_out / cutchunk_out / ncut_host (optional; allocated here): the same cut rows keyed by OUTPUT row, for the slice
// reduction — pieces cutchunk[cutptr[r] .. cutptr[r+1]) (chunk numbers; the piece of chunk c is P[2c]) belong to row r.
// Cv[row, :] += the row's head pieces in the partial slab P, in chunk order, for every row of the list (k % 4 == 0)
// dyn (drop-in flexspmm): nfix is an upper bound, the count is dyn[2] and nothing runs when dyn[0] == 0
hipError_t launch_group_fixup(const int* fix, int nfix, const float* P, float* Cv, int k, hipStream_t s,
                              const int* dyn = nullptr);
// dst[(c / w)*(w+1) + c % w, :] = rowscale[c] * src[c, :] (rowscale nullptr: 1; row stride ld >= k, padding columns zero), row w of
// every slice zero: the layout GroupArgs::Bp describes
hipError_t launch_scale_rows_sliced(float* dst, const float* src, const float* rowscale, int n, int k, int ld,
                                    int S, int w, hipStream_t s);

// sddmm.hip — out[e] = sum_j A[row(e), j] * B[col(e), j] for every stored entry, in CSR order.  Chunks of T entries of a
// CSR (the caller's, vsrc = nullptr) or of a plan's slice-major virtual CSR (rows = S*m; vsrc[vr] = CSR position of the
// first entry of virtual row vr; A row vr % m).  A [m x k] and B [n x k] row-major fp32.
struct SddmmArgs {
  const int *rowptr = nullptr, *col = nullptr, *chunk_row = nullptr, *vsrc = nullptr;
  const float *A = nullptr, *B = nullptr;
  float* out = nullptr;
  int rows = 0, m = 0, nnz = 0, T = 0, nchunks = 0, k = 0;
};
hipError_t launch_sddmm(const SddmmArgs& s, hipStream_t st);
bool sddmm_vec(const float* A, const float* B, int k);   // 16-byte loads (k % 4 == 0, aligned operands)

// edge_softmax.hip — softmax over the stored entries of each CSR row, its backward, the fused GAT-score forms and CSR row
// sums, for one head ([nnz] arrays) and for H heads in one pass ([nnz, H] arrays with an entry's heads contiguous, per-node
// scalars [rows, H]; nnz * H < 2^31) (plan-free, capturable, no atomics: see the file's header).  The one-head launchers
// are the H = 1 case of the _heads ones.  ws: edge_workspace_bytes(nnz, H) bytes of device memory — a flag and one partial
// per (chunk of kEdgeChunk entries, long row, head) — owned by the call while it runs.
constexpr int kEdgeChunk = 8192;
size_t edge_workspace_bytes(int nnz, int H = 1);
hipError_t launch_edge_softmax(const int* rowptr, int m, int nnz, const float* s, float* p, void* ws, hipStream_t st);
hipError_t launch_edge_softmax_backward(const int* rowptr, int m, int nnz, const float* p, const float* g, float* ds, void* ws,
                                        hipStream_t st);
hipError_t launch_gat_edge_softmax(const int* rowptr, const int* col, int m, int nnz, const float* a_dst, const float* a_src,
                                   float slope, float* p, void* ws, hipStream_t st);
hipError_t launch_gat_edge_softmax_backward(const int* rowptr, const int* col, int m, int nnz, const float* a_dst,
                                            const float* a_src, float slope, const float* p, const float* g, float* ds,
                                            float* grad_a_dst, void* ws, hipStream_t st);
hipError_t launch_segment_sum(const int* rowptr, int m, int nnz, const float* x, const int* perm, float* out, void* ws,
                              hipStream_t st);
hipError_t launch_edge_softmax_heads(const int* rowptr, int m, int nnz, int H, const float* s, float* p, void* ws, hipStream_t st);
hipError_t launch_edge_softmax_heads_backward(const int* rowptr, int m, int nnz, int H, const float* p, const float* g, float* ds,
                                              void* ws, hipStream_t st);
hipError_t launch_gat_edge_softmax_heads(const int* rowptr, const int* col, int m, int nnz, int H, const float* a_dst,
                                         const float* a_src, float slope, float* p, void* ws, hipStream_t st);
hipError_t launch_gat_edge_softmax_heads_backward(const int* rowptr, const int* col, int m, int nnz, int H, const float* a_dst,
                                                  const float* a_src, float slope, const float* p, const float* g, float* ds,
                                                  float* grad_a_dst, void* ws, hipStream_t st);
hipError_t launch_segment_sum_heads(const int* rowptr, int rows, int nnz, int H, const float* x, const int* perm, float* out,
                                    void* ws, hipStream_t st);

// aggregate.hip — element-wise max / min over each CSR row's stored entries with the winning entry index, and its backward
// as a walk of the transposed pattern (plan-free, capturable, no atomics: see the file's header).  x / out / g / gx are
// fp32 or bf16 (bf16 != 0) row-major with row stride k.  ws: aggregate_workspace_bytes(nnz, k) bytes of device memory — a
// flag and one (value, entry) pair per (chunk of kAggChunk entries, long row, column) — owned by the call while it runs.
constexpr int kAggChunk = 4096;
constexpr int kAggMax = 0, kAggMin = 1;                // GCN_REDUCE_MAX / GCN_REDUCE_MIN
size_t aggregate_workspace_bytes(int nnz, int k);
hipError_t launch_aggregate(const int* rowptr, const int* col, int m, int nnz, const void* x, int bf16, int k, int op, void* out,
                            int* arg, void* ws, hipStream_t st);
hipError_t launch_aggregate_backward(const int* trowptr, const int* trow, const int* tperm, int n, int nnz, const void* g, int bf16,
                                     const int* arg, int k, void* gx, void* ws, hipStream_t st);

// multihead.hip — the gather primitives of multi-head attention, H heads in one pass: the head-weighted SpMM and the
// per-head SDDMM (plan-free, capturable, no atomics: see the file's header).  Per-entry arrays are [nnz, H] with an entry's
// heads contiguous, node arrays [rows, H * F] with k = H * F; nnz * H < 2^31.  ws: heads_spmm_workspace_bytes /
// kHeadsSddmmWsBytes of device memory (a flag and the long rows' chunk partials).
size_t heads_spmm_workspace_bytes(int nnz, int k);
constexpr size_t kHeadsSddmmWsBytes = 16;
hipError_t launch_spmm_heads(const int* rowptr, const int* idx, const int* perm, int rows, int nnz, int H, int k, const float* vals,
                             const float* x, float* out, void* ws, hipStream_t st);
hipError_t launch_sddmm_heads(const int* rowptr, const int* col, int m, int nnz, int H, int k, const float* a, const float* b,
                              float* out, void* ws, hipStream_t st);
// the GATv2 score s[e, h] = sum_j att[h, j] leaky_relu(h_dst[row(e), hF + j] + h_src[col[e], hF + j]) on the SDDMM's walk (ws:
// kHeadsSddmmWsBytes will do) and its backward on one side on the SpMM's walk: grad_own [rows, k] and, where act_sums is not
// null, act_sums [rows, k] whose column sums are grad_att.  ws: gatv2_workspace_bytes (a flag, the chunk partials of two sums).
size_t gatv2_workspace_bytes(int nnz, int k);
hipError_t launch_gatv2_scores(const int* rowptr, const int* col, int m, int nnz, int H, int k, const float* h_dst, const float* h_src,
                               const float* att, float slope, float* out, void* ws, hipStream_t st);
hipError_t launch_gatv2_scores_backward(const int* rowptr, const int* idx, const int* perm, int rows, int nnz, int H, int k,
                                        const float* own, const float* other, const float* att, float slope, const float* g,
                                        float* grad_own, float* act_sums, void* ws, hipStream_t st);

// sample.hip — uniform neighbour sampling without replacement from the rows of seeds[n_seeds], a pure function of (seed,
// offset, entry index) (plan-free, no global atomics: see the file's header and include/gcn_spmm.h).  fanout < 0: every entry.
// out_rowptr [n_seeds + 1] is an INPUT (row i holds min(row length, fanout) entries); ws: kSampleWsBytes of device memory (a
// flag).  A row of more than kSampleLongRow entries gets a 256-thread workgroup instead of a wave.
constexpr int kSampleLongRow = 2048;
constexpr size_t kSampleWsBytes = 16;
hipError_t launch_sample_neighbors(const int* rowptr, const int* col, int m, int nnz, const int* seeds, int n_seeds, int fanout,
                                   unsigned long long seed, unsigned long long offset, const int* out_rowptr, int* out_col,
                                   int* out_eid, void* ws, hipStream_t st);

// subgraph.hip — the vertex-induced subgraph of nodes[n_nodes] (count, the caller's scan, fill) and uniform random walks
// (plan-free, no global atomics: see the file's header and include/gcn_spmm.h).  vmap [n]: a vertex's position in nodes or
// -1; out_rowptr [n_nodes + 1] is an INPUT of the fill; ws: kSubgraphWsBytes of device memory (a flag).  Rows of more than
// kSampleLongRow entries get a 256-thread workgroup instead of a wave.  out_walks [length + 1][n_walks].
constexpr size_t kSubgraphWsBytes = 16;
hipError_t launch_induced_subgraph_count(const int* rowptr, const int* col, int m, int nnz, const int* nodes, int n_nodes,
                                         const int* vmap, int* out_len, void* ws, hipStream_t st);
hipError_t launch_induced_subgraph_fill(const int* rowptr, const int* col, int m, int nnz, const int* nodes, int n_nodes,
                                        const int* vmap, const int* out_rowptr, int* out_col, int* out_eid, void* ws,
                                        hipStream_t st);
hipError_t launch_random_walk(const int* rowptr, const int* col, int m, int nnz, const int* starts, int n_walks, int length,
                              unsigned long long seed, unsigned long long offset, int* out_walks, hipStream_t st);

// lookup.hip — the entry index of (q_rows[i], q_cols[i]) in a CSR with column-sorted rows, or -1, and num_neg columns per
// query row that the row does not store (a pure function of (seed, offset, slot); slots = n_queries * num_neg): one lane per
// query / slot, no workspace, no atomics (see the file's header and include/gcn_spmm.h).
hipError_t launch_find_entries(const int* rowptr, const int* col, int m, int nnz, const int* q_rows, const int* q_cols,
                               int n_queries, int* out_eid, hipStream_t st);
hipError_t launch_negative_sample(const int* rowptr, const int* col, int m, int n, int nnz, const int* q_rows, int slots,
                                  int num_neg, int max_tries, int exclude_self, unsigned long long seed,
                                  unsigned long long offset, int* out_cols, hipStream_t st);

// construct.hip — stable bucketing of the indices 0 .. count - 1 by an int key in [0, nbuckets) (count, the caller's scan,
// fill) and the gather that turns the bucketing of a CSR's entries by column into its transpose (see the file's header and
// include/gcn_spmm.h).  A bucket of at most kBucketWaveMax entries is ordered by a wave, one of at most kBucketBlockMax by a
// workgroup in LDS, a longer one by a workgroup in place.  ws: bucket_workspace_bytes(count, nbuckets) of device memory.
constexpr int kBucketWaveMax = 256;
constexpr int kBucketBlockMax = 8192;
size_t bucket_workspace_bytes(int count, int nbuckets);
hipError_t launch_bucket_count(const int* keys, int count, int nbuckets, int* offsets, hipStream_t st);
hipError_t launch_bucket_fill(const int* keys, int count, int nbuckets, const int* offsets, int* perm, void* ws, hipStream_t st);
hipError_t launch_transpose_gather(const int* rowptr, int m, int nnz, const int* perm, const float* val, int* trow, float* tval,
                                   hipStream_t st);

// coalesce.hip — merging the runs of equal columns of a CSR's rows (count, the caller's scan, fill), with the diagonal
// dropped, filled or added to on the way, and the two kernels of the normalisation: row sums in fp64 and the scaled values
// (plan-free, no global atomics: see the file's header and include/gcn_spmm.h).  out_rowptr [m + 1] is an INPUT of the
// fill; ws: kCoalesceWsBytes of device memory (a flag).  Rows of more than kSampleLongRow entries get a 256-thread workgroup
// instead of a wave, in all four.
constexpr size_t kCoalesceWsBytes = 16;
constexpr int kCoalesceSum = 0, kCoalesceMax = 1, kCoalesceMin = 2, kCoalesceFirst = 3;      // GCN_COALESCE_*
constexpr int kDiagKeep = 0, kDiagDrop = 1, kDiagFill = 2, kDiagAdd = 3;                     // GCN_DIAG_*
constexpr int kNormSym = 0, kNormRow = 1;                                                    // GCN_NORM_*
hipError_t launch_csr_coalesce_count(const int* rowptr, const int* col, int m, int n, int nnz, int diagonal, int* out_len,
                                     void* ws, hipStream_t st);
hipError_t launch_csr_coalesce_fill(const int* rowptr, const int* col, const float* val, int m, int n, int nnz, int reduce,
                                    int diagonal, float diag_value, const int* out_rowptr, int* out_col, float* out_val,
                                    int* out_first, int* seg, void* ws, hipStream_t st);
hipError_t launch_csr_degree(const int* rowptr, const float* val, int m, int nnz, double* deg, hipStream_t st);
hipError_t launch_csr_normalize(const int* rowptr, const int* col, const float* val, int m, int n, int nnz, const double* deg,
                                int mode, float* out_val, hipStream_t st);

// spgemm.hip — C = A * B of two CSR matrices (count, the caller's scan, fill): row-wise Gustavson with the products of an
// entry added in A's entry order (plan-free, no floating-point atomics: see the file's header and include/gcn_spmm.h).
// A [m x p], B [p x n]; a row of at most kSpgemmWaveMax possible columns is taken by a wave with a table in LDS, one of at
// most kSpgemmBlockMax by a 256-thread workgroup with a table in LDS, a longer one by one of kSpgemmDenseBlocks workgroups
// with a dense accumulator in the workspace.  out_rowptr [m + 1] is an INPUT of the fill; ws: spgemm_workspace_bytes(m, n).
constexpr int kSpgemmWaveMax = 512;
constexpr int kSpgemmBlockMax = 8192;
constexpr int kSpgemmDenseBlocks = 16;
size_t spgemm_workspace_bytes(int m, int n);
hipError_t launch_spgemm_count(const int* a_rowptr, const int* a_col, int m, int p, int nnz_a, const int* b_rowptr,
                               const int* b_col, int n, int nnz_b, int* out_len, void* ws, hipStream_t st);
hipError_t launch_spgemm_fill(const int* a_rowptr, const int* a_col, const float* a_val, int m, int p, int nnz_a,
                              const int* b_rowptr, const int* b_col, const float* b_val, int n, int nnz_b,
                              const int* out_rowptr, int* out_col, float* out_val, void* ws, hipStream_t st);

// sampled_dot.hip — the product of two CSR matrices sampled on a pattern: out[e] for the entry e = (i, j) of P is the dot
// product of X's row i (x_by_col: j) and Y's row j (x_by_col: i) over their common columns in [0, w), the products added in
// X's entry order; Y's rows ascend strictly (plan-free, no atomics: see the file's header and include/gcn_spmm.h).  A wave per
// row of P, a 256-thread workgroup per row of more than kSampleLongRow entries; ws: kSampledDotWsBytes (a flag).
constexpr size_t kSampledDotWsBytes = 16;
hipError_t launch_csr_sampled_dot(const int* p_rowptr, const int* p_col, int mp, int np, int nnz_p, const int* x_rowptr,
                                  const int* x_col, const float* x_val, int nnz_x, const int* y_rowptr, const int* y_col,
                                  const float* y_val, int nnz_y, int w, int x_by_col, float* out, void* ws, hipStream_t st);

// knn.hip — brute-force k nearest neighbours of fp32 rows by squared Euclidean distance (plan-free, no floating-point
// atomics: see the file's header and include/gcn_spmm.h).  A 256-thread workgroup owns kKnnTileQ queries and streams its part
// of the candidates through in tiles of kKnnTileC; `eff_splits` = knn_effective_splits(...) parts per query block, merged by
// a second kernel.  ws: knn_workspace_bytes(q, k, eff_splits), 8-byte aligned.
constexpr int kKnnKMax = 64;
constexpr int kKnnTileQ = 64;
constexpr int kKnnTileC = 64;
int knn_auto_splits(int q, int n, int cus);            // plan_policy.cpp
int knn_effective_splits(int q, int n, int splits, int cus);
size_t knn_workspace_bytes(int q, int k, int eff_splits);
hipError_t launch_knn(const float* x, long long ldx, const float* y, long long ldy, int q, int n, int d, int k, int self_offset,
                      int eff_splits, int* out_idx, float* out_dist2, double* out_sum, void* ws, hipStream_t st);

// slicing.hip — mutable values.  vsrc[s*m + r] = CSR position of the first entry of row r in slice s (from the sliced
// row pointer; column-sorted rows make every (row, slice) part one contiguous run of the CSR row).
hipError_t build_value_map(const int* rowptr, const int* vrowptr, int m, int S, int* vsrc, hipStream_t st);
// new CSR-order values into the sliced copy (vval, slice-major) and, when gvals is set, into the group stream's values
// (position group_phys(vrowptr_g[vr] + i)); padding entries keep their zero.  One wave per virtual row, no allocation.
hipError_t launch_refresh_values(const int* vrowptr, const int* vsrc, const int* vrowptr_g, int m, int S, const float* val,
                                 float* vval, float* gvals, hipStream_t st);

// spmm_group_bf16.hip — bf16 feature operands, fp32 accumulation: the element-wise passes around the walk.
// the bf16 table: rowscale nullptr copies the bits (weighted pass), else bf16(rowscale[c] * src[c, :]) with one RNE rounding
hipError_t launch_relay_bf16_sliced(unsigned short* dst, const unsigned short* src, const float* rowscale, int n, int k, int ld,
                                    int S, int w, hipStream_t s);
hipError_t launch_bf16_to_f32(float* dst, const unsigned short* src, long long count, hipStream_t st);
hipError_t launch_f32_to_bf16(unsigned short* dst, const float* src, long long count, hipStream_t st);
hipError_t launch_dropout_bf16(unsigned short* dst, const unsigned short* src, long long count, const DropoutSpec& drop,
                               hipStream_t st);

// spmm_panel.hip — LDS-staged feature tiles per row panel (near-diagonal matrices)
// cnt_dev (optional, [panels]): in-window non-zeros of every panel
hipError_t panel_plan(const int* rowptr, const int* col, int m, int n, int R, int* w0_dev,
                      unsigned long long* inside_host, hipStream_t st, int* cnt_dev = nullptr);
// dense_slot (optional, [panels]): slot of the panel's dense tile, -1 for an ordinary panel; the in-window entries of
// dense panels go into `adense` (MFMA fragment order, 128 x 512 floats per slot, zeroed by the caller) instead
hipError_t panel_split(const int* rowptr, const int* col, const float* val, const int* w0_dev, int m,
                       int R, int* in_rowptr, int* out_rowptr, int* in_off, float* in_val,
                       int* out_col, float* out_val, int* nnz_in_host, hipStream_t st,
                       const int* dense_slot = nullptr, float* adense = nullptr);
hipError_t launch_panel_in(const int* in_rowptr, const int* in_off, const float* in_val, const float* B,
                           float* C, const int* panel_w0, int m, int n, int k, int R, int tile,
                           hipStream_t s, const int* dense_slot = nullptr);
hipError_t launch_panel_dense(const float* adense, const int* dense_panel, int ndense, const float* B, float* C,
                              const int* panel_w0, int m, int n, int k, int R, int tile, hipStream_t s);
hipError_t launch_panel_epilogue(float* C, const float* bias, int relu, int m, int k, hipStream_t s);

// reorder_device.hip — degree / RCM orderings and the CSR rewrite on the device (same integers as reorder.cpp)
hipError_t device_order_deg(const int* rowptr, const int* col, int n, int nnz, int which, int desc,
                            int* rank_out, hipStream_t st);
hipError_t device_order_rcm(const int* rowptr, const int* col, int n, int nnz, int* rank_out,
                            int* levels_out, hipStream_t st);
hipError_t device_csr_apply_rank(const int* rowptr, const int* col, const float* val, const int* rank, int n,
                                 int nnz, int* out_rowptr, int* out_col, float* out_val, int* vomp_out,
                                 int* bad_rank_host, hipStream_t st);

// rabbit_device.hip — Rabbit ordering by parallel incremental aggregation (Arai et al., IPDPS 2016; renumber.cu:328-330);
// rowptr/col: SYMMETRIC pattern (self-loops ignored); stats_host[4] = {communities, passes, retried, left top-level}
hipError_t device_order_rabbit(const int* rowptr, const int* col, int n, int nnz, int* rank_out_dev, int* community_out_dev,
                               long long* stats_host, hipStream_t st);

// slicing.hip
// 16-bit column stream of a sliced CSR (S <= 8, slice width <= 65 535): every slice padded to a multiple of T
// with 0xFFFF markers; vrowptr16 [S*m+1] (the last row of a slice owns its markers), col16 [*nnz16_host],
// start_host[S+1] = where each slice starts in the padded stream.  col16 is allocated here (caller frees).
hipError_t build_col16_stream(const int* vrowptr, const int* vcol, int m, int n, int S, int T, int* vrowptr16,
                              unsigned short** col16_out, int* nnz16_host, int* start_host, hipStream_t st);
hipError_t build_sliced_csr(const int* rowptr, const int* col, const float* val, int m, int n,
                            int nnz, int S, int* vrowptr, int* vcol, float* vval,
                            int* sorted_out, hipStream_t st);
// rows of the group kernels' stream cut by chunk ends, per output row (build_group_stream): the reduction adds the pieces
// P[2 * chunk[q]], q in [ptr[r], ptr[r+1]), behind the S partial rows of row r — the fix-up pass folded into the reduction
struct CutLists {
  const int* ptr = nullptr;      // [m+1]; null: no pieces to add
  const int* chunk = nullptr;    // [ptr[m]]
  const float* P = nullptr;      // the piece slab of the launch (GroupArgs::P)
};
// One slice reduction: C[r, :] = dropout(act(rowscale[r] * (sum_s Cv[s*m + r, :] + the row's cut pieces) + bias)), the
// partial rows added in slice order, then the pieces in chunk order.
constexpr int kDtypeF32 = 0, kDtypeBf16 = 1;          // GCN_DTYPE_F32 / GCN_DTYPE_BF16
struct SliceReduce {
  const float* Cv = nullptr;         // partial rows [S*m x k]
  void* C = nullptr;                 // [m x k] of c_dtype; bf16: the same sums and epilogue, one RNE rounding at the end
  int c_dtype = kDtypeF32;
  const float* bias = nullptr;       // [k] or null
  int relu = 0, m = 0, S = 0, k = 0;
  const float* rowscale = nullptr;   // [m] or null: the row factor u_row of a value-free pass
  DropoutSpec drop;
  const int* guard = nullptr;        // device word; the kernel does nothing when *guard == 0 (drop-in flexspmm)
  const float* outscale = nullptr; int gap_w = 0;   // pre-laid output: row r lands in row r + r / gap_w, times outscale[r]
  CutLists cuts;
};
// the one kernel rule (slicing.hip).  A bf16 result needs k % 4 == 0, aligned Cv and cuts.P, no guard and no pre-laid output
// (else hipErrorInvalidValue); its kernel is in spmm_group_bf16.hip, launched through enqueue_slice_reduce_bf16 once checked.
hipError_t launch_slice_reduce(const SliceReduce& r, hipStream_t st);
hipError_t enqueue_slice_reduce_bf16(const SliceReduce& r, int nblocks, int vec_out, hipStream_t st);
// dst[i] = dropout(src[i]) for i < total, mask from the flat index i (dst may be src)
hipError_t launch_dropout(float* dst, const float* src, long long total, const DropoutSpec& drop, hipStream_t st);
// values factor as u[r]*u[c]?  u_out[n] (device), *ok_host = 1 when every stored entry matches within 4 ulp
hipError_t verify_value_factors(const int* rowptr, const int* col, const float* val, const float* u_row,
                                const float* u_col, int m, int* ok_host, hipStream_t st);
hipError_t detect_rank1_values(const int* rowptr, const int* col, const float* val, int n, float* u_out,
                               int* ok_host, hipStream_t st);
// values that depend on the row only (mode 1: u_col = 1) or on the column only (mode 2: u_row = 1)?
hipError_t detect_constant_values(const int* rowptr, const int* col, const float* val, int m, int n, int nnz, int mode,
                                  float* u_row_out, float* u_col_out, int* ok_host, hipStream_t st);

}  // namespace gcn
