/*
 * gcn_spmm.h — C ABI of libgcnspmm.so, the MI355X (gfx950) GCN aggregation library.
 *
 * Everything here is `extern "C"`, plain pointers and sizes; no torch types.
 * Two groups of entry points:
 *
 *  (1) NATIVE API (gcn_*): what the Python host layer (gcn_amd/) binds.  Explicit
 *      stream, explicit status codes, cached plan object.
 *  (2) DROP-IN API: the exact symbols / signatures the reference's ctypes call
 *      sites bind (pygcn/gcn6.py:21-25).  They are exported both from
 *      libgcnspmm.so and from five tiny shared objects that carry the reference's
 *      file names (flexspmm.so, cuspmm.so, tile.so, permutate.so, renumber.so),
 *      so that gcn6.py loads them unchanged.  See INTEGRATION.md.
 *
 * Each declaration cites the reference interface it replaces (file:line under
 * the reference tree guohaoqiang/gcn @ v1).
 */
#ifndef GCN_SPMM_H
#define GCN_SPMM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- */
/* status codes (native API).  The reference has no error convention at all   */
/* (void functions, cuspmm.cu:3-21 only prints) — the drop-in symbols keep    */
/* `void`, print ONE line to stderr and return with the caller's outputs      */
/* untouched (section (2) below): never silent, never fatal.                  */
/* ------------------------------------------------------------------------- */
#define GCN_OK                 0
#define GCN_ERR_INVALID_ARG    1
#define GCN_ERR_HIP            2
#define GCN_ERR_NO_DEVICE      3
#define GCN_ERR_CAPACITY       4   /* caller buffer too small for the packed plan */
#define GCN_ERR_ALLOC          5
#define GCN_ERR_NOT_FACTORED   6   /* set_value_factors: some stored entry is not u_row[r]*u_col[c]; the plan keeps its value stream */
#define GCN_ERR_INTERNAL       7   /* a consistency guard inside the library tripped (gcn_order_rabbit_device: stats_host[4..7]); outputs not written */

const char* gcn_status_string(int status);
/* library version, "major.minor.patch" */
const char* gcn_version(void);
/* number of compute units of the current device (replaces the per-call
 * cudaGetDeviceProperties of flexspmm.cu:506-508 / tile.cu:118-122); <0 on error */
int gcn_device_cu_count(void);

/* ------------------------------------------------------------------------- */
/* (1a) SpMM plan + launch:   C[m x k] = A[m x n, CSR fp32] * B[n x k]        */
/*      replaces  cuspmm()   cuspmm.cu:23-68   (the math: op(A)=A, op(B)=B,   */
/*                row-major B and C, alpha=1, beta=0)                         */
/*      and       flexspmm() flexspmm.cu:499-544 (the launcher + 5 kernels)   */
/* ------------------------------------------------------------------------- */
typedef struct gcn_spmm_plan gcn_spmm_plan_t;

/* Build the per-graph schedule (equal-nnz chunks + first row of each chunk) on
 * the device.  `rowptr_dev` is the int32 CSR row pointer [m+1] in device memory;
 * it is only read during this call (the call synchronises `stream` before it returns).  `chunk_nnz` = 0 picks a size automatically
 * (multiple of 64).  The plan owns a small device buffer and a grow-only
 * workspace for the partial sums of rows that straddle chunk boundaries. */
int gcn_spmm_plan_create(gcn_spmm_plan_t** plan, const int32_t* rowptr_dev,
                         int32_t m, int32_t n, int32_t nnz, int32_t chunk_nnz,
                         void* stream);
int gcn_spmm_plan_destroy(gcn_spmm_plan_t* plan);
/* introspection (tests, bench) */
int32_t gcn_spmm_plan_num_chunks(const gcn_spmm_plan_t* plan);
int32_t gcn_spmm_plan_chunk_nnz(const gcn_spmm_plan_t* plan);
/* bytes of workspace the plan needs for feature width k */
size_t  gcn_spmm_plan_workspace_bytes(const gcn_spmm_plan_t* plan, int32_t k);

/* C = A*B.  All pointers are device pointers; C is fully overwritten (no need
 * to pre-zero, unlike gcn6.py:37).  Asynchronous on `stream` (NULL = the legacy
 * default stream, which is what the reference launches on, flexspmm.cu:512).
 * Deterministic: no atomics, each row is summed in CSR order within a chunk
 * and chunk partials are added in chunk order.
 * Stream capture: the first call for a width allocates the plan's workspaces
 * (and builds the streams of a sliced plan); every later call with the same width
 * only enqueues kernels on `stream`, so it can be captured in a HIP graph and
 * replayed on new operand contents (tests/test_spmm_gpu.py,
 * test_spmm_can_be_captured_in_a_hip_graph_and_replayed).
 * Non-finite features (every entry point below, fp32 and bf16, every plan shape; tests/test_nonfinite_gpu.py): a NaN or
 * +-Inf in B[c, j] reaches exactly the C[i, j] whose row i stores column c, and every other element keeps the bits it has
 * without it.  The class of a reached element — NaN, +Inf or -Inf — is that of the IEEE sum of the row's products in any
 * order.  In the fused epilogues a ReLU keeps NaN (as torch.relu does) and maps -Inf to 0, and a dropped element is 0
 * whatever it held.  Outside the contract: a stored zero in A (0 * Inf is NaN by IEEE; dense panels skip zeros), and, inside
 * a dense panel's window, repeated entries of one (row, column), which are multiplied as their sum. */
int gcn_spmm_csr_f32(gcn_spmm_plan_t* plan,
                     const int32_t* rowptr_dev, const int32_t* col_dev,
                     const float* val_dev, const float* B_dev, float* C_dev,
                     int32_t k, void* stream);

/* Same, plus a fused epilogue  C = act(A*B + bias)  (bias may be NULL;
 * relu = 0/1).  Covers gcn6.py:141-142,245 (bias add, ReLU) — SURVEY §8(f).1 */
int gcn_spmm_csr_f32_bias_relu(gcn_spmm_plan_t* plan,
                     const int32_t* rowptr_dev, const int32_t* col_dev,
                     const float* val_dev, const float* B_dev, float* C_dev,
                     const float* bias_dev, int32_t relu,
                     int32_t k, void* stream);

/* The full fused epilogue of a GCN layer (pygcn/gcn6.py:141-142, 245-246: bias add, ReLU and
 * dropout are three separate PyTorch ops there):  C = dropout(act(A*B + bias)).  dropout_p in [0, 1) is the drop
 * probability (0 = none); kept elements are scaled by 1/(1-p).  The mask is NOT stored: element i = r*k + c is kept
 * iff word (i mod 4) of Philox4x32-10(counter = (i / 4, offset), key = seed) >= p * 2^32, so the backward pass
 * regenerates it with gcn_dropout_f32 on the gradient (same p, seed, offset) and every kernel family agrees.  Where
 * the plan has an epilogue pass (column slicing: the slice reduction) the mask rides in it; otherwise one in-place
 * pass over C applies it.  (torch's own dropout stream cannot be reproduced: the semantic — Bernoulli(1-p), scaled
 * — is what is matched.) */
int gcn_spmm_csr_f32_epilogue(gcn_spmm_plan_t* plan,
                     const int32_t* rowptr_dev, const int32_t* col_dev,
                     const float* val_dev, const float* B_dev, float* C_dev,
                     const float* bias_dev, int32_t relu, float dropout_p, uint64_t seed, uint64_t offset,
                     int32_t k, void* stream);
/* dst[i] = dropout(src[i]) for i < count with the mask defined above (dst may equal src): the backward of the
 * fused epilogue, and the forward where no fused pass exists. */
int gcn_dropout_f32(float* dst_dev, const float* src_dev, int64_t count, float dropout_p, uint64_t seed,
                    uint64_t offset, void* stream);


/* bf16 feature operands (torch.bfloat16; raw 16-bit words on the device), fp32 accumulation everywhere.  B is bf16
 * [n x k] row-major; C is [m x k] row-major of c_dtype (GCN_DTYPE_F32 or GCN_DTYPE_BF16; anything else:
 * GCN_ERR_INVALID_ARG); the epilogue and its dropout mask are those of gcn_spmm_csr_f32_epilogue, applied in fp32, and a
 * bf16 C is rounded once (round to nearest even).  Values and bias stay fp32.
 *   Hot path: k % 8 == 0, k >= 64, on a plan whose k-wide call would run a group kernel (column slicing, no panels): B is
 *   re-laid as a bf16 table in the group kernels' slice layout — value-free pass: bf16(u_col[c] * B[c, :]), rounded once
 *   (relative error <= 2^-9 per entry); weighted pass: the bits of B — and walked by spmm_group_bf16[_weighted]_kernel (the
 *   group walk of the fp32 kernels on rows of bf16), one 128-column tile per pass, into the same fp32 partial rows the
 *   fp32 path reduces.  The slice set is the one an fp32 call with the same row bytes (k / 2 columns) takes.
 *   Fallback, every other plan and width: B widened to fp32 in a plan buffer, the fp32 entry, C narrowed.  Correct, not
 *   fast: three passes and fp32 traffic.
 * A plan is shared with the fp32 calls (its re-laid copy of B serves both); like the fp32 calls, the calls of one plan
 * are issued on one stream at a time. */
#define GCN_DTYPE_F32  0
#define GCN_DTYPE_BF16 1
int gcn_spmm_csr_bf16_epilogue(gcn_spmm_plan_t* plan, const int32_t* rowptr_dev, const int32_t* col_dev, const float* val_dev,
                               const void* B_dev, void* C_dev, int32_t c_dtype, const float* bias_dev, int32_t relu,
                               float dropout_p, uint64_t seed, uint64_t offset, int32_t k, void* stream);
int gcn_spmm_csr_bf16(gcn_spmm_plan_t* plan, const int32_t* rowptr_dev, const int32_t* col_dev, const float* val_dev,
                      const void* B_dev, void* C_dev, int32_t c_dtype, int32_t k, void* stream);
/* gcn_dropout_f32 on bf16 data: the mask of element i as there, the kept value scaled in fp32 and rounded once */
int gcn_dropout_bf16(void* dst_dev, const void* src_dev, int64_t count, float dropout_p, uint64_t seed, uint64_t offset,
                     void* stream);
/* Feature-column tile per kernel pass: 0 = automatic, else 64, 128 or 256 columns.  A k-wide
 * SpMM runs as ceil(k/tile) back-to-back passes, each gathering only its column slice of B
 * (smaller per-pass working set -> more of it stays in L2 / Infinity Cache). */
int gcn_spmm_plan_set_tile_cols(gcn_spmm_plan_t* plan, int32_t cols);
/* Grid size of the main kernel in 256-thread blocks per CU, 1..64 (default 32).  At most 8 blocks
 * (4 for the four-per-gather kernel) are resident on a CU; the default oversubscribes on purpose so
 * that the hardware dispatcher hands out the remaining blocks as earlier ones finish (load balance:
 * 3.96 -> 3.68 ms on the Reddit-shaped graph).  A value below the resident count leaves wave slots
 * and registers free so that a kernel on another stream — the RCCL all-gather of the multi-GPU
 * path — can run beside the SpMM instead of behind it. */
int gcn_spmm_plan_set_blocks_per_cu(gcn_spmm_plan_t* plan, int32_t blocks);
/* Non-zeros per gather instruction of the 64-column-tile kernel: 0 = automatic — 4 (16 lanes x 16 bytes
 * per feature row, spmm_quad.hip) when k % 4 == 0 (odd widths are rounded up internally), operands are
 * 16-byte aligned, n < 2^24, n*k*4 < 4 GiB AND rows are long (>= 48 non-zeros per row, or per virtual
 * row when sliced: every finished row costs that layout a cross-lane reduction), else 1; 1 = always the
 * one-row-per-instruction kernel (52 VGPRs: leaves more room for a concurrent kernel); 4 = the
 * four-per-gather kernel wherever its layout applies, whatever the row length.  Any other value:
 * GCN_ERR_INVALID_ARG. */
int gcn_spmm_plan_set_gather_width(gcn_spmm_plan_t* plan, int32_t nz_per_gather);
/* number of main-kernel launches (column passes) one k-wide SpMM issues with the current tile */
int32_t gcn_spmm_plan_num_passes(const gcn_spmm_plan_t* plan, int32_t k);
/* name (as rocprofv3 --kernel-trace prints it, without the argument list) of the main kernel a
 * k-wide SpMM on this plan launches with the current settings and 16-byte aligned operands;
 * epilogue != 0: the bias/ReLU variant.  For benchmarks that report which kernel they timed. */
int gcn_spmm_plan_main_kernel(const gcn_spmm_plan_t* plan, int32_t k, int32_t epilogue, char* buf, int32_t buflen);
/* ... of a bf16 call (gcn_spmm_csr_bf16_epilogue): the bf16 group kernel on the hot path, else the fp32 kernel the
 * fallback runs */
int gcn_spmm_plan_main_kernel_bf16(const gcn_spmm_plan_t* plan, int32_t k, int32_t epilogue, char* buf, int32_t buflen);

/* XCD-aware column slicing (optional, off by default).  Builds, on the device, a slice-major copy
 * of the matrix (`slices` equal column ranges; virtual row s*m+r = the part of row r in slice s)
 * that later gcn_spmm_csr_f32* calls on this plan use instead of the caller's col/val: every XCD
 * then gathers from only ~slices/8 column slices of B, sized to stay in its 4 MiB L2, and a
 * reduction over slices (in slice order, deterministic) produces C.  Needs column-sorted rows
 * (GCN_ERR_INVALID_ARG otherwise); slices = 0/1 turns it off; slices = -1 picks the count from
 * (m, n, nnz) — off for low-degree graphs and tables that fit an L2 anyway, 2..8 otherwise — and silently stays off for
 * unsorted rows.  The matrix passed here must be the
 * one the plan was created for.  Costs one extra copy of col/val plus slices*m*k floats.
 * Values that factor as u_row[r]*u_col[c] — found here on the device, every entry checked to 4 ulp: the symmetric GCN
 * normalisation D^-1/2 (A+I) D^-1/2 (square matrices), values that depend on the row only (an unweighted adjacency,
 * the row-normalised D^-1 (A+I)) or on the column only (its transpose) — let the sliced pass run WITHOUT its value
 * stream (B scaled by u_col in the copy it gathers from, rows scaled by u_row in the reduction; results within the
 * 1e-5 contract).  gcn_spmm_plan_set_value_factors hands factors over for matrices that cannot see them (row blocks). */
int gcn_spmm_plan_enable_slicing(gcn_spmm_plan_t* plan, const int32_t* rowptr_dev,
                                 const int32_t* col_dev, const float* val_dev,
                                 int32_t slices, void* stream);
int32_t gcn_spmm_plan_num_slices(const gcn_spmm_plan_t* plan);
/* Slices of the slice set a k-wide call runs on when it is NOT the plan's own (0: it is).  Value-free plans whose slice
 * count was automatic cut the matrix again at their first call with k <= 32: a table row is 128 bytes there, half as
 * many slices fill an L2, and the partial rows — whose cost goes with the slice count — halve (Reddit-shaped: 8
 * instead of 15). */
int32_t gcn_spmm_plan_narrow_slices(const gcn_spmm_plan_t* plan, int32_t k);
/* Build NOW whatever a k-wide call of this plan would build at its first use (the narrow slice set above, the map of a
 * sliced gcn_sddmm_csr_f32: device
 * allocations and a stream synchronisation), e.g. before a stream capture whose first k-wide call must only enqueue
 * kernels.  The matrix arrays must be the ones the plan was created for.  Idempotent; GCN_OK also when nothing is to build. */
int gcn_spmm_plan_prepare_width(gcn_spmm_plan_t* plan, const int32_t* rowptr_dev, const int32_t* col_dev,
                                const float* val_dev, int32_t k, void* stream);

/* Rank-1 values.  When every stored value is u_row[r] * u_col[c] — the GCN normalisation
 * D^-1/2 (A+I) D^-1/2 has u = D^-1/2 — the sliced main pass runs WITHOUT its value stream (5 % of the
 * bytes it moves, and they are its time): B is gathered from a copy whose rows were scaled by u_col and
 * the finished rows are scaled by u_row in the slice reduction; results stay within the 1e-5 contract
 * (each term carries one more rounding).  gcn_spmm_plan_enable_slicing detects this by itself for SQUARE
 * matrices with a stored diagonal (u = sqrt(diag)); for anything else — e.g. a row block of such a
 * matrix with renumbered columns — hand the factors over here (device arrays [m] and [n], copied).
 * Every entry is checked (4 ulp): GCN_ERR_NOT_FACTORED if one does not factor (the plan then keeps working on
 * its value stream; every other status is a real failure).  (NULL, NULL) forgets the factors.  The matrix arrays must be the ones the plan was created for. */
int gcn_spmm_plan_set_value_factors(gcn_spmm_plan_t* plan, const int32_t* rowptr_dev, const int32_t* col_dev,
                                    const float* val_dev, const float* u_row_dev, const float* u_col_dev,
                                    void* stream);
int32_t gcn_spmm_plan_has_value_factors(const gcn_spmm_plan_t* plan);   /* 1 / 0 */

/* Mutable values (learned edge weights): the pattern stays, the values change.  Call before any stream capture (it
 * allocates and synchronises).  Drops what exists only for fixed values — value factors, the value-free streams and
 * panels — and builds the sliced copy again, once, as a weighted plan (an automatic slice count is re-chosen for one),
 * keeping the CSR start of every virtual row.  Afterwards gcn_spmm_plan_set_value_factors and enabling panels return
 * GCN_ERR_INVALID_ARG.  The matrix arrays must be the ones the plan was created for. */
int gcn_spmm_plan_set_values_mutable(gcn_spmm_plan_t* plan, const int32_t* rowptr_dev, const int32_t* col_dev,
                                     const float* val_dev, void* stream);
int32_t gcn_spmm_plan_values_mutable(const gcn_spmm_plan_t* plan);        /* 1 / 0 */
/* New values val_dev [nnz] (CSR order) into every value-bearing layout of a mutable plan: one O(nnz) kernel, no
 * allocation, no host synchronisation (legal inside a stream capture).  Later SpMM calls must pass these same values as
 * their val_dev (the unsliced paths read them there).  GCN_ERR_INVALID_ARG on a plan not made mutable. */
int gcn_spmm_plan_update_values(gcn_spmm_plan_t* plan, const float* val_dev, void* stream);

/* SDDMM on the plan's pattern: out_val[e] = sum_j A[row(e), j] * B[col(e), j] for every stored entry e, in CSR order.
 * A is m x k, B is n x k, both row-major fp32 (device); fp32 accumulation.  Empty rows write nothing; duplicate (r, c)
 * entries each get their own output.  k = 0 writes zeros.  Deterministic: the same (A, B, k) gives the same bits on
 * every plan of the matrix and every call.  Works on any plan; from k = 33 a sliced plan walks its slice-major copy
 * (the SpMM's L2 locality).  On a plan with fixed values its first such call ALLOCATES the map of the virtual rows
 * (4*S*m bytes) and synchronises, so it must not be the first inside a stream capture: call it once before, or
 * gcn_spmm_plan_prepare_width with that k.  Mutable plans have the map already. */
int gcn_sddmm_csr_f32(gcn_spmm_plan_t* plan, const int32_t* rowptr_dev, const int32_t* col_dev, const float* A,
                      const float* B, float* out_val, int32_t k, void* stream);
/* name of the kernel a k-wide gcn_sddmm_csr_f32 on this plan launches (16-byte-aligned operands) */
int gcn_spmm_plan_sddmm_kernel(const gcn_spmm_plan_t* plan, int32_t k, char* buf, int32_t buflen);

/* Edge softmax family: softmax over the stored entries of each row of a CSR pattern, its backward, both fused with GAT
 * scores, and CSR row sums of a per-entry array.  Plan-free: they work on the caller's CSR (rowptr_dev [m + 1], col_dev
 * [nnz] where named), all per-entry arrays are fp32 [nnz] in CSR entry order.  They only enqueue (a 4-byte memset node and
 * kernels): no allocation, no host synchronisation, no host read of device data — legal inside a stream capture.  No
 * atomics: every output has one writer, results are bit-identical from call to call.  Any nnz an int32 holds is fine:
 * entries are addressed as offsets from their row's start, never past its end.  Row lengths may be anything — short
 * rows share a wave, a row of more than 8192 entries is spread over the chip, empty rows cost a row-pointer read.
 * ws: device scratch of at least GCN_EDGE_WS_BYTES(nnz) bytes, 16-byte aligned, owned by the call until it has run
 * (calls on different streams need different ones).  Null pointers, negative sizes or a short workspace:
 * GCN_ERR_INVALID_ARG; m == 0 or nnz == 0: GCN_OK, nothing is launched and nothing written. */
#define GCN_EDGE_WS_BYTES(nnz) (16 + 16 * (((size_t)(nnz) + 8191) / 8192))
/* p[e] = exp(scores[e] - max_row) / sum_row exp(scores[e'] - max_row).  p may alias scores.  Empty rows write nothing.
 * DELIBERATELY UNLIKE torch.softmax, so that masks work: a row whose entries are all -inf gets zeros, not NaN (an entry of
 * -inf beside a finite one gets 0, as there).  A NaN makes every entry of its own row NaN and touches no other row. */
int gcn_edge_softmax_csr_f32(const int32_t* rowptr_dev, int32_t m, int32_t nnz, const float* scores, float* p, void* ws,
                             size_t ws_bytes, void* stream);
/* ds[e] = p[e] * (g[e] - sum_row p[e'] g[e']) from the saved p and the incoming gradient g.  ds may alias g. */
int gcn_edge_softmax_backward_csr_f32(const int32_t* rowptr_dev, int32_t m, int32_t nnz, const float* p, const float* g,
                                      float* ds, void* ws, size_t ws_bytes, void* stream);
/* The same softmax of s[e] = leaky_relu(a_dst[row(e)] + a_src[col(e)], negative_slope), computed on the fly: the score
 * array is never written.  a_dst [m], a_src [n] (gathered by column). */
int gcn_gat_edge_softmax_csr_f32(const int32_t* rowptr_dev, const int32_t* col_dev, int32_t m, int32_t nnz, const float* a_dst,
                                 const float* a_src, float negative_slope, float* p, void* ws, size_t ws_bytes, void* stream);
/* Its backward: recomputes the scores, writes ds[e] = p (g - sum_row p g) * (s_pre > 0 ? 1 : negative_slope) — the
 * derivative at 0 is the slope, as in torch — and grad_a_dst[r] = sum_row ds (0 for an empty row).  ds may alias g.
 * grad_a_src[c] = sum over col(e) = c of ds[e] is gcn_segment_sum_csr_f32 over the transpose's row pointer with the
 * permutation that takes CSR order to the transpose's order. */
int gcn_gat_edge_softmax_backward_csr_f32(const int32_t* rowptr_dev, const int32_t* col_dev, int32_t m, int32_t nnz,
                                          const float* a_dst, const float* a_src, float negative_slope, const float* p,
                                          const float* g, float* ds, float* grad_a_dst, void* ws, size_t ws_bytes,
                                          void* stream);
/* out[r] = sum of x[e] over the entries e of row r (0 for an empty row); with perm_dev (int32 [nnz], may be NULL) the
 * entry read is x[perm_dev[e]]. */
int gcn_segment_sum_csr_f32(const int32_t* rowptr_dev, int32_t m, int32_t nnz, const float* x, const int32_t* perm_dev,
                            float* out, void* ws, size_t ws_bytes, void* stream);

/* Neighbourhood max / min ("pooling" aggregation: GraphSAGE, PyG aggr="max", DGL copy_u_max) over the stored entries of
 * each row of a CSR pattern, and its backward.  Plan-free like the edge softmax family: the caller's CSR, only memset nodes
 * and kernels (no allocation, no host synchronisation, no host read of device data: legal inside a stream capture), no
 * atomics, the same bits at every call.  The stored VALUES of the matrix are not used; every stored entry is a candidate
 * of its own, duplicated (row, column) pairs included.  Row lengths may be anything: a row of more than 4096 entries is
 * spread over the chip, empty rows cost a row-pointer read and their stores.
 *   out[r, j] = max (min) over the entries e of row r of x[col[e], j],   arg[r, j] = that e (its index into col_dev)
 * x [n x k], out [m x k] row-major, both fp32 (GCN_DTYPE_F32) or both bf16 (GCN_DTYPE_BF16); arg [m x k] int32.
 * An empty row gets out = 0, arg = -1.  Equal values (-0.0 equals +0.0): the lowest entry index wins and its bits are
 * stored.  A NaN beats every number and the first NaN entry of the row is the arg.  +-inf are ordinary values.  The result
 * is exact (a selection: nothing is rounded).  Any k >= 1; 16-byte loads and stores are used when x, out and arg are
 * 16-byte aligned and k is a multiple of 4 (bf16: 8), element accesses otherwise.
 * ws: device scratch of at least GCN_AGGREGATE_WS_BYTES(nnz, k) bytes, 16-byte aligned, owned by the call until it has run
 * (calls on different streams need different ones).  Null pointers, negative sizes, k < 1, an unknown op or dtype or a
 * short workspace: GCN_ERR_INVALID_ARG.  m == 0: GCN_OK, nothing written; nnz == 0: out is zeroed and arg set to -1. */
#define GCN_AGGREGATE_WS_BYTES(nnz, k) (16 + 16 * (size_t)(k) * (((size_t)(nnz) + 4095) / 4096))
#define GCN_REDUCE_MAX 0
#define GCN_REDUCE_MIN 1
int gcn_aggregate_csr(const int32_t* rowptr_dev, const int32_t* col_dev, int32_t m, int32_t n, int32_t nnz, const void* x,
                      int32_t dtype, int32_t k, int32_t op, void* out, int32_t* arg, void* ws, size_t ws_bytes, void* stream);
/* Its backward, as a walk of the TRANSPOSED pattern (no atomics, one writer per element): trowptr_dev [n + 1], trow_dev
 * [nnz] (the row of each entry of the transpose, i.e. the forward's row) and tperm_dev [nnz] (the entry's index in the
 * forward's CSR order) describe the transpose of the m x n pattern, duplicates kept as separate entries.
 *   gx[c, j] = sum of g[trow[t], j] over the entries t of transposed row c with arg[trow[t], j] == tperm[t]
 * g [m x k] and gx [n x k] of `dtype`, arg as the forward wrote it.  Sums are fp32 in a fixed order (bf16: rounded once at
 * the store).  n == 0: nothing written; nnz == 0: gx is zeroed.  Same workspace rule (the forward's workspace will do). */
int gcn_aggregate_backward_csr(const int32_t* trowptr_dev, const int32_t* trow_dev, const int32_t* tperm_dev, int32_t n,
                               int32_t m, int32_t nnz, const void* g, int32_t dtype, const int32_t* arg, int32_t k, void* gx,
                               void* ws, size_t ws_bytes, void* stream);

/* Edge-feature message passing (edge_message.hip; DGL's u_op_e -> reduce: GINE, MPNN, CGConv): a feature VECTOR per stored
 * entry beside the gathered node row.  Plan-free like the aggregation family above: the caller's CSR, one memset node and
 * kernels (no allocation, no host synchronisation, no host read of device data: legal inside a stream capture), no
 * atomics, every output element has one writer and every sum a fixed order: the same bits at every call.  The stored
 * VALUES of the matrix are not used; duplicated (row, column) pairs are separate entries.  Any row length (rows of more
 * than 4096 entries are spread over the chip).  All operands fp32, row-major: x [n x k], w [nnz x k] in the CSR's entry
 * order (row e belongs to entry e of col_dev), out [m x k].  nnz * k may pass 2^31: offsets into w and ge are 64-bit.
 *   The message.  t = x[col[e], j] + w[e, j] (GCN_EDGE_OP_ADD) or x[col[e], j] * w[e, j] (GCN_EDGE_OP_MUL): one fp32
 *   operation, rounded once, never fused into the accumulation.  Then act: GCN_EDGE_ACT_NONE, or GCN_EDGE_ACT_RELU:
 *   msg = t < 0 ? +0 : t, so a NaN and -0.0 pass.  The derivative D = t <= 0 ? 0 : 1 under relu (a NaN t passes the
 *   gradient; D selects: a zero D gives a zero, whatever g holds), 1 without.
 *   out[r, j] = the reduce over the entries e of row r of msg(e, j).  GCN_REDUCE_SUM: slot s of 64 / LPS adds the entries
 *   s, s + SLOTS, ... in ascending order as a compensated (Kahan) chain, the slots are merged by an xor butterfly, chunk
 *   partials of a long row in chunk order (LPS = 16, 32 or 64 lanes for k / VEC <= 16, <= 32, more).  GCN_REDUCE_MAX / GCN_REDUCE_MIN: the selection rule
 *   of gcn_aggregate_csr applied to the message (the first entry among equals, -0.0 equals +0.0, a NaN beats every number
 *   and the first NaN wins; the message's bits are stored) and arg[r, j] = that entry's index.  An empty row gets 0 (arg
 *   -1).  arg [m x k] int32 is required for max / min and ignored (may be NULL) for the sum.
 * 16-byte accesses (VEC = 4) when x, w and out (g, gx, ge) are 16-byte aligned and k % 4 == 0, element accesses otherwise.
 * ws: device scratch of at least GCN_EDGE_AGGREGATE_WS_BYTES(nnz, k) bytes, 16-byte aligned, owned by the call until it
 * has run; the three calls on a pattern and its transpose may share it.  GCN_ERR_INVALID_ARG, before any pointer is read:
 * null pointers, negative sizes, k < 1, k > 16 * 65535 (column tiles ride in the grid), an unknown op, act or reduce, a
 * short workspace.  m == 0: GCN_OK, nothing launched; nnz == 0: out is zeroed and arg set to -1. */
#define GCN_EDGE_AGGREGATE_WS_BYTES(nnz, k) (16 + 16 * (size_t)(k) * (((size_t)(nnz) + 4095) / 4096))
#define GCN_EDGE_OP_ADD 0
#define GCN_EDGE_OP_MUL 1
#define GCN_EDGE_ACT_NONE 0
#define GCN_EDGE_ACT_RELU 1
#define GCN_REDUCE_SUM 2
int gcn_edge_aggregate_csr_f32(const int32_t* rowptr_dev, const int32_t* col_dev, int32_t m, int32_t n, int32_t nnz,
                               const float* x, const float* w, int32_t k, int32_t op, int32_t act, int32_t reduce, float* out,
                               int32_t* arg, void* ws, size_t ws_bytes, void* stream);
/* The gradient of the SUM in x, as the forward's walk on the TRANSPOSED pattern (trowptr_dev [n + 1], trow_dev, tperm_dev as
 * in gcn_aggregate_backward_csr): for the entry t of transposed row c, r = trow[t] and e = tperm[t],
 *   gx[c, j] = sum of g[r, j] * D * (w[e, j] if mul),   D from t = x[c, j] op w[e, j], recomputed
 * in the forward's fixed order; nothing of size nnz x k is kept by the forward.  g [m x k], gx [n x k]; an empty row gets
 * zeros.  n == 0: nothing written; nnz == 0: gx is zeroed. */
int gcn_edge_aggregate_backward_x_csr_f32(const int32_t* trowptr_dev, const int32_t* trow_dev, const int32_t* tperm_dev, int32_t n,
                                          int32_t m, int32_t nnz, const float* g, const float* x, const float* w, int32_t k,
                                          int32_t op, int32_t act, float* gx, void* ws, size_t ws_bytes, void* stream);
/* The gradient of the SUM in w, one writer per element of ge [nnz x k]:
 *   ge[e, j] = g[row(e), j] * D * (x[col[e], j] if mul)
 * x is gathered only where D or mul needs it and w read only where D needs it.  m == 0 or nnz == 0: nothing written.
 * (The backward of max / min needs neither kernel: with arg it is element-wise work on [m x k] arrays and one
 * gcn_aggregate_backward_csr.) */
int gcn_edge_aggregate_backward_e_csr_f32(const int32_t* rowptr_dev, const int32_t* col_dev, int32_t m, int32_t n, int32_t nnz,
                                          const float* g, const float* x, const float* w, int32_t k, int32_t op, int32_t act,
                                          float* ge, void* ws, size_t ws_bytes, void* stream);

/* Head-batched attention primitives (multihead.hip): the edge softmax family, the weighted SpMM and the SDDMM for H heads
 * in one pass over the adjacency.  Plan-free like the two families above: the caller's CSR, one 4-byte memset node and
 * kernels (legal inside a stream capture), no host read of device data, no atomics, the same bits at every call; any row
 * length, rows of more than 8192 (softmax family) or 4096 (SpMM, SDDMM) entries are spread over the chip in chunks whose
 * partials are merged in chunk order.  All operands fp32.
 *   Layouts.  H = heads >= 1, F columns per head, k = H * F.  Node arrays are [rows, k] row-major and head h owns columns
 *   hF .. hF + F - 1; per-entry arrays are [nnz, H] in CSR entry order with an entry's heads contiguous; per-node scalars
 *   are [rows, H].  nnz * H must stay below 2^31.
 *   Power-of-two H <= 16 is the fast case of the softmax family and the segment sum (a lane owns one head and the row's
 *   [len, H] block is read as one contiguous stream); any other H walks the row once per head with stride H.  The SpMM and
 *   the SDDMM use 16-byte accesses when every operand is 16-byte aligned and F % 4 == 0, element accesses otherwise.
 * ws: device scratch of at least the bytes gcn_heads_ws_bytes reports for (m, nnz, heads, k) — enough for every entry
 * point below on that pattern and its transpose — 16-byte aligned, owned by the call until it has run.
 * GCN_ERR_INVALID_ARG: null pointers, negative sizes, heads < 1, k < heads or k % heads != 0 where k is taken,
 * nnz * heads >= 2^31 (checked before any pointer), k > 16 * 65535, a short workspace.  rows == 0 or nnz == 0: GCN_OK,
 * nothing is launched and nothing written (as in the edge softmax family: the caller zeroes per-row outputs). */
int gcn_heads_ws_bytes(int32_t m, int32_t nnz, int32_t heads, int32_t k, size_t* bytes);
/* p[e, h] = softmax over the entries of row(e), separately per head, of scores[e, h]; the conventions of
 * gcn_edge_softmax_csr_f32 per (row, head): all -inf gives zeros, a NaN poisons its own (row, head) only.  p may alias scores. */
int gcn_edge_softmax_heads_csr_f32(const int32_t* rowptr_dev, int32_t m, int32_t nnz, int32_t heads, const float* scores,
                                   float* p, void* ws, size_t ws_bytes, void* stream);
/* ds[e, h] = p[e, h] * (g[e, h] - sum over row(e) of p[., h] g[., h]) (row sums in fp64).  ds may alias g. */
int gcn_edge_softmax_heads_backward_csr_f32(const int32_t* rowptr_dev, int32_t m, int32_t nnz, int32_t heads, const float* p,
                                            const float* g, float* ds, void* ws, size_t ws_bytes, void* stream);
/* the same softmax of s[e, h] = leaky_relu(a_dst[row(e), h] + a_src[col[e], h], negative_slope), never stored.
 * a_dst [m, H], a_src [n, H]. */
int gcn_gat_edge_softmax_heads_csr_f32(const int32_t* rowptr_dev, const int32_t* col_dev, int32_t m, int32_t nnz, int32_t heads,
                                       const float* a_dst, const float* a_src, float negative_slope, float* p, void* ws,
                                       size_t ws_bytes, void* stream);
/* its backward: ds [nnz, H] (times the leaky_relu derivative, the slope at 0) and grad_a_dst [m, H] = row sums of ds.
 * grad_a_src [n, H] is gcn_segment_sum_heads_csr_f32 of ds over the transposed pattern with its permutation. */
int gcn_gat_edge_softmax_heads_backward_csr_f32(const int32_t* rowptr_dev, const int32_t* col_dev, int32_t m, int32_t nnz,
                                                int32_t heads, const float* a_dst, const float* a_src, float negative_slope,
                                                const float* p, const float* g, float* ds, float* grad_a_dst, void* ws,
                                                size_t ws_bytes, void* stream);
/* out[r, h] = sum over the entries e of row r of x[perm ? perm[e] : e, h], carried in fp64 (0 for an empty row). */
int gcn_segment_sum_heads_csr_f32(const int32_t* rowptr_dev, int32_t rows, int32_t nnz, int32_t heads, const float* x,
                                  const int32_t* perm_dev, float* out, void* ws, size_t ws_bytes, void* stream);
/* out[r, hF + j] = sum over the entries e of row r of vals[perm ? perm[e] : e, h] * x[idx[e], hF + j].  Forward: idx = col,
 * perm = NULL.  Gradient with respect to x: the transposed pattern (rowptr = trowptr, idx = the source row of each entry,
 * perm = the entry's index in the forward's order).  out [rows, k]; x has a row for every value of idx. */
int gcn_spmm_heads_csr_f32(const int32_t* rowptr_dev, const int32_t* idx_dev, const int32_t* perm_dev, int32_t rows, int32_t nnz,
                           int32_t heads, int32_t k, const float* vals, const float* x, float* out, void* ws, size_t ws_bytes,
                           void* stream);
/* out[e, h] = sum over j < F of a[row(e), hF + j] * b[col[e], hF + j]: per-head dot-product scores, and the gradient of
 * the SpMM above with respect to vals (a = grad_out, b = x).  The summation order of an (entry, head) depends on F and on
 * the aligned / element form only. */
int gcn_sddmm_heads_csr_f32(const int32_t* rowptr_dev, const int32_t* col_dev, int32_t m, int32_t nnz, int32_t heads, int32_t k,
                            const float* a, const float* b, float* out, void* ws, size_t ws_bytes, void* stream);

/* GATv2 attention scores (multihead.hip), in the layouts and under the argument rules of the head-batched family above:
 *   out[e, h] = sum over j < F of att[h, j] * leaky_relu(h_dst[row(e), hF + j] + h_src[col[e], hF + j], negative_slope)
 * h_dst [m, k], h_src with a row for every value of col, att [H, F] row-major (its flat index is the node column), out
 * [nnz, H].  Per element t = h_dst + h_src rounded to fp32, then t > 0 ? t : negative_slope * t, then one fma with att; at
 * t == 0 the value is negative_slope * 0 and the derivative below is the slope.  The summation order of an (entry, head)
 * is the one of gcn_sddmm_heads_csr_f32: a function of F and of the aligned / element form only (the aligned form: h_dst,
 * h_src and att 16-byte aligned and F % 4 == 0).  A NaN in t makes that (entry, head) NaN and no other.
 * ws: at least the bytes gcn_gatv2_ws_bytes reports — 16 + 2 * 8 * k * ceil(nnz / 4096), the flag and the long rows' chunk
 * partials of the backward's two sums — 16-byte aligned; the three calls on a pattern and its transpose share it. */
int gcn_gatv2_ws_bytes(int32_t m, int32_t nnz, int32_t heads, int32_t k, size_t* bytes);
int gcn_gatv2_scores_csr_f32(const int32_t* rowptr_dev, const int32_t* col_dev, int32_t m, int32_t nnz, int32_t heads, int32_t k,
                             const float* h_dst, const float* h_src, const float* att, float negative_slope, float* out,
                             void* ws, size_t ws_bytes, void* stream);
/* The backward on one side, a row walk like gcn_spmm_heads_csr_f32 over (rowptr, idx, perm).  With
 * t = own[r, j] + other[idx[e], j] and D = t > 0 ? 1 : negative_slope, over the entries e of row r and h the head of j:
 *   grad_own[r, j] = att[j] * sum of g[perm ? perm[e] : e, h] * D                  (multiplied once, after the sum)
 *   act_sums[r, j] =          sum of g[perm ? perm[e] : e, h] * (t * D)            (where act_sums is not NULL)
 * grad_h_dst and act_sums: own = h_dst, other = h_src, idx = col, perm = NULL; grad_att[h, j] is the sum over r of
 * act_sums[r, hF + j].  grad_h_src: the transposed pattern (rowptr = trowptr, idx = the source row of each entry, perm = the
 * entry's index in the forward's order), own = h_src, other = h_dst, act_sums = NULL.  g [nnz, H]; own, grad_own and
 * act_sums [rows, k]; an empty row gets zeros.  Fixed order: a sum is carried in SLOTS interleaved fma chains merged by an xor
 * butterfly, rows of more than 4096 entries as chunk partials merged in chunk order.  A NaN in t or g stays in its (row, j). */
int gcn_gatv2_scores_backward_csr_f32(const int32_t* rowptr_dev, const int32_t* idx_dev, const int32_t* perm_dev, int32_t rows,
                                      int32_t nnz, int32_t heads, int32_t k, const float* own, const float* other,
                                      const float* att, float negative_slope, const float* g, float* grad_own, float* act_sums,
                                      void* ws, size_t ws_bytes, void* stream);

/* Uniform neighbour sampling without replacement from the rows of a CSR matrix (GraphSAGE's mini-batch sampler).  Plan-free
 * like the aggregation family: the caller's CSR, one memset node and kernels, no allocation, no host read of device data, no
 * global atomics; every output element has one writer, so a call gives the same bits every time.  The stored values are
 * not used.  The contract, exact and meant to be re-implemented (tests/sampling_ref.py is the numpy twin):
 *   Output row i belongs to the vertex v = seeds_dev[i] (seeds in any order, repeats allowed).  Its entries are
 *   e in [rowptr[v], rowptr[v + 1]); d is their number, f = fanout.
 *   Selection.  fanout < 0 or d <= f: all d entries.  Otherwise key(e) = word (e & 3) of Philox4x32-10 with counter
 *   (lo32(e >> 2), hi32(e >> 2), lo32(offset), hi32(offset)) and key (lo32(seed), hi32(seed)) — the word and counter
 *   convention of the dropout mask above with the entry index e (the index into col_dev) in the place of the element
 *   index — and the f entries with the smallest (key(e), e) in lexicographic order are selected: among equal keys the lower
 *   entry index wins.
 *   Order.  The selected entries of a row are written in ascending e (the CSR's own order: a column-sorted row stays
 *   sorted): out_col[out_rowptr[i] + t] = col[e_t] and out_eid[out_rowptr[i] + t] = e_t for t = 0 .. min(d, f) - 1.
 * Consequences: the keys are i.i.d. words, so the f smallest are a uniform subset — the sample is uniform without
 * replacement; the neighbours drawn for a vertex depend on (seed, offset) only, not on the batch it is in or on its place
 * there — so two hops of one batch, and successive batches, must use different offsets.
 * out_rowptr_dev [n_seeds + 1] is an INPUT: out_rowptr[i + 1] - out_rowptr[i] = min(d_i, f) (d_i for fanout < 0), computed
 * by the caller, who needs the total to size out_col / out_eid anyway.  A seed outside [0, m), or a row whose out_rowptr
 * length is not that number, writes nothing.  Every row length from 0 to nnz works and the host never reads one: a row of
 * at most GCN_SAMPLE_LONG_ROW entries is taken by one wave, a longer one by a 256-thread workgroup.
 * ws: GCN_SAMPLE_WS_BYTES of device scratch, owned by the call until it has run.  fanout == 0, negative sizes, a null
 * pointer or a short workspace: GCN_ERR_INVALID_ARG; n_seeds == 0, m == 0 or nnz == 0: GCN_OK, nothing written. */
#define GCN_SAMPLE_WS_BYTES 16
#define GCN_SAMPLE_LONG_ROW 2048
int gcn_sample_neighbors_csr(const int32_t* rowptr_dev, const int32_t* col_dev, int32_t m, int32_t nnz, const int32_t* seeds_dev,
                             int32_t n_seeds, int32_t fanout, uint64_t seed, uint64_t offset, const int32_t* out_rowptr_dev,
                             int32_t* out_col_dev, int32_t* out_eid_dev, void* ws, size_t ws_bytes, void* stream);

/* The vertex-induced subgraph of a CSR matrix (the mini-batch of Cluster-GCN and of GraphSAINT's samplers: the square
 * adjacency over a vertex set that a GCN layer needs), as two calls with the caller's prefix sum between them.  Plan-free
 * like the sampling call and under the same rules: the caller's CSR, one memset node and kernels, no allocation, no host
 * read of device data, no global atomics; every output element has one writer, so a call gives the same bits every time.
 * The stored values are not used.  Every access is a 4-byte one: no pointer needs more than 4-byte alignment.  The
 * contract, exact and meant to be re-implemented (tests/subgraph_ref.py is the numpy twin):
 *   nodes_dev [n_nodes]: vertex ids in any order (row ids in [0, m)).  vmap_dev [n], n the number of columns: vmap[c] is
 *   the position of column c in the vertex set, or -1 (any negative number) when c is not in it.  The caller fills it
 *   before the calls and clears it afterwards; the calls only read it.  Every col[e] must lie in [0, n), as for the SpMM.
 *   Output row i belongs to the vertex v = nodes_dev[i].  Its entries are the e in [rowptr[v], rowptr[v + 1]) with
 *   vmap[col[e]] >= 0, e_0 < e_1 < ... (the parent's entry order: a column-sorted row stays sorted by parent column).
 *   Count:  out_len_dev[i] = the number of those entries.
 *   Fill:   out_col_dev[out_rowptr[i] + t] = vmap[col[e_t]] and out_eid_dev[out_rowptr[i] + t] = e_t.
 * out_rowptr_dev [n_nodes + 1] is an INPUT of the fill: the exclusive prefix sum of out_len, computed by the caller, who
 * needs its last element to size out_col / out_eid anyway — which is why there are two calls.
 * These write nothing for their row: a node outside [0, m), a row pointer outside [0, nnz], and in the fill a row whose
 * out_rowptr length differs from its count (or whose out_rowptr[i] is negative).  Every row length from 0 to nnz works and
 * the host never reads one: a row of at most GCN_SAMPLE_LONG_ROW entries is taken by one wave, a longer one by a
 * 256-thread workgroup.
 * ws: GCN_SUBGRAPH_WS_BYTES of device scratch, owned by the call until it has run.  Negative sizes, a null pointer or a
 * short workspace: GCN_ERR_INVALID_ARG; n_nodes == 0, m == 0 or nnz == 0: GCN_OK, nothing written (out_len keeps what it
 * held: a caller who may pass nnz == 0 zeroes it first).  A caller whose counts sum to 0 has nothing to fill and skips the
 * second call (its empty outputs may have no address, and a null output is refused). */
#define GCN_SUBGRAPH_WS_BYTES 16
int gcn_induced_subgraph_count_csr(const int32_t* rowptr_dev, const int32_t* col_dev, int32_t m, int32_t nnz,
                                   const int32_t* nodes_dev, int32_t n_nodes, const int32_t* vmap_dev, int32_t* out_len_dev,
                                   void* ws, size_t ws_bytes, void* stream);
int gcn_induced_subgraph_fill_csr(const int32_t* rowptr_dev, const int32_t* col_dev, int32_t m, int32_t nnz,
                                  const int32_t* nodes_dev, int32_t n_nodes, const int32_t* vmap_dev,
                                  const int32_t* out_rowptr_dev, int32_t* out_col_dev, int32_t* out_eid_dev, void* ws,
                                  size_t ws_bytes, void* stream);

/* Uniform random walks on a square CSR pattern (GraphSAINT's random-walk sampler; DeepWalk's walks), a pure function of
 * (seed, offset, walk index, step).  One kernel, no workspace, no allocation, no host read of device data, no atomics;
 * every output element has one writer.  The stored values are not used; 4-byte accesses only.  The contract:
 *   out_walks_dev is int32 [length + 1][n_walks], STEP-major: element (t, i) at out_walks_dev[t * n_walks + i] (the index
 *   is computed in 64 bits).  Row 0 is the starts: out_walks[0][i] = starts_dev[i].
 *   Step t = 0 .. length - 1 of walk i, at the vertex v = out_walks[t][i], d = rowptr[v + 1] - rowptr[v]:
 *     d == 0 (a dead end), or a row pointer outside [0, nnz]: the walk stays, out_walks[t + 1][i] = v.  Otherwise let
 *     L4 = 4 * ceil(length / 4) and j = i * L4 + t as a 64-bit integer;
 *     key  = word (j & 3) of Philox4x32-10 with counter (lo32(j >> 2), hi32(j >> 2), lo32(offset), hi32(offset)) and key
 *            (lo32(seed), hi32(seed)) — the word and counter convention of the dropout mask and of the sampling call;
 *     pick = (key * d) >> 32, the high word of the 32 x 32-bit product, in [0, d);
 *     c    = col[rowptr[v] + pick];  out_walks[t + 1][i] = c, or v when c is outside [0, m) (the walk stays).
 *   L4 is a multiple of 4, so the four steps 4q .. 4q + 3 of a walk share the counter i * L4 / 4 + q: one Philox call
 *   serves four consecutive steps.
 * Uniformity: key is a uniform 32-bit word, so pick takes each value in [0, d) with probability floor or ceil of 2^32 / d
 * over 2^32: uniform up to a bias below d / 2^32 per entry (relative), e.g. 2^-19 for a row of 8192 entries.  A stored
 * entry that is repeated in a row is chosen in proportion to its multiplicity.
 * A walk depends on its own index i, its start, length (through L4), seed and offset only — not on n_walks or on the other
 * walks of the call; successive batches must use different offsets.
 * A start outside [0, m) fills that walk with -1, row 0 included.  Negative sizes or a null pointer: GCN_ERR_INVALID_ARG
 * (rowptr_dev may be null when m == 0, col_dev when nnz == 0); n_walks == 0: GCN_OK, nothing written; length == 0 writes
 * row 0. */
int gcn_random_walk_csr(const int32_t* rowptr_dev, const int32_t* col_dev, int32_t m, int32_t nnz, const int32_t* starts_dev,
                        int32_t n_walks, int32_t length, uint64_t seed, uint64_t offset, int32_t* out_walks_dev, void* stream);

/* Edge lookup on a CSR pattern whose rows hold ASCENDING columns (DGL's has_edges_between / edge_ids): the entry index of
 * each queried pair.  One kernel, one lane per query, no workspace, no allocation, no host read of device data, no atomics;
 * every output element has one writer; the call only enqueues.  The stored values are not used; 4-byte accesses only: no
 * pointer needs more than 4-byte alignment.  The contract (tests/linkpred_ref.py is the numpy twin):
 *   out_eid_dev[i] = the LOWEST entry index e in [rowptr[r], rowptr[r + 1]) with col[e] == q_cols_dev[i], r = q_rows_dev[i]
 *   (a row may repeat a column), or -1 when the pair is not stored, r is outside [0, m), or the row's pointers are outside
 *   [0, nnz] or out of order.  A q_cols_dev[i] that is negative or beyond the last column is simply not found.
 * The search is a lower bound over the row (about log2 of its length dependent probes).  On a row whose columns do NOT
 * ascend it still terminates and reads nothing outside the row's entries, but the answer is unspecified: an entry index of
 * that row holding the column, or -1 although the column is stored.  The caller sorts first (gcn_amd.csr_from_edges
 * with sort_columns=True, gcn_amd.coalesce_csr).
 * The launch shape depends on n_queries only; the host never reads a row length.
 * Negative sizes or a null pointer: GCN_ERR_INVALID_ARG (rowptr_dev may be null when m == 0, col_dev when nnz == 0);
 * n_queries == 0: GCN_OK, nothing written. */
int gcn_csr_find_entries(const int32_t* rowptr_dev, const int32_t* col_dev, int32_t m, int32_t nnz, const int32_t* q_rows_dev,
                         const int32_t* q_cols_dev, int32_t n_queries, int32_t* out_eid_dev, void* stream);

/* Negative sampling for link prediction: num_neg columns per queried row that the row does NOT store, by rejection, a pure
 * function of (seed, offset, slot).  Same pattern (ascending columns within rows, same behaviour on a row that does not
 * ascend: terminates in bounds, answer unspecified) and same rules as the lookup, whose row search it shares: one kernel,
 * one lane per slot, no workspace, no allocation, no host read of device data, no atomics, one writer per output element,
 * 4-byte accesses only.  The contract (tests/linkpred_ref.py is the numpy twin):
 *   out_cols_dev is int32 [n_queries * num_neg]; slot p = i * num_neg + s (a 64-bit integer) belongs to row r = q_rows_dev[i].
 *   Let T4 = 4 * ceil(max_tries / 4).  Try t = 0 .. max_tries - 1 of slot p uses j = p * T4 + t:
 *     key = word (j & 3) of Philox4x32-10 with counter (lo32(j >> 2), hi32(j >> 2), lo32(offset), hi32(offset)) and key
 *           (lo32(seed), hi32(seed)) — the word and counter convention of gcn_random_walk_csr;
 *     c   = (key * n) >> 32, the high word of the 32 x 32-bit product, in [0, n).
 *   out_cols_dev[p] = the first c, in ascending t, that is not stored in row r and, with exclude_self != 0, differs from r;
 *   -1 when all max_tries candidates are refused, or the row is unusable (r outside [0, m), row pointers outside [0, nnz] or
 *   out of order).
 *   T4 is a multiple of 4, so the tries 4q .. 4q + 3 of a slot share the counter p * T4 / 4 + q: one Philox call serves
 *   four consecutive tries, made when the first of the four is needed.
 * Uniformity: key is a uniform 32-bit word, so c takes each value in [0, n) with probability floor or ceil of 2^32 / n over
 * 2^32; over the columns that pass the two tests the accepted column is therefore uniform up to a relative bias below
 * n / 2^32, e.g. 2^-14 for n = 2^18.  A slot is -1 with probability (refused columns / n)^max_tries.
 * Independence: a slot depends on (seed, offset, p, max_tries — through T4 —, n, and the contents of its row) only, not on
 * n_queries or the other queries of the call; successive batches must use different offsets.  The slots of one query are
 * drawn independently of each other: two of them MAY hold the same column.
 * 1 <= max_tries <= 64, num_neg >= 1, n_queries * num_neg < 2^31, n >= 1 when n_queries > 0; anything else, negative sizes
 * or a null pointer: GCN_ERR_INVALID_ARG (rowptr_dev may be null when m == 0, col_dev when nnz == 0); n_queries == 0:
 * GCN_OK, nothing written.  The launch shape depends on n_queries * num_neg only. */
int gcn_negative_sample_csr(const int32_t* rowptr_dev, const int32_t* col_dev, int32_t m, int32_t n, int32_t nnz,
                            const int32_t* q_rows_dev, int32_t n_queries, int32_t num_neg, int32_t max_tries,
                            int32_t exclude_self, uint64_t seed, uint64_t offset, int32_t* out_cols_dev, void* stream);

/* Stable bucketing of the indices 0 .. count - 1 by an integer key: the primitive under the device CSR transpose and under
 * building a CSR from an edge list (gcn_amd/construct.py).  Two calls with the caller's prefix sum between them, as for the
 * induced subgraph, and plan-free under the same rules: the caller's arrays, memset / copy nodes and kernels, no allocation,
 * no host read of device data; the calls only enqueue on the given stream.  4-byte accesses only: no pointer needs more than
 * 4-byte alignment.  The contract, exact and meant to be re-implemented (tests/construct_ref.py is the numpy twin):
 *   keys_dev [count]: int32, every key in [0, nbuckets) — a precondition: a key outside the range is not counted and not
 *   placed (nothing is written out of bounds), and the result is then not a permutation.
 *   Count:  offsets_dev[0] = 0 and offsets_dev[b + 1] = the number of i with keys[i] == b, for b in [0, nbuckets).
 *   The caller then turns offsets_dev [nbuckets + 1] into its inclusive prefix sum IN PLACE (offsets[b] = the start of
 *   bucket b, offsets[nbuckets] = count).
 *   Fill:   perm_dev[offsets[b] .. offsets[b + 1]) = the i with keys[i] == b, IN ASCENDING i.
 * That is perm = argsort(keys, stable) and offsets = the prefix sum of bincount(keys, minlength = nbuckets), bit for bit
 * and the same at every call: the counts are integer atomic adds, which commute, and the fill scatters the indices to
 * their buckets with atomic cursors and then sorts every bucket of two or more entries, which takes the order the atomics
 * landed in out of the result.  Every bucket length from 0 to count works and the host never reads one: a bucket of at most
 * GCN_BUCKET_WAVE_MAX entries is ordered by one wave, one of at most GCN_BUCKET_BLOCK_MAX by a workgroup in LDS, a longer
 * one by a workgroup in place; buckets of 0 or 1 entries get no per-bucket work.
 * ws: device scratch owned by the fill until it has run, at least
 *   16 + 4 * (nbuckets + min(nbuckets, count / 2) + min(nbuckets, count / (GCN_BUCKET_WAVE_MAX + 1))
 *                      + min(nbuckets, count / (GCN_BUCKET_BLOCK_MAX + 1)))  bytes, rounded up to a multiple of 16
 * (integer divisions; `gcn_amd._lib.bucket_ws_bytes`).  Negative sizes, a null pointer where data is required or a short
 * workspace: GCN_ERR_INVALID_ARG.  count == 0 or nbuckets == 0: GCN_OK and no kernel is launched; the count call still
 * zeroes offsets_dev [nbuckets + 1] (offsets[0] = 0 and empty buckets), the fill writes nothing and takes null pointers. */
#define GCN_BUCKET_WAVE_MAX  256
#define GCN_BUCKET_BLOCK_MAX 8192
int gcn_bucket_count_i32(const int32_t* keys_dev, int32_t count, int32_t nbuckets, int32_t* offsets_dev, void* stream);
int gcn_bucket_fill_i32(const int32_t* keys_dev, int32_t count, int32_t nbuckets, const int32_t* offsets_dev /* scanned */,
                        int32_t* perm_dev, void* ws, size_t ws_bytes, void* stream);

/* The arrays of a CSR transpose from the bucketing of its entries by column (keys = col_dev, nbuckets = n: the scanned
 * offsets ARE the transpose's row pointer and perm maps its entries to the source's).  One lane per transposed entry t:
 *   trow_dev[t] = the row r of source entry e = perm_dev[t], i.e. rowptr[r] <= e < rowptr[r + 1] (a binary search in
 *   rowptr_dev [m + 1]); tval_dev[t] = val_dev[e] when val_dev is given.
 * Entries of a transposed row come out in ascending e: ascending source row, repeated (row, column) pairs in source order;
 * they stay separate entries.  An e outside [0, nnz) writes trow = -1, tval = 0 and reads nothing.
 * val_dev and tval_dev are both null (pattern only) or both set.  Negative sizes, a null pointer where data is required,
 * or nnz > 0 with m == 0: GCN_ERR_INVALID_ARG; nnz == 0: GCN_OK, nothing launched. */
int gcn_csr_transpose_gather(const int32_t* rowptr_dev, int32_t m, int32_t nnz, const int32_t* perm_dev,
                             const float* val_dev /* may be NULL */, int32_t* trow_dev, float* tval_dev /* NULL iff val is */,
                             void* stream);

/* Merging the repeated (row, column) entries of a CSR matrix, with the diagonal dropped, filled or added to on the way:
 * what turns an edge list with repeats and mirrors into the pattern of A + A^T, A + I or their union (gcn_amd/coalesce.py),
 * as two calls with the caller's prefix sum between them.  Plan-free like the induced subgraph and under the same rules:
 * the caller's arrays, one memset node and kernels, no allocation, no host read of device data, no global atomics; every
 * output element has one writer, so a call gives the same bits every time.  Every access is a 4-byte one: no pointer
 * needs more than 4-byte alignment.  The contract, exact and meant to be re-implemented (tests/coalesce_ref.py is the
 * numpy twin):
 *   Input: rowptr_dev [m + 1], col_dev [nnz], val_dev [nnz] or NULL (a pattern), n the number of columns.
 *   RUNS.  A run is a maximal stretch of consecutive entries of one row with the same column; its first entry is the head.
 *   With column-sorted rows — the precondition of a full merge; two stable bucketings give that order — a run is exactly
 *   one distinct (row, column) pair.  On unsorted rows the calls stay memory-safe and are defined by the same sentence:
 *   only adjacent equal columns merge.
 *   VALUES.  The value of a run e_0 < ... < e_k is folded in fp32, left to right in entry order, by `reduce`:
 *     GCN_COALESCE_SUM:    acc = val[e_0]; acc += val[e_j]
 *     GCN_COALESCE_MAX:    acc = val[e_0]; acc = (v > acc || v != v) ? v : acc   (a NaN propagates, as in np.maximum)
 *     GCN_COALESCE_MIN:    the same with <
 *     GCN_COALESCE_FIRST:  val[e_0]
 *   The head's lane walks its run: a run costs its length in ONE lane.  Real inputs have runs of 1-3 entries; a run of
 *   thousands is correct and slow.
 *   DIAGONAL.  `diagonal` applies to the rows r < n, whose diagonal column is r (a row r >= n has none):
 *     GCN_DIAG_KEEP:  no special handling.
 *     GCN_DIAG_DROP:  runs with col == r produce no output entry.
 *     GCN_DIAG_FILL:  if no entry of the row has col == r, one entry (r, r, diag_value) is inserted; an existing diagonal
 *                     entry stays as merged.
 *     GCN_DIAG_ADD:   the same insertion, and an existing diagonal run becomes merged + diag_value: one more fp32 add,
 *                     applied last.
 *   The output entries of a row are its heads (less the dropped ones) in entry order.  An inserted entry takes output
 *   position P = the number of heads of the row with col < r, and the heads from that position on move up by one: on a
 *   column-sorted row it sits after the entries with col < r and before those with col > r.  "No entry has col == r" and
 *   P are defined, and computed, without sortedness.
 *   Count:  out_len_dev[r] = the number of output entries of row r.
 *   The caller turns out_len into out_rowptr_dev [m + 1], its exclusive prefix sum, an INPUT of the fill.
 *   Fill, for output entry j = out_rowptr[r] + t of row r:
 *     out_col_dev[j], out_val_dev[j] (when given): the column and the value as above;
 *     out_first_dev[j] (when given): the head's entry index in the input, or -1 for an inserted diagonal;
 *     seg_dev[e] (when given) for every input entry e of the row: the output entry j it was merged into, or -1 when it
 *     was dropped.
 *   val_dev == NULL means a pattern: out_val_dev must then be NULL too, and the reverse (GCN_ERR_INVALID_ARG otherwise).
 * These write nothing for their row: a row pointer outside [0, nnz], and in the fill a row whose out_rowptr length differs
 * from its count (or whose out_rowptr[r] is negative).  Every row length from 0 to nnz works and the host never reads one:
 * a row of at most GCN_SAMPLE_LONG_ROW entries is taken by one wave, a longer one by a 256-thread workgroup.
 * ws: GCN_COALESCE_WS_BYTES of device scratch, owned by the call until it has run.  Negative sizes, a null pointer where
 * data is required (col_dev may be null when nnz == 0; out_first_dev and seg_dev are optional), a short workspace or an
 * unknown reduce / diagonal code: GCN_ERR_INVALID_ARG.  m == 0: GCN_OK, nothing written.  nnz == 0 is an ordinary call:
 * with FILL or ADD it still inserts the diagonals.  A caller whose counts sum to 0 has nothing to fill and skips the second
 * call (every entry was dropped: seg is -1 everywhere). */
#define GCN_COALESCE_WS_BYTES 16
#define GCN_COALESCE_SUM   0
#define GCN_COALESCE_MAX   1
#define GCN_COALESCE_MIN   2
#define GCN_COALESCE_FIRST 3
#define GCN_DIAG_KEEP 0
#define GCN_DIAG_DROP 1
#define GCN_DIAG_FILL 2
#define GCN_DIAG_ADD  3
int gcn_csr_coalesce_count(const int32_t* rowptr_dev, const int32_t* col_dev, int32_t m, int32_t n, int32_t nnz,
                           int32_t diagonal, int32_t* out_len_dev, void* ws, size_t ws_bytes, void* stream);
int gcn_csr_coalesce_fill(const int32_t* rowptr_dev, const int32_t* col_dev, const float* val_dev /* may be NULL */, int32_t m,
                          int32_t n, int32_t nnz, int32_t reduce, int32_t diagonal, float diag_value,
                          const int32_t* out_rowptr_dev, int32_t* out_col_dev, float* out_val_dev /* NULL iff val is */,
                          int32_t* out_first_dev /* may be NULL */, int32_t* seg_dev /* may be NULL */, void* ws,
                          size_t ws_bytes, void* stream);

/* The two kernels of a normalised adjacency on a CSR matrix: its row sums, and the scaled values.  Plan-free, no workspace,
 * no atomics, one writer per element; a wave per row and a 256-thread workgroup per row of more than GCN_SAMPLE_LONG_ROW
 * entries, so no expanded row array and no nnz-sized intermediate exists.  deg_dev is fp64 and needs 8-byte alignment;
 * every other access is a 4-byte one.
 *   Degree:  deg_dev[r] = the sum of val_dev over row r, accumulated in fp64 — or the row's length when val_dev is NULL.
 *   The order of the sum is fixed (the same bits at every call) and otherwise unspecified.
 *   Normalise, for every entry e of row r with column c and v = val_dev[e] (1 when val_dev is NULL), in fp64:
 *     GCN_NORM_SYM (m == n required):  out_val_dev[e] = (float)(s_r * v * s_c),  s_i = deg[i] == 0 ? 0 : 1 / sqrt(deg[i])
 *     GCN_NORM_ROW:                    out_val_dev[e] = (float)(v * t_r),        t_r = deg[r] == 0 ? 0 : 1 / deg[r]
 *   (the zero for a zero degree is the inf -> 0 rule of the usual host formulation).  A column outside [0, n) is not
 *   followed (s_c = 0); a row pointer outside [0, nnz] writes nothing for its row.  out_val_dev may be val_dev.
 * Negative sizes, a null pointer where data is required, an unknown mode or GCN_NORM_SYM with m != n: GCN_ERR_INVALID_ARG;
 * m == 0 (and for the normalisation nnz == 0): GCN_OK, nothing written. */
#define GCN_NORM_SYM 0
#define GCN_NORM_ROW 1
int gcn_csr_degree_f64(const int32_t* rowptr_dev, const float* val_dev /* may be NULL */, int32_t m, int32_t nnz, double* deg_dev,
                       void* stream);
int gcn_csr_normalize_f32(const int32_t* rowptr_dev, const int32_t* col_dev, const float* val_dev /* may be NULL */, int32_t m,
                          int32_t n, int32_t nnz, const double* deg_dev, int32_t mode, float* out_val_dev, void* stream);

/* C = A * B for two CSR matrices (SpGEMM), A [m x p] and B [p x n]: int32 row pointers and columns, fp32 values, a NULL
 * value pointer meaning a pattern (every value 1).  Two calls with the caller's prefix sum between them, plan-free and under
 * the rules of the merge above: the caller's arrays and workspace, one memset node and kernels, no allocation, no host read of
 * device data, no floating-point atomic; the same bits at every call.  Every access is a 4-byte one.  The contract, exact and
 * meant to be re-implemented (tests/spgemm_ref.py is the numpy twin):
 *   PATTERN.  Row i of C has one entry for every column c for which an entry (i, j) of A and an entry (j, c) of B exist.
 *   The pattern is structural: explicit zeros and sums that cancel keep their entry.  The entries of a row ascend by column.
 *   VALUE.  The products of an output entry (i, c) are listed with A's entries of row i, in entry order, as the outer loop and
 *   B's entries of row j, in entry order, as the inner loop.  Each product is fl32(a * b), one rounding, never contracted into
 *   an FMA; the value is the first product, then acc = fl32(acc + product) left to right ("the first product", not 0 +
 *   product: a lone -0.0 stays -0.0).  NaN and infinities propagate as the arithmetic gives them.  A pattern operand counts as
 *   ones; with both operands patterns there are no values: out_val_dev must be NULL exactly then (GCN_ERR_INVALID_ARG
 *   otherwise).
 *   PRECONDITIONS.  A may repeat (row, column) pairs freely: they are more products, in entry order.  B must hold each column
 *   at most once per row (what gcn_csr_coalesce_* returns); its rows need not be sorted.  Where B repeats a column inside a
 *   row, the pattern is still right and the values of the entries that column feeds are unspecified; nothing is written out
 *   of bounds.
 *   An A column outside [0, p) and a B column outside [0, n) contribute nothing.  A row pointer of A outside [0, nnz_a] (or a
 *   descending pair) makes that row of C empty; one of B makes the entries of A that point at that row contribute nothing.
 *   Count:  out_len_dev[i] = the number of entries of row i of C.  The caller turns out_len into out_rowptr_dev [m + 1], its
 *   exclusive prefix sum, an INPUT of the fill.
 *   Fill:  out_col_dev and out_val_dev of every row.  A row whose out_rowptr length differs from its count (or whose
 *   out_rowptr[i] is negative) gets nothing written.
 * HOW A ROW IS TAKEN depends on K_i = min(U_i, n) alone, U_i the number of products of the row (the lengths of the B rows its
 * entries point at, added up), so both calls agree: K_i <= GCN_SPGEMM_WAVE_MAX: a wave with a hash table in LDS;
 * K_i <= GCN_SPGEMM_BLOCK_MAX: a 256-thread workgroup with a hash table in LDS; above: one of GCN_SPGEMM_DENSE_BLOCKS
 * workgroups with n stamps and n floats of the workspace.  A table has the power of two >= 2 K_i slots (at least 64) and is
 * probed linearly from column & (slots - 1).  Every row length from 0 to n works and the host never reads one.
 * ws: device scratch owned by the call until it has run, gcn_spgemm_ws_bytes(m, n) =
 *   16 + 4 * m rounded up to a multiple of 16 + 8 * n * GCN_SPGEMM_DENSE_BLOCKS  bytes; 4-byte alignment is enough.
 * Negative sizes, a null pointer where data is required or a short workspace: GCN_ERR_INVALID_ARG, before any GPU work.
 * m == 0: GCN_OK, nothing written.  nnz_a == 0, nnz_b == 0, p == 0 or n == 0: no product exists; the count zeroes out_len_dev
 * (its only required pointer), the fill writes nothing and needs out_rowptr_dev only.  A caller whose counts sum to 0 has
 * nothing to fill and skips the second call. */
#define GCN_SPGEMM_WAVE_MAX     512
#define GCN_SPGEMM_BLOCK_MAX    8192
#define GCN_SPGEMM_DENSE_BLOCKS 16
int gcn_spgemm_ws_bytes(int32_t m, int32_t n, size_t* bytes);
int gcn_spgemm_count_csr(const int32_t* a_rowptr_dev, const int32_t* a_col_dev, int32_t m, int32_t p, int32_t nnz_a,
                         const int32_t* b_rowptr_dev, const int32_t* b_col_dev, int32_t n, int32_t nnz_b, int32_t* out_len_dev,
                         void* ws, size_t ws_bytes, void* stream);
int gcn_spgemm_fill_csr(const int32_t* a_rowptr_dev, const int32_t* a_col_dev, const float* a_val_dev /* may be NULL */, int32_t m,
                        int32_t p, int32_t nnz_a, const int32_t* b_rowptr_dev, const int32_t* b_col_dev,
                        const float* b_val_dev /* may be NULL */, int32_t n, int32_t nnz_b, const int32_t* out_rowptr_dev,
                        int32_t* out_col_dev, float* out_val_dev /* NULL iff both values are */, void* ws, size_t ws_bytes,
                        void* stream);

/* The product of two CSR matrices SAMPLED ON A PATTERN (an SDDMM with sparse operands): one fp32 value for every entry of a
 * pattern P [mp x np], given as p_rowptr_dev [mp + 1] and p_col_dev [nnz_p].  X and Y are two CSR operands over a common column
 * range [0, w): int32 row pointers and columns, fp32 values, a NULL value pointer meaning ones.  It is what flows back through
 * gcn_spgemm_*: dC/dA on A's pattern, dC/dB on B's, and — on C's own pattern with X = A and Y = B transposed — the values of
 * C, bit for bit as gcn_spgemm_fill_csr gives them (for a fixed output entry every entry of A's row contributes at most one
 * product, so "A's entries in entry order" is the same fold order in both), with no count, no scan and no host read.
 * Plan-free under the rules of the merge above: the caller's arrays and workspace only, one memset node and two kernels (one
 * linear chain under graph capture), no allocation, no host read of device data, no synchronisation, no floating-point
 * atomic; the same bits at every call.  Every access is a 4-byte one and 4-byte alignment is enough.  The contract, exact and
 * meant to be re-implemented (tests/sampled_dot_ref.py is the numpy twin):
 *   ROWS.  For the entry e = (i, j) of P: (xr, yr) = (i, j) when x_by_col == 0 and (j, i) otherwise.  So X has mp rows and Y
 *   has np when x_by_col == 0, and the other way round otherwise (x_rowptr_dev and y_rowptr_dev hold one more word).
 *   VALUE.  out_dev[e] = the sum of x_t * Y[yr, col_t] over the entries t of X's row xr, IN ENTRY ORDER, for which Y's row yr
 *   holds the column col_t.  Each product is fl32(x * y), one rounding, never contracted into an FMA; the value is the first
 *   product, then acc = fl32(acc + product) left to right ("the first product", not 0 + product: a lone -0.0 stays -0.0).  No
 *   match gives +0.0 (all bits zero).  NaN and infinities propagate as the arithmetic gives them.
 *   PRECONDITIONS.  Y's rows ascend strictly by column (sorted, no repeats: what gcn_csr_coalesce_* and the transpose of such
 *   a matrix return).  Where a row of Y does not, the values of the entries that use it are unspecified; every search still
 *   terminates and nothing is accessed out of bounds.  X is free: any order, and repeated columns are more products.
 *   OUT OF RANGE.  An X column outside [0, w) contributes nothing.  A P column outside [0, np) gives +0.0.  A row pointer pair
 *   of X or Y outside [0, nnz] or descending makes that row empty; one of P means nothing is written for that row of P.
 * The work of an entry is the length of its X row.  A row of P of at most GCN_SAMPLE_LONG_ROW entries is taken by one wave,
 * a longer one by a 256-thread workgroup; an X row of any length is walked 16 entries at a time by a 16-lane group (rows of
 * at most 64 entries) or 64 at a time by a wave, never by one lane.
 * ws: GCN_SAMPLED_DOT_WS_BYTES of device scratch, owned by the call until it has run.  Negative sizes, a null pointer where
 * data is required (x_col_dev / y_col_dev may be null when the operand has no entries) or a short workspace:
 * GCN_ERR_INVALID_ARG, before any GPU work.  mp == 0 or nnz_p == 0: GCN_OK, nothing written. */
#define GCN_SAMPLED_DOT_WS_BYTES 16
int gcn_csr_sampled_dot_f32(const int32_t* p_rowptr_dev, const int32_t* p_col_dev, int32_t mp, int32_t np, int32_t nnz_p,
                            const int32_t* x_rowptr_dev, const int32_t* x_col_dev, const float* x_val_dev /* may be NULL */,
                            int32_t nnz_x, const int32_t* y_rowptr_dev, const int32_t* y_col_dev,
                            const float* y_val_dev /* may be NULL */, int32_t nnz_y, int32_t w, int32_t x_by_col, float* out_dev,
                            void* ws, size_t ws_bytes, void* stream);

/* Brute-force k nearest neighbours: for every query row x_i (fp32 [q x d], row stride ldx >= d floats) the k candidate rows
 * y_j (fp32 [n x d], row stride ldy >= d) of smallest squared Euclidean distance.  The q x n distance matrix is never written
 * to memory.  Plan-free: the caller's arrays and workspace, two kernels enqueued on the stream, no allocation, no host read
 * of device data, no synchronisation (one linear chain under graph capture), no floating-point atomic; the same bits at every
 * call.  x and y may be the same array or overlap.  Operands need 4-byte alignment only.  The contract, exact and meant to be
 * re-implemented (tests/knn_ref.py is the numpy twin):
 *   DISTANCE.  d2(i, j) is a pure function of the two rows: one fp32 accumulator starting at 0, the columns c = 0 .. d - 1 in
 *   ascending order, diff = fl32(x_ic - y_jc), acc = fmaf(diff, diff, acc) (one rounding).  It is computed from differences,
 *   never as |x|^2 + |y|^2 - 2 x.y.  So a row is at distance exactly 0 from itself and from a duplicate, d2(a, b) and
 *   d2(b, a) are the same bits, the result does not depend on tile, split or launch shape, and it is within
 *   (d + 4) * 2^-24 relative of the exact value (each term: one rounding of the difference, squared, and one of the fma, on a
 *   sum of non-negative terms).
 *   ORDER.  The key of a candidate is the pair (fp32 bits of d2, index j) compared as unsigned integers: non-negative floats
 *   order as their bits; a NaN distance, of either sign bit, ranks behind every number, +inf included, all NaNs tie, and it
 *   is returned as NaN.  Keys are unique, so the k smallest keys are a unique set.  Output row i lists them ascending by key:
 *   on equal distances the smaller index comes first.  With fewer than k admissible candidates the tail is index -1 and
 *   distance +inf.
 *   SELF EXCLUSION.  self_offset >= 0 makes candidate self_offset + i inadmissible for query i ("x is y, without the point
 *   itself" is 0; "the queries are rows [o, o + q) of y" is o); -1 turns it off.
 *   ROW SUMS.  out_sum_dev (fp64 [q], NULL skips it): sum over ALL n candidates j of sqrt((double) d2(i, j)), the excluded one
 *   too, with its true distance (0 for a self).  The order of the additions depends on nothing but the effective split
 *   count: the same bits at every call; two split counts differ by at most n * 2^-53 relative.
 * HOW THE WORK IS SPREAD.  A 256-thread workgroup owns GCN_KNN_TILE_Q queries and streams candidates through in tiles of
 * GCN_KNN_TILE_C.  The ceil(n / GCN_KNN_TILE_C) tiles are cut into S contiguous parts (part p: tiles [p T / S, (p + 1) T / S));
 * every (query block, part) writes its k smallest keys and its part of the row sum to the workspace and a second kernel, a
 * wave per query, selects among the S * k keys and adds the partial sums in part order.  Apart from the last bits of the row
 * sum the result is identical for every S.  splits >= 1 is taken as given; splits == 0 lets the library choose
 * (NOT MEASURED: a guess that awaits a sweep):  S = ceil(2 * CUs / ceil(q / GCN_KNN_TILE_Q)), at most T / 8.  Either is then
 * clamped to [1, T]: S = gcn_knn_splits(q, n, splits).
 * ws: device scratch owned by the call until it has run, 8-byte aligned, gcn_knn_ws_bytes(q, n, k, splits) =
 *   16 + 8 * q * S * (k + 1) rounded up to a multiple of 16  bytes.
 * GCN_ERR_INVALID_ARG, before any GPU work: negative q, n or splits, k < 1, k > GCN_KNN_K_MAX, d < 1, a stride below d,
 * self_offset < -1, ceil(q / GCN_KNN_TILE_Q) * S >= 2^31, and (with q > 0) a null x, out_idx or ws, a null y with n > 0, a
 * workspace that is short or not 8-byte aligned.  q == 0: GCN_OK, nothing launched.  n == 0: every output row is -1 / +inf and
 * the sums are 0.  out_idx_dev: int32 [q * k]; out_dist2_dev: fp32 [q * k], NULL skips it. */
#define GCN_KNN_K_MAX  64
#define GCN_KNN_TILE_Q 64
#define GCN_KNN_TILE_C 64
int gcn_knn_splits(int32_t q, int32_t n, int32_t splits);                  /* the effective S; -1 for a negative argument */
int gcn_knn_ws_bytes(int32_t q, int32_t n, int32_t k, int32_t splits, size_t* bytes);
int gcn_knn_f32(const float* x_dev, int64_t ldx, const float* y_dev, int64_t ldy, int32_t q, int32_t n, int32_t d, int32_t k,
                int32_t self_offset, int32_t splits, int32_t* out_idx_dev, float* out_dist2_dev /* may be NULL */,
                double* out_sum_dev /* may be NULL */, void* ws, size_t ws_bytes, void* stream);

/* LDS-staged row panels (optional): for matrices whose non-zeros sit near the diagonal (community
 * graphs after Rabbit / RCM / Gorder renumbering) a workgroup stages the feature rows of its panel's
 * column window (512 rows x 64 columns = 128 KiB of LDS) once and sums the in-window non-zeros
 * from LDS; the matrix is split on the device into that staged part and the rest, which the chunk
 * kernel adds in accumulate mode (the split copy costs one extra copy of col/val).  mode 0 = off, 1 = on, -1 = on iff at least half of the
 * non-zeros fall inside their panel's window (measured here, on the device).  When on it is used for
 * k > 32 and takes precedence over slicing; results stay deterministic (rows are summed in CSR order). */
int gcn_spmm_plan_enable_panels(gcn_spmm_plan_t* plan, const int32_t* rowptr_dev,
                                const int32_t* col_dev, const float* val_dev, int32_t mode,
                                void* stream);
int32_t gcn_spmm_plan_panel_rows(const gcn_spmm_plan_t* plan);       /* rows per panel, 0 = off */
/* Panels whose 128 x 512 window holds >= 25 % non-zeros are stored as dense fp32 tiles and contracted on the matrix
 * cores (v_mfma_f32_32x32x2_f32: exact fp32) instead of entry by entry — the BASELINE north_star's "MFMA on the
 * dense row-panel x feature-tile product where nnz-per-panel forms a dense contraction"; a window that holds a
 * non-finite feature value falls back to entry-by-entry sums so that NaN/Inf never reach rows that do not reference
 * them.  Returns how many panels of the plan take that path (0 when panels are off). */
int32_t gcn_spmm_plan_dense_panels(const gcn_spmm_plan_t* plan);
double gcn_spmm_plan_panel_coverage(const gcn_spmm_plan_t* plan);    /* fraction of nnz inside windows */

/* Live kernel timing for bench.py: between _begin and _end every gcn_spmm_csr_f32*
 * call on this plan records a HIP event pair on its launch stream right around the
 * MAIN kernel passes of one SpMM (up to `capacity` SpMM calls).  _end synchronises the events and returns
 * the per-launch durations in milliseconds.  (The reference times with CUDA events
 * from Python, pygcn/perf/dmk.py:71-117.) */
int gcn_spmm_profile_begin(gcn_spmm_plan_t* plan, int32_t capacity);
int gcn_spmm_profile_end(gcn_spmm_plan_t* plan, float* ms_out, int32_t* count_out);

/* One-shot convenience: the schedule is rebuilt on the device at every call into scratch buffers that belong to
 * the calling (device, stream) pair, so concurrent calls on different streams or devices never share state.
 * This is the body of the drop-in `cuspmm` symbol. */
int gcn_spmm_csr_f32_oneshot(const int32_t* rowptr_dev, const int32_t* col_dev,
                     const float* val_dev, const float* B_dev, float* C_dev,
                     int32_t m, int32_t n, int32_t nnz, int32_t k, void* stream);

/* Chains of aggregations (H <- A·H per layer: the multi-GPU pipeline, SGC-style models) without the per-call copy
 * of B.  A sliced plan whose values factor (u_row[r]*u_col[c]) gathers from B' = diag(u_col)·B laid out slice by
 * slice: slice s (columns [s*w, (s+1)*w)) at rows [s*(w+1), (s+1)*(w+1)) of a [table_rows x ld] array, row w of every
 * slice all zero.  gcn_spmm_csr_f32 builds that copy at every call (one pass over B, O(n*k) whatever the matrix
 * holds); `_prelaid_layout` describes it (GCN_ERR_INVALID_ARG when a k-wide SpMM of this plan does not take that
 * pass: k % 4 != 0, no factors, no slicing, ...), and `_prelaid` multiplies with a B' the caller already holds:
 *   out[r + r / out_gap, 0:k] = out_scale[r] * (A·B)[r, 0:k]          (out_gap > 0; out_scale NULL = 1)
 * i.e. the result is written straight INTO the B' layout of a consumer whose slices hold `out_gap` of these rows
 * each (the zero row behind every slice is never touched) and already carries the consumer's column factor — the
 * next layer's call needs no copy at all.  out_gap = 0 writes a plain [m x k] result.  The reference has no
 * counterpart: its flexspmm re-reads B as handed over on every call (flexspmm.cu:499-544). */
int gcn_spmm_plan_prelaid_layout(const gcn_spmm_plan_t* plan, int32_t k, int32_t* slices, int32_t* slice_cols,
                                 int64_t* table_rows, int32_t* ld_floats);
int gcn_spmm_csr_f32_prelaid(gcn_spmm_plan_t* plan, const int32_t* rowptr_dev, const int32_t* col_dev,
                             const float* val_dev, const float* Bp_dev, float* out_dev, const float* out_scale_dev,
                             int32_t out_gap, int32_t k, void* stream);

/* The column-slice count gcn_spmm_plan_enable_slicing(-1) would choose for an m x n matrix with nnz entries
 * (value_free: its values factor, the group kernels run) — host arithmetic; 0 = no slicing.  A caller that must
 * align its own buffers with the slices (the multi-GPU row shards: slices = whole fractions of a rank's rows) asks
 * here first and then passes an explicit count. */
int32_t gcn_spmm_auto_slices(int64_t m, int64_t n, int64_t nnz, int32_t value_free);

/* How the group kernels (csrc/spmm_group.hip) address a slice-by-slice copy of B with `table_rows` rows of
 * `ld_floats` floats: 0 = 32-bit byte offsets (table below 4 GiB and 2^24 rows), 1 = the slice base is added in
 * 64 bits (any size), -1 = not served by them (rows of 128 KiB or more in a table that needs 64 bits, or a
 * stride that is no multiple of 4 floats): such a plan runs the four-per-gather / one-per-gather kernels.
 * Host arithmetic only; the reference has no counterpart (its `int addr = row*k`, flexspmm.cu:67, wraps). */
int32_t gcn_spmm_group_addressing(int64_t table_rows, int32_t ld_floats);

/* ------------------------------------------------------------------------- */
/* (1b) feature-row permutation  dst[r,:] = src[idx[r],:]                     */
/*      replaces flexspmm_v9_permuteX / put_back / permutate()                */
/*      permutate.cu:3-59                                                     */
/* ------------------------------------------------------------------------- */
int gcn_gather_rows_f32(float* dst_dev, const float* src_dev, const int32_t* idx_dev,
                        int32_t nrows, int32_t k, void* stream);

/* ------------------------------------------------------------------------- */
/* (1c) host-side reorderers (CPU, bit-exact with the reference's integer      */
/*      vectors).  rank_out[old] = new, n entries, computed from a CSR graph   */
/*      (one directed edge per stored entry, self-loops included —            */
/*      edgelist.cuh:16-25).                                                  */
/*      order_deg   order_deg.cu:19-45    which: 0 total(in+out) 1 out 2 in   */
/*      order_rcm   order_rcm.cu:15-33 + algo_bfs.cu:11-39                    */
/*      gorder      order_gorder.cu:13-143 + unitheap.cu (RCM∘Gorder)         */
/* ------------------------------------------------------------------------- */
int gcn_order_deg(const int32_t* rowptr, const int32_t* col, int32_t n, int32_t nnz,
                  int32_t which, int32_t desc, int64_t* rank_out);
int gcn_order_rcm(const int32_t* rowptr, const int32_t* col, int32_t n, int32_t nnz,
                  int32_t directed, int64_t* rank_out);
int gcn_order_gorder(const int32_t* rowptr, const int32_t* col, int32_t n, int32_t nnz,
                     int32_t window, int64_t* rank_out);
/* rabbit (renumber.cu:319-520: serial modularity merging, rounds in degree order) WITHOUT the CSR rewrite the
 * drop-in symbol does: vomp_out[new] = old (bit-exact with the reference) and, optionally, the surviving top-level
 * vertex every vertex ended under (community_out; what the parallel version's quality is measured against). */
int gcn_order_rabbit(const int32_t* rowptr, const int32_t* col, int32_t n, int32_t nnz, int32_t* vomp_out,
                     int32_t* community_out);
/* CSR rewrite under a rank: rows/cols relabelled, each row's columns sorted
 * ascending with values carried along (renumber.cu:190-217); vomp_out[new]=old.
 * The order of the values of a repeated (row, column) is unspecified, as in the reference (see (1d)). */
int gcn_csr_apply_rank(int32_t* rowptr, int32_t* col, float* vals, int32_t n, int32_t nnz,
                       const int64_t* rank, int32_t* vomp_out);

/* ------------------------------------------------------------------------- */
/* (1d) the same orderings ON THE DEVICE: device pointers in,   */
/*      int32 rank_out[old] = new on the device, identical integers to the    */
/*      host versions above.  order_rcm_device works on the symmetrised       */
/*      pattern A ∪ Aᵀ (= gcn_order_rcm with directed = 0; for symmetric      */
/*      patterns also directed = 1): component labelling + multi-source       */
/*      level-synchronous BFS whose per-level radix sort reproduces the       */
/*      serial queue order of algo_bfs.cu:11-39 exactly (reorder_device.hip). */
/*      csr_apply_rank_device = gcn_csr_apply_rank out of place (outputs must */
/*      not alias inputs); GCN_ERR_INVALID_ARG if rank is not a permutation.  */
/*      Repeated (row, column) entries keep their STORED order on the device  */
/*      (a stable sort on (new row, new column)): that order is the contract. */
/*      The host gcn_csr_apply_rank sorts a row by column alone with the      */
/*      reference's unstable sort call and leaves the order of repeats        */
/*      unspecified, as the reference does: rowptr, col and vomp agree always, */
/*      the values where no row repeats a column.                             */
/*      All three synchronise the stream before returning.                    */
/* ------------------------------------------------------------------------- */
int gcn_order_deg_device(const int32_t* rowptr_dev, const int32_t* col_dev, int32_t n, int32_t nnz,
                         int32_t which, int32_t desc, int32_t* rank_out_dev, void* stream);
int gcn_order_rcm_device(const int32_t* rowptr_dev, const int32_t* col_dev, int32_t n, int32_t nnz,
                         int32_t* rank_out_dev, int32_t* bfs_levels_out /* host, may be NULL */, void* stream);
int gcn_csr_apply_rank_device(const int32_t* rowptr_dev, const int32_t* col_dev, const float* val_dev,
                              const int32_t* rank_dev, int32_t n, int32_t nnz, int32_t* out_rowptr_dev,
                              int32_t* out_col_dev, float* out_val_dev, int32_t* vomp_out_dev, void* stream);
/* Rabbit ON THE DEVICE: the parallel algorithm the reference's serial code cites as "Rabbit properly" (renumber.cu:
 * 328-330: Arai et al., IPDPS 2016) — every vertex once, in ascending degree order, one wave per vertex; lazy
 * aggregation of the merged vertices' (community, weight) lists; the merge itself is one compare-and-swap on the
 * target's {lock, degree, child} word (csrc/rabbit_device.hip).  NOT the serial code's integers (gcn_order_rabbit /
 * the `rabbit` symbol give those) and not bit-reproducible from run to run (which merges race differs): what is
 * guaranteed is a permutation whose communities reach the serial version's modularity to a few percent (tests).
 * Input: a SYMMETRIC pattern (A = Aᵀ; self-loops ignored; values play no part, as in the reference).
 * rank_out_dev[old] = new; community_out_dev (may be NULL): top-level vertex of every vertex; stats_host (may be NULL,
 * else 8 words): {communities, passes, vertices retried, vertices left top-level for lack of table or pool room, and
 * four guard counters — pointer chain, child chain, full table, bad index}.  Every loop of the kernel is bounded by
 * such a guard; all four are 0 in a sound run, and a non-zero one means an aggregation ran on broken state: the call
 * then returns GCN_ERR_INTERNAL, prints one line and writes NO ordering (the counters are still reported). */
int gcn_order_rabbit_device(const int32_t* rowptr_dev, const int32_t* col_dev, int32_t n, int32_t nnz,
                            int32_t* rank_out_dev, int32_t* community_out_dev, int64_t* stats_host, void* stream);

/* ------------------------------------------------------------------------- */
/* (1e) the "push" form of the multi-GPU layer exchange (gcn_amd/dist.py,      */
/*      exchange="push"; csrc/exchange.hip).  The reference is single-GPU      */
/*      (device 0 hard-coded, flexspmm.cu:507): no counterpart.  Every rank    */
/*      maps its peers' exchange buffers once (IPC handles), writes its shard  */
/*      of a layer output straight into them with the runtime's copy path      */
/*      (no compute units), raises one flag per peer and layer behind the      */
/*      data, and waits for its own flags with one wave.                       */
/* ------------------------------------------------------------------------- */
/* `count` (<= 64) int32 flags, zeroed, in FINE-GRAINED device memory of the current device (a peer's copy engine writes
 * them, a wave of this GPU polls them: coherent at system scope, which ordinary device memory is not promised to be),
 * and the 64-byte IPC handle under which another process maps them (gcn_exchange_flags_open; _close unmaps, _destroy
 * frees — after every peer has closed). */
int gcn_exchange_flags_create(int32_t count, int32_t** flags_dev_out, void* ipc_handle_out_64);
int gcn_exchange_flags_open(const void* ipc_handle_64, int32_t** flags_peer_out);
int gcn_exchange_flags_close(int32_t* flags_peer);
int gcn_exchange_flags_destroy(int32_t* flags_dev);
/* dst_peer[0:bytes] = src[0:bytes]; dst_peer is a pointer into a peer's buffer mapped into this process; asynchronous */
int gcn_exchange_push(void* dst_peer, const void* src, size_t bytes, void* stream);
/* *flag_peer = *value_dev (4 bytes), enqueued behind the pushes on the same stream: "my shard has landed" */
int gcn_exchange_signal(int32_t* flag_peer, const int32_t* value_dev, void* stream);
/* Enqueue ONE wave that returns when flags_dev[i] == value for every i < count (<= 64) except i == skip (-1: none).
 * Bounded: after timeout_seconds a lane gives up and writes 1 + (the flag it waited for) to *status_dev (0 otherwise
 * untouched) — the stream goes on, the caller checks the status word at its next synchronisation point. */
int gcn_exchange_wait(const int32_t* flags_dev, int32_t count, int32_t skip, int32_t value, int32_t* status_dev,
                      double timeout_seconds, void* stream);

/* ------------------------------------------------------------------------- */
/* (2) DROP-IN symbols — identical names and argument lists to the reference.  */
/* ------------------------------------------------------------------------- */

/* Error convention of every drop-in symbol: the reference's (void, print — cuspmm.cu:3-21).  On malformed input,
 * foreign buffers or a HIP failure ONE line goes to stderr ("libgcnspmm: <symbol>: ...") and the call RETURNS with
 * the caller's outputs untouched; nothing aborts the host process. */

/* renumber.so — renumber.cu:23 (dfs), :157 (gorder), :233 (perm_apply), :319 (rabbit).
 * All pointers HOST, CSR rewritten in place, vomp[new] = old. */
void dfs(int* rowPtr, int* col, float* vals, int* vomp, int m, int n, int nnz);
void gorder(int* rowPtr, int* col, float* vals, int* vomp, int m, int n, int nnz);
void perm_apply(int* rowPtr, int* col, float* vals, int* vomp, int m, int n, int nnz);
void rabbit(int* rowPtr, int* col, float* vals, int* vomp, int m, int n, int nnz);

/* tile.so — tile.cu:104-106.  All pointers HOST.  Packs THIS library's plan
 * (not the reference's defective tile-seg arrays, SURVEY defects D1-D3) into the
 * caller's buffers; capacities honoured: seg_rowPtr nnz ints, segNzCV 2*nnz
 * floats, segVoMap nnz ints, grouped_tailSeg/next_seg 256 ints (gcn6.py:334-339).
 * n_segs[0] = nnz / 9, or one less so that its lowest bit tells flexspmm whether the values are u[r]*u[c] (n_segs is the
 * only scalar gcn6 carries from csr2tile to flexspmm, gcn6.py:353-366); needs nnz >= m + 19, else nothing is packed
 * and n_segs[0] = 0.  The matrix is m x n: the row pointer has m + 1 entries and every column index lies in [0, n) —
 * anything else is refused with one line that names m, n and nnz (n_segs[0] = 0, every buffer untouched).  Encoding
 * documented in INTEGRATION.md. */
void csr2tile(int* rowPtr, int* colIdx, float* vals, int m, int n, int nnz,
              int* vo_mp, int* segVoMap, int* seg_rowPtr, float* segNzCV,
              int* grouped_tailSeg, int* next_seg, int tm, int* n_segs);

/* tile.so — tile.cu:11-12: the per-panel helper csr2tile loops over in the reference, exported there as well.  No call
 * site binds it (gcn6.py:341-352 calls csr2tile only) and this library's packing has no per-panel step: the symbol
 * resolves, prints one line to stderr and returns with every buffer (n_segs included) untouched. */
void csr2seg_Cmajor(int ridx, int* rowPtr, int* colIdx, float* vals, int m, int n, int nnz,
                    int* voMp, int* segVoMap, int* seg_rowPtr, float* segNzCV, int tm, int* n_segs);

/* flexspmm.so — flexspmm.cu:499-502.  All pointers DEVICE.  Consumes the arrays
 * written by this library's csr2tile (plain CSR, or — square graphs that qualify for XCD-aware slicing — the group
 * kernels' stream format).  Like the reference's (flexspmm.cu:497-540) the call only ENQUEUES
 * kernels on the legacy default stream (flexspmm.cu:512): in the group format the chunk and cut-row counts are read
 * from the packed header ON THE DEVICE by a one-thread guard kernel (grids sized from upper bounds) — no layer drains
 * the stream.  Only the first call on a given set of buffers reads the 64-byte header once, to report buffers this
 * library did not pack (message, return, C as handed over); a header that disappears later is caught by the guard. */
void flexspmm(int* seg_rowPtr, float* segNzCV, int* segVoMap,
              int* grouped_tailSeg, int* next_seg,
              int m, int n, int k, int n_segs, float* B, float* C);

/* permutate.so — permutate.cu:40-41.  Device pointers; B permuted in place
 * (B[r,:] <- B[voMp[r],:]); labels untouched exactly like the reference
 * (`if (false && lane_id==0)`, permutate.cu:17,35). */
void permutate(float* B, int* voMp, int* labels, int m, int n, int k);

/* cuspmm.so — cuspmm.cu:23-24 (first parameter is declared float* there although
 * it carries the int32 row pointer; kept for signature parity). */
void cuspmm(float* rowPtr, int* col, float* vals, float* X, float* C,
            int m, int n, int nnz, int dim);

#ifdef __cplusplus
}
#endif
#endif /* GCN_SPMM_H */
