// The row cursor of the chunk-schedule SpMM kernels (gcn_amd/csrc/chunk_walk.h: GCN_ROW_WALK_OPEN / _NEXT, next_nonempty_row) under
// AddressSanitizer + UBSan, against a serial walk (CPU only; built and run by tests/test_chunk_walk_sanitizers.py).
// Every chunk of seeded row pointers is driven the way the kernels drive it — consume min(step, entries left in the row),
// next() at every row end — and each emitted piece is recorded as (row, from, to, kind).  The pieces must tile every
// non-empty row exactly once; the kinds must be the ones spmm_fixup_kernel's ownership rule expects.  rowptr and chunk_row
// live in heap arrays of exactly m + 1 and nchunks ints, so a read outside them is an ASan report.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../gcn_amd/csrc/chunk_walk.h"

enum Kind { WHOLE, SLOT_EVEN, SLOT_ODD };               // into C; slab slot 2c; slab slot 2c + 1
struct Piece { int row, from, to, kind, chunk; };

static int g_walks = 0;
static struct { int span3, ends_on, begins_on, run65, last_empty, ragged, exact, all_empty; } g_seen;

#define REQUIRE(cond, ...)                                                                         \
  do { if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n  ", __FILE__, __LINE__, #cond);     \
                      std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); std::exit(2); } } while (0)

// plan_chunk_rows_kernel (spmm_kernels.hip), thread c
static int plan_chunk_row(const int* rowptr, int m, int T, int c) {
  if (c == 0) return 0;
  const long long target = (long long)c * T;
  int lo = 0, hi = m + 1;                               // first index i in [0, m] with rowptr[i] > target
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if ((long long)rowptr[mid] > target) hi = mid; else lo = mid + 1;
  }
  return lo - 1;
}

static void walk(const std::vector<int>& len, int T, int step, const char* name) {
  const int m = (int)len.size();
  int* rowptr = new int[(size_t)m + 1];                 // exactly m + 1: the redzone starts at rowptr[m + 1]
  rowptr[0] = 0;
  for (int r = 0; r < m; ++r) rowptr[r + 1] = rowptr[r] + len[(size_t)r];
  const int nnz = rowptr[m];
  const int nchunks = (int)(((long long)nnz + T - 1) / T);
  int* chunk_row = new int[(size_t)std::max(nchunks, 1)];
  for (int c = 0; c < nchunks; ++c) chunk_row[c] = plan_chunk_row(rowptr, m, T, c);

  std::vector<std::vector<Piece>> of_row((size_t)m);
  for (int c = 0; c < nchunks; ++c) {
    const int start = c * T, end = std::min(start + T, nnz);
    const int* const rp = rowptr;                       // (the macros index what they are given: the exact-size arrays)
    const int* const cr = chunk_row;
    GCN_ROW_WALK_OPEN(rp, cr, c, T, m);                 // r, row_end, row_end_nx, head, pos, last_flush
    REQUIRE(pos == start && last_flush == start, "%s T=%d chunk %d opens at %d", name, T, c, pos);
    auto emit = [&](int to, int kind) {
      REQUIRE(r >= 0 && r < m, "%s T=%d step=%d chunk %d: piece for row %d", name, T, step, c, r);
      of_row[(size_t)r].push_back(Piece{r, last_flush, to, kind, c});
    };
    auto flush = [&]() {                                // what every kernel's flush does, without the sums
      if (head) emit(pos, SLOT_EVEN);
      else if (last_flush != pos) emit(pos, WHOLE);
      GCN_ROW_WALK_NEXT(rp, m)
    };
    while (pos == row_end) flush();                     // leading empty rows
    while (pos < end) {
      REQUIRE(row_end > pos, "%s T=%d step=%d chunk %d: row_end %d at pos %d", name, T, step, c, row_end, pos);
      pos += std::min(step, std::min(row_end, end) - pos);
      while (pos == row_end) flush();
    }
    REQUIRE(pos == end, "%s T=%d step=%d chunk %d: stopped at %d, not %d", name, T, step, c, pos, end);
    if (last_flush != end) emit(end, head ? SLOT_EVEN : SLOT_ODD);
  }

  int empty_run = 0;
  for (int r = 0; r < m; ++r) {
    const int rs = rowptr[r], re = rowptr[r + 1];
    const std::vector<Piece>& ps = of_row[(size_t)r];
    if (rs == re) {
      REQUIRE(ps.empty(), "%s T=%d step=%d: %zu pieces for empty row %d", name, T, step, ps.size(), r);
      if (++empty_run > 64) g_seen.run65 = 1;
      continue;
    }
    empty_run = 0;
    REQUIRE(!ps.empty(), "%s T=%d step=%d: no piece for row %d [%d, %d)", name, T, step, r, rs, re);
    int at = rs;                                        // the pieces tile [rs, re) once, in order
    for (const Piece& p : ps) {
      REQUIRE(p.from == at && p.to > p.from, "%s T=%d step=%d: row %d piece [%d, %d) at %d", name, T, step, r, p.from, p.to, at);
      at = p.to;
    }
    REQUIRE(at == re, "%s T=%d step=%d: row %d covered to %d of %d", name, T, step, r, at, re);
    const int c0 = rs / T, c1 = (re - 1) / T;
    if (c0 == c1) {                                     // inside one chunk: one whole-row piece
      REQUIRE(ps.size() == 1 && ps[0].kind == WHOLE && ps[0].chunk == c0, "%s T=%d step=%d: row %d in chunk %d: %zu pieces, kind %d",
              name, T, step, r, c0, ps.size(), ps[0].kind);
    } else {                                            // cut: slot 2c0 + 1, then slot 2c of every later chunk
      REQUIRE((int)ps.size() == c1 - c0 + 1, "%s T=%d step=%d: row %d spans chunks %d..%d in %zu pieces", name, T, step, r, c0, c1, ps.size());
      for (int i = 0; i <= c1 - c0; ++i)
        REQUIRE(ps[(size_t)i].chunk == c0 + i && ps[(size_t)i].kind == (i == 0 ? SLOT_ODD : SLOT_EVEN),
                "%s T=%d step=%d: row %d piece %d: chunk %d kind %d", name, T, step, r, i, ps[(size_t)i].chunk, ps[(size_t)i].kind);
      if (c1 - c0 >= 2) g_seen.span3 = 1;
    }
    if (re % T == 0) g_seen.ends_on = 1;
    if (rs % T == 0 && rs > 0) g_seen.begins_on = 1;
  }

  // spmm_fixup_kernel: boundary c owns row chunk_row[c] when it is the first boundary inside the row, and adds
  // P[2(c-1)+1] + P[2c] + ... + P[2c1].  Those must be exactly the slab pieces the walk emitted, for exactly the cut rows.
  std::vector<int> owned((size_t)m, 0);
  for (int c = 1; c < nchunks; ++c) {
    const int r = chunk_row[c], rs = rowptr[r];
    if (!(rs < (long long)c * T && rs / T == c - 1)) continue;
    const int re = rowptr[r + 1], c1 = (re - 1) / T;
    const std::vector<Piece>& ps = of_row[(size_t)r];
    REQUIRE(++owned[(size_t)r] == 1, "%s T=%d: row %d owned twice", name, T, r);
    REQUIRE((int)ps.size() == c1 - (c - 1) + 1 && ps[0].kind == SLOT_ODD && ps[0].chunk == c - 1,
            "%s T=%d step=%d: fix-up of boundary %d, row %d: %zu pieces", name, T, step, c, r, ps.size());
    for (int cc = c; cc <= c1; ++cc)
      REQUIRE(ps[(size_t)(cc - c + 1)].kind == SLOT_EVEN && ps[(size_t)(cc - c + 1)].chunk == cc,
              "%s T=%d step=%d: fix-up adds slot %d of row %d, the walk did not write it", name, T, step, 2 * cc, r);
  }
  for (int r = 0; r < m; ++r) {
    const bool cut = !of_row[(size_t)r].empty() && of_row[(size_t)r][0].kind != WHOLE;
    REQUIRE(cut == (owned[(size_t)r] == 1), "%s T=%d step=%d: row %d cut %d, owned %d", name, T, step, r, (int)cut, owned[(size_t)r]);
  }

  if (nnz == 0) g_seen.all_empty = 1;
  else if (nnz % T) g_seen.ragged = 1; else g_seen.exact = 1;
  if (m > 1 && len.back() == 0 && nnz > 0) g_seen.last_empty = 1;
  ++g_walks;
  delete[] rowptr;
  delete[] chunk_row;
}

static void run(const std::vector<int>& len, int T, const char* name) {
  for (int step : {1, 4, 16, 64}) walk(len, T, step, name);
  long long nnz = 0;
  for (int l : len) nnz += l;
  std::printf("%s ok (m=%zu T=%d nnz=%lld)\n", name, len.size(), T, nnz);
}

int main() {
  std::mt19937 rng(20240611);
  auto small = [&]() { return (int)(rng() % 41); };
  int cases = 0;
  for (int m : {1, 2, 65, 300}) for (int T : {64, 128}) {
    auto fit = [&](std::vector<int> v) { v.resize((size_t)m, 0); return v; };
    // the whole matrix empty
    run(std::vector<int>((size_t)m, 0), T, "all empty"); ++cases;
    // a row over four chunks first, ragged nnz, the last row empty
    { std::vector<int> v((size_t)m); for (int& l : v) l = small(); v[0] = 3 * T + 5; if (m > 1) v.back() = 0;
      run(v, T, "long first row, last row empty"); ++cases; }
    // rows that end on a chunk boundary, begin on one, are cut and end on one; three empty rows in between; then a row
    // from boundary to boundary over two chunks and one over three chunks and one entry; nnz a multiple of T when all fit
    { std::vector<int> v = fit({T - 10, 10, 7, T - 7, 0, 0, 0, 2 * T, 3 * T + 1, T - 1});
      run(v, T, "chunk boundaries"); ++cases; }
    { std::vector<int> v = fit({T - 10, 10 + T}); run(v, T, "cut row ending on a boundary"); ++cases; }
    // leading, middle and trailing runs of empty rows (longer than 64 where m allows)
    { std::vector<int> v((size_t)m); for (int& l : v) l = 1 + small();
      const int run_len = m >= 300 ? 70 : m / 4;
      for (int i = 0; i < run_len; ++i) { v[(size_t)i] = 0; v[(size_t)(m / 2 + i)] = 0; v[(size_t)(m - 1 - i)] = 0; }
      if (m >= 4) v[(size_t)(m / 2 - 1)] = 2 * T + 3;   // a cut row right in front of the middle run
      run(v, T, "empty runs"); ++cases; }
    // seeded: 30 % empty rows, now and then a row of more than two chunks
    for (int rep = 0; rep < 3; ++rep) {
      std::vector<int> v((size_t)m);
      for (int& l : v) { const unsigned x = rng() % 100; l = x < 30 ? 0 : (x < 33 ? 2 * T + (int)(rng() % (2 * T)) : 1 + (int)(rng() % 50)); }
      run(v, T, "seeded"); ++cases;
    }
  }
  REQUIRE(g_seen.span3 && g_seen.ends_on && g_seen.begins_on && g_seen.run65 && g_seen.last_empty && g_seen.ragged &&
          g_seen.exact && g_seen.all_empty, "the sweep missed a shape: %d %d %d %d %d %d %d %d", g_seen.span3, g_seen.ends_on,
          g_seen.begins_on, g_seen.run65, g_seen.last_empty, g_seen.ragged, g_seen.exact, g_seen.all_empty);
  std::printf("chunk walk ok: %d cases, %d walks\n", cases, g_walks);
  return 0;
}
