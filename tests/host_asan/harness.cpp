// CPU sanitizer leg of libg3hip's host logic ("-fsanitize=address host build of the C-ABI
// shim"): g3py_amd/csrc/g3_host.h is pure C++ and is compiled here with g++ -fsanitize=address,undefined.  Every
// table / schedule builder is driven over the shapes the library produces (and some it never should) and its output
// is checked the way the device consumes it: the tile lookup of the GEMM kernel, the op list of the stripe solve, the
// chunking of the multi-GPU staircase and the segment lists of its steps, the recursion's split point, the panel-width ladder, panel boundaries, the fast-path matcher, the program ring, the jitter schedule, the layout
// of the batched entry points' device buffer, the host expansion of a chain member and the argument checks of the entry
// points that run on a finished factor.
// TEST INFRASTRUCTURE: never linked into the product.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "g3_host.h"

static int g_fail = 0;
#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      if (++g_fail > 20) exit(1);                                       \
    }                                                                   \
  } while (0)

// the device side of the raster: virtual tile id -> (row tile, column tile), as gemm_nt_kernel does it
static void lookup(const RasterTab& tab, int v, int* bm, int* bn) {
  int lo = 0, hi = tab.ngroups;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tab.g[mid].prefix <= v) lo = mid; else hi = mid;
  }
  const int w = v - tab.g[lo].prefix, rows = (int)tab.g[lo].nrows;
  *bn = w / rows;
  *bm = (int)tab.g[lo].row0 + (w - *bn * rows);
}

template <int BM, int BN>
static void check_raster(const GemmShape& sh) {
  RasterTab tab;
  memset(&tab, 0xCD, sizeof(tab));
  const long long nv = build_raster<BM, BN>(sh, &tab);
  if (nv < 0) {   // refused: only legal for very long staircases / block tables
    CHECK(sh.kind == 2 || sh.m / BM > 65535LL * G3_RASTER_MAX);
    return;
  }
  CHECK(tab.ngroups >= 0 && tab.ngroups <= G3_RASTER_MAX);
  CHECK(tab.g[tab.ngroups].prefix == (int)nv);
  for (int g = 0; g + 1 <= tab.ngroups; ++g) CHECK(tab.g[g].prefix <= tab.g[g + 1].prefix);
  // every launched tile: inside C, unique, and (for the wanted region) complete
  std::set<std::pair<int, int>> seen;
  const int64_t tiles_m = sh.m / BM;
  for (long long v = 0; v < nv; ++v) {
    int bm, bn;
    lookup(tab, (int)v, &bm, &bn);
    CHECK(bm >= 0 && bm < tiles_m);
    CHECK(bn >= 0 && (int64_t)bn * BN < sh.n);
    CHECK(seen.insert({bm, bn}).second);
  }
  // coverage: every wanted element's tile was launched
  if (sh.kind == 0) {
    CHECK((long long)seen.size() == tiles_m * (sh.n / BN));
  } else if (sh.kind == 1) {
    for (int64_t i = 0; i < sh.m; i += 61)
      for (int64_t j = 0; j < sh.n; j += 53)
        if (j <= i + sh.off) CHECK(seen.count({(int)(i / BM), (int)(j / BN)}) == 1);
    // and no tile that lies entirely above the shifted diagonal of its group's last row
    for (auto& t : seen) {
      const int64_t last_row_of_group_at_most = ((int64_t)t.first / GROUP_M + 1) * GROUP_M * BM + (int64_t)GROUP_M * BM;
      CHECK((int64_t)t.second * BN <= last_row_of_group_at_most + sh.off + (int64_t)65536 * BM);
    }
  } else {
    int64_t r = 0;
    for (int s = 0; s < sh.nseg; ++s) {
      const bool dg = sh.seg_diag && sh.seg_diag[s];
      const int64_t c0 = sh.seg_cols[s] - sh.seg_rows[s];
      for (int64_t i = 0; i < sh.seg_rows[s]; i += 97)
        for (int64_t j = 0; j < sh.seg_cols[s]; j += 89) {
          const bool wanted = !dg || j <= c0 + i;
          if (wanted) CHECK(seen.count({(int)((r + i) / BM), (int)(j / BN)}) == 1);
        }
      // nothing beyond the segment's width
      for (auto& t : seen)
        if ((int64_t)t.first * BM >= r && (int64_t)t.first * BM < r + sh.seg_rows[s]) CHECK((int64_t)t.second * BN < sh.seg_cols[s]);
      r += sh.seg_rows[s];
    }
    if (sh.b_nb > 0 && sh.b_perm) {
      CHECK(tab.b_nb == (int)sh.b_nb);
      for (int i = 0; i < sh.nperm; ++i) CHECK(tab.b_blk[i] == (unsigned short)sh.b_perm[i]);
    } else {
      CHECK(tab.b_nb == 0);
    }
  }
  // the algorithmic element count is what the profiler divides by: compare with a brute-force count
  double cnt = 0;
  if (sh.kind == 0) cnt = (double)sh.m * sh.n;
  else if (sh.kind == 1) { for (int64_t i = 0; i < sh.m; ++i) { int64_t c = i + sh.off + 1; c = c < 0 ? 0 : (c > sh.n ? sh.n : c); cnt += c; } }
  else for (int s = 0; s < sh.nseg; ++s) {
    cnt += (double)sh.seg_rows[s] * sh.seg_cols[s];
    if (sh.seg_diag && sh.seg_diag[s] && sh.seg_cols[s] >= sh.seg_rows[s]) cnt -= 0.5 * (double)sh.seg_rows[s] * (sh.seg_rows[s] - 1.0);
  }
  CHECK(fabs(shape_elems(sh) - cnt) <= 1e-9 * (cnt + 1));
}

static void test_rasters() {
  std::mt19937 rng(5);
  { GemmShape big{1, 65536 + 128, 1024, 0, 0, nullptr, nullptr, 0, nullptr, 0, nullptr}; check_raster<128, 128>(big); }
  for (int64_t m : {64, 128, 1024, 4096, 30720})
    for (int64_t n : {64, 128, 1024, 4096}) {
      GemmShape d{0, m, n, 0, 0, nullptr, nullptr, 0, nullptr, 0, nullptr};
      check_raster<64, 64>(d);
      if (m % 128 == 0 && n % 128 == 0) check_raster<128, 128>(d);
      for (int64_t off : {(int64_t)0, (int64_t)-128, (int64_t)256, m, -m, (int64_t)1 << 20}) {
        GemmShape t{1, m, n, off, 0, nullptr, nullptr, 0, nullptr, 0, nullptr};
        check_raster<64, 64>(t);
        if (m % 128 == 0 && n % 128 == 0) check_raster<128, 128>(t);
        if (m % 32 == 0 && n % 128 == 0) check_raster<32, 128>(t);
      }
    }
  // staircases: random segments, block tables, diagonal flags, more segments than one table can hold
  for (int it = 0; it < 80; ++it) {
    const int nseg = 1 + (int)(rng() % (it % 10 == 0 ? 260 : 24));
    const int64_t nb = 128 * (1 + rng() % 8);
    std::vector<int64_t> rows(nseg), cols(nseg), diag(nseg);
    int64_t width = 0;
    for (int s = 0; s < nseg; ++s) {
      rows[s] = (rng() % 9 == 0) ? 0 : nb;
      cols[s] = nb * (rng() % (it % 10 == 0 ? 200 : 24));
      diag[s] = (rng() % 2) && cols[s] >= rows[s];
      width = cols[s] > width ? cols[s] : width;
    }
    if (width == 0) continue;
    const int nperm = (int)(width / nb);
    std::vector<int32_t> perm(nperm);
    for (int i = 0; i < nperm; ++i) perm[i] = (int32_t)(rng() % 4096);
    int64_t m = 0;
    for (auto r : rows) m += r;
    if (m == 0) continue;
    const bool with_perm = rng() % 2;
    GemmShape sh{2, m, width, 0, nseg, rows.data(), cols.data(), with_perm ? nb : 0, with_perm ? perm.data() : nullptr,
                 with_perm ? nperm : 0, (rng() % 2) ? diag.data() : nullptr};
    check_raster<128, 128>(sh);
    check_raster<64, 64>(sh);
    // and through the chunker of the multi-GPU driver: the chunks tile the staircase exactly once
    std::vector<G3hStairChunk> ch;
    const int limit = g3h_tune_from_env().stair_max;        // (the test lowers G3_STAIR_MAX)
    g3h_stair_chunks(rows, cols, nb, nperm, &ch, sh.seg_diag ? &diag : nullptr, limit);
    std::map<std::pair<int64_t, int64_t>, int> cover;   // (segment-row block, column block) -> times covered
    for (auto& c : ch) {
      CHECK((int)c.rows.size() <= limit && c.nblk <= limit && c.nblk >= 1);
      CHECK(c.blk0 >= 0 && c.blk0 + c.nblk <= nperm);
      CHECK(c.col0 % nb == 0 && c.col0 == (int64_t)c.blk0 * nb);
      int64_t r = c.row0;
      for (size_t s = 0; s < c.rows.size(); ++s) {
        CHECK(c.cols[s] >= 0 && c.cols[s] <= (int64_t)c.nblk * nb);
        if (c.diag[s]) CHECK(c.cols[s] >= c.rows[s]);
        if (c.rows[s] > 0)
          for (int64_t j = 0; j < c.cols[s]; j += nb) cover[{r, c.col0 + j}]++;
        r += c.rows[s];
      }
      // what the launch itself will build
      GemmShape sub{2, 0, 0, 0, (int)c.rows.size(), c.rows.data(), c.cols.data(), nb, perm.data() + c.blk0, c.nblk,
                    sh.seg_diag ? c.diag.data() : nullptr};
      for (size_t s = 0; s < c.rows.size(); ++s) { sub.m += c.rows[s]; sub.n = c.cols[s] > sub.n ? c.cols[s] : sub.n; }
      if (sub.m > 0 && sub.n > 0) check_raster<128, 128>(sub);
    }
    int64_t r = 0;
    for (int s = 0; s < nseg; ++s) {
      if (rows[s] > 0)
        for (int64_t j = 0; j < cols[s]; j += nb) CHECK((cover[{r, j}] == 1));
      r += rows[s];
    }
    size_t want = 0;
    for (int s = 0; s < nseg; ++s) if (rows[s] > 0) want += (size_t)(cols[s] / nb);
    CHECK(cover.size() == want);
    // exactly one chunk carries each flagged diagonal block
    if (sh.seg_diag) {
      std::vector<int> got(nseg, 0);
      for (auto& c : ch) {
        // segments of a chunk are consecutive segments of the staircase starting at the one whose first row is c.row0
        int s0 = 0; int64_t rr = 0;
        while (s0 < nseg && rr < c.row0) rr += rows[s0++];
        while (s0 < nseg && rows[s0] == 0 && rr == c.row0 && s0 % limit != 0) ++s0;
        for (size_t s = 0; s < c.rows.size() && s0 + (int)s < nseg; ++s) got[(s0 / limit) * limit + s] += c.diag[s] ? 1 : 0;
      }
      for (int s = 0; s < nseg; ++s) if (rows[s] > 0 && diag[s]) CHECK(got[s] == 1);
    }
  }
}

static void test_trsm_ops() {
  // run the op list on the host (one "stripe" of 3 rows) and compare with a direct triangular solve
  std::mt19937 rng(7);
  std::uniform_real_distribution<double> U(-1, 1);
  for (int64_t n = 128; n <= 1024; n += 128) {
    TrsmOps ops;
    memset(&ops, 0xCD, sizeof(ops));
    ops.nops = 0;
    trsm_ops_rec(&ops, 0, n);
    CHECK(ops.nops >= 1 && ops.nops <= G3_TRSM_MAXOPS);
    std::vector<double> L(n * n, 0.0), X(3 * n), X0;
    for (int64_t i = 0; i < n; ++i) { for (int64_t j = 0; j < i; ++j) L[i * n + j] = 0.05 * U(rng); L[i * n + i] = 1.0 + 0.5 * fabs(U(rng)); }
    for (auto& v : X) v = U(rng);
    X0 = X;
    // inverses of the 128 x 128 diagonal blocks
    std::vector<double> W((n / 128) * 128 * 128, 0.0);
    for (int64_t b = 0; b < n / 128; ++b)
      for (int c = 0; c < 128; ++c) {          // column c of inv(L_bb) by forward substitution
        double col[128];
        for (int i = 0; i < 128; ++i) {
          double s = (i == c) ? 1.0 : 0.0;
          for (int j = 0; j < i; ++j) s -= L[(b * 128 + i) * n + b * 128 + j] * col[j];
          col[i] = s / L[(b * 128 + i) * n + b * 128 + i];
        }
        for (int i = 0; i < 128; ++i) W[b * 128 * 128 + i * 128 + c] = col[i];
      }
    for (int q = 0; q < ops.nops; ++q) {
      const auto o = ops.op[q];
      CHECK(o.col >= 0 && o.col + 128 <= n && o.acol >= 0 && o.acol + o.k <= n && o.k > 0 && o.k % 128 == 0);
      for (int r = 0; r < 3; ++r) {
        double out[128];
        for (int c = 0; c < 128; ++c) {
          double s = 0;
          if (o.leaf) {     // X_j <- X_j W_j^T
            CHECK(o.brow >= 0 && o.brow < n / 128 && o.k == 128 && o.acol == o.col);
            for (int t = 0; t < 128; ++t) s += X[r * n + o.acol + t] * W[o.brow * 128 * 128 + c * 128 + t];
            out[c] = s;
          } else {          // X_hi -= X_lo L_hi,lo^T
            CHECK(o.brow == o.col && o.bcol == o.acol && o.acol + o.k <= o.col);
            for (int t = 0; t < o.k; ++t) s += X[r * n + o.acol + t] * L[(o.brow + c) * n + o.bcol + t];
            out[c] = X[r * n + o.col + c] - s;
          }
        }
        for (int c = 0; c < 128; ++c) X[r * n + o.col + c] = out[c];
      }
    }
    // X L^T must equal X0
    double err = 0;
    for (int r = 0; r < 3; ++r)
      for (int64_t j = 0; j < n; ++j) {
        double s = 0;
        for (int64_t t = 0; t <= j; ++t) s += X[r * n + t] * L[j * n + t];
        err = fmax(err, fabs(s - X0[r * n + j]));
      }
    CHECK(err < 1e-10);
  }
}

// the two schedule rules the sweeps share: the recursion's split point and the default panel-width ladder
static void test_split_and_ladder() {
  for (int64_t n = 256; n <= 4096; n += 128) {
    const int64_t n1 = g3h_split_point(n);
    CHECK(n1 >= 128 && n1 <= n - 128);
    CHECK(n1 % 128 == 0);
  }
  const int64_t split[][2] = {{256, 128}, {384, 256}, {640, 384}, {1024, 512}, {2048, 1024}, {3072, 1536}};
  for (auto& p : split) CHECK(g3h_split_point(p[0]) == p[1]);
  const int64_t ladder[][2] = {{4096, 128}, {4224, 256}, {6144, 256}, {6272, 512}, {12288, 512}, {12416, 1024}};
  for (auto& p : ladder) CHECK(g3h_default_panel_width(p[0]) == p[1]);
}

static void test_panel_bounds() {
  for (int64_t n = 128; n <= 70000; n += (n < 2048 ? 128 : 11 * 128 + (n % 1024)))
    for (int64_t NB : {128, 256, 512, 1024, 2048})
      for (int G : {1, 2, 3, 8})
        for (int batch : {1, 16}) {
          const int64_t np = g3h_roundup(n, 128);
          std::vector<int64_t> b;
          std::vector<int> g;
          g3h_panel_bounds(np, NB, G, batch, g3h_tune_from_env(), &b, &g);
          CHECK(b.size() >= 2 && b.front() == 0 && b.back() == np);
          for (size_t i = 0; i + 1 < b.size(); ++i) {
            CHECK(b[i] < b[i + 1] || (i + 2 == b.size() && b[i] <= b[i + 1]));
            CHECK(b[i] % 128 == 0);
            CHECK(b[i + 1] - b[i] <= g3h_roundup(NB, 128) || i + 2 == b.size());
          }
          CHECK(g.front() == 0 && g.back() == (int)b.size() - 1);
          for (size_t i = 0; i + 1 < g.size(); ++i) CHECK(g[i] < g[i + 1] && g[i + 1] - g[i] <= G);
        }
}

static void test_match_and_validate() {
  std::mt19937 rng(11);
  for (int it = 0; it < 6000; ++it) {
    g3_kernel_prog p;
    memset(&p, 0, sizeof(p));
    const bool wild = it % 5 == 0;       // out-of-range structure must be refused by validate before any matching
    p.nleaf = wild ? (int)(rng() % 12) - 2 : 1 + (int)(rng() % 3);
    p.nprod = wild ? (int)(rng() % 20) - 2 : 1 + (int)(rng() % 3);
    const int d = 1 + (int)(rng() % 8);
    for (int l = 0; l < G3_MAXLEAF; ++l) {
      p.leaf[l].kind = wild ? (int)(rng() % 14) - 2 : (int)(rng() % 11);
      p.leaf[l].ndims = wild ? (int)(rng() % 40) - 2 : d;
      for (int k = 0; k < G3_MAXD; ++k) { p.leaf[l].dims[k] = wild ? (int)(rng() % 50) - 5 : (k < d ? k : 0); p.leaf[l].rate[k] = 1.0; p.leaf[l].freq[k] = 0.3; }
      p.leaf[l].var = 1.0; p.leaf[l].alpha = 2.0;
    }
    for (int q = 0; q < G3_MAXPROD; ++q) {
      p.prod[q].coef = (rng() % 7 == 0) ? 2.0 : 1.0;
      p.prod[q].nfac = wild ? (int)(rng() % 7) - 1 : 1 + (int)(rng() % 2 == 0 ? 0 : 1);
      for (int f = 0; f < G3_MAXFAC; ++f) p.prod[q].fac[f] = wild ? (int)(rng() % 12) - 2 : (int)(rng() % (p.nleaf > 0 ? p.nleaf : 1));
    }
    if (g3h_validate_prog(&p, d)) continue;          // the library stops here (status -2)
    int pk;
    SeParams<double, 1> s1; SeParams<double, 2> s2; SeParams<double, 3> s3; SeParams<double, 4> s4; SeParams<double, 8> s8;
    SeParams<float, 16> s16;
    int k = -1;
    k = g3h_match_fast<double, 1>(&p, d, &s1, &pk);
    if (k < 0) k = g3h_match_fast<double, 2>(&p, d, &s2, &pk);
    if (k < 0) k = g3h_match_fast<double, 3>(&p, d, &s3, &pk);
    if (k < 0) k = g3h_match_fast<double, 4>(&p, d, &s4, &pk);
    if (k < 0) k = g3h_match_fast<double, 8>(&p, d, &s8, &pk);
    if (k < 0) k = g3h_match_fast<float, 16>(&p, d, &s16, &pk);
    if (k >= 0) {
      CHECK(k == G3_K_SE || k == G3_K_OU || k == G3_K_MAT32 || k == G3_K_MAT52 || k == G3_K_RQ);
      CHECK(pk == -1 || ((pk == G3_K_COS || pk == G3_K_SIN || pk == G3_K_SM) && (k == G3_K_SE || k == G3_K_MAT32 || k == G3_K_MAT52) && (d == 1 || d == 2 || d == 4 || d == 8)));
      CHECK(p.nprod <= 3 && p.shift == 0.0);
      int two = 0;
      for (int q = 0; q < p.nprod; ++q) { CHECK((p.prod[q].nfac == 1 || p.prod[q].nfac == 2) && p.prod[q].coef == 1.0); two += p.prod[q].nfac == 2; }
      CHECK(two <= 1 && (two == 0 || pk >= 0));      // a two-factor term is stationary * periodic, at most one
    }
  }
}

static void test_ring_and_jitter() {
  bool busy[8] = {false};
  int next = 0, last = -1;
  std::vector<int> order;
  for (int it = 0; it < 100; ++it) {
    bool wait; int mark;
    const int s = g3h_ring_take(busy, 8, &next, &last, &wait, &mark);
    CHECK(s >= 0 && s < 8 && s == it % 8);
    CHECK(mark == (it == 0 ? -1 : (it - 1) % 8));
    CHECK(wait == (it >= 8));          // a slot is only waited for once the ring has wrapped onto it
    CHECK(last == s && !busy[s]);
  }
  // A model of the ring across streams (g3i_upload_prog + g3i_ctx_forget_stream): a slot's event is recorded on the stream the
  // slot was consumed on, when the NEXT slot is taken.  The context alternates between its own stream (0) and the chain
  // streams of drivers that come and go (1, 2, ...: the entry points of the multi-GPU driver switch to them); when a driver is
  // destroyed its drained stream is forgotten.  No take may ever wait for an event of a stream that is gone -- also when the
  // ring had moved back to stream 0 before the destruction, the case a rule that only looks at the current stream misses
  for (int back_first : {0, 1})
    for (int uploads_between : {0, 1, 3}) {
      const int NS = 8;
      bool rb[NS] = {false};
      int rnext = 0, rlast = -1, ev_stream[NS], cur_stream = 0, prog_stream = -1, alive = 0;
      for (int i = 0; i < NS; ++i) ev_stream[i] = -1;
      auto take = [&]() {
        bool wait; int mark;
        const int s = g3h_ring_take(rb, NS, &rnext, &rlast, &wait, &mark);
        if (mark >= 0) { CHECK(prog_stream == 0 || prog_stream == alive); ev_stream[mark] = prog_stream; }
        if (wait) CHECK(ev_stream[s] == 0 || ev_stream[s] == alive);      // never an event of a destroyed stream
        prog_stream = cur_stream;
      };
      for (int driver = 1; driver <= 6; ++driver) {
        alive = driver;
        cur_stream = driver;                       // an entry point: a few programs on the driver's chain stream
        for (int i = 0; i < 3; ++i) take();
        cur_stream = 0;
        if (back_first) for (int i = 0; i < uploads_between; ++i) take();      // ... the caller's own work before the destruction
        // destruction: the chain stream is drained (its events are done), the caller's stream may still be busy
        g3h_ring_forget(rb, NS, &rlast, prog_stream == driver, [&](int i) { return ev_stream[i] == driver; });
        if (prog_stream == driver) prog_stream = -1;
        alive = 0;
        for (int i = 0; i < NS; ++i) CHECK(!(rb[i] && ev_stream[i] == driver));
        if (!back_first) for (int i = 0; i < uploads_between; ++i) take();
      }
    }
  // the reference's schedule: dK = mean * 1e-6 (float32 constant), x10 per retry, lift when min <= 0
  G3hJitter j(2.0, 0.5);
  CHECK(j.lift == 0.0 && fabs(j.value() - 2.0 * (double)1e-6f) < 1e-18 && j.usable());
  double prev = j.value();
  for (int t = 0; t < 19; ++t) { j.next(); CHECK(fabs(j.value() / prev - 10.0) < 1e-12); prev = j.value(); }
  CHECK(j.tries == 19 && G3hJitter::max_tries() == 20);
  G3hJitter k(3.0, -0.25);
  CHECK(fabs(k.lift - (3.0 * (double)1e-6f + 0.25)) < 1e-15 && k.value() > 0.25);
  G3hJitter n(NAN, 1.0);
  CHECK(!n.usable());
}

static void test_dealing() {
  // the multi-GPU driver's block dealing and gather tables: every block has exactly one owner, the rounds keep the
  // counts within one and the ranks' total work (block I weighs I^2 + 6 I + 1) within a few per cent once every rank holds
  // four blocks, the table is injective, rank-major, ascending inside a rank, and never reaches past P * count
  for (int P = 1; P <= 9; ++P)
    for (int nblk = 1; nblk <= 70; nblk += (nblk < 20 ? 1 : 7)) {
      std::vector<int> cnt(P, 0), owner;
      std::vector<double> load(P, 0.0);
      g3h_deal(P, nblk, &owner);
      CHECK((int)owner.size() == nblk);
      for (int I = 0; I < nblk; ++I) {
        const int q = owner[I];
        CHECK(q >= 0 && q < P);
        cnt[q]++;
        load[q] += (double)I * I + 6.0 * I + 1.0;
      }
      int lo = cnt[0], hi = cnt[0];
      double lmax = 0, lsum = 0;
      for (int q = 0; q < P; ++q) { lo = cnt[q] < lo ? cnt[q] : lo; hi = cnt[q] > hi ? cnt[q] : hi; lmax = load[q] > lmax ? load[q] : lmax; lsum += load[q]; }
      CHECK(hi - lo <= 1);
      if (nblk >= 4 * P) CHECK(lmax <= 1.05 * lsum / P);
      for (int a = -1; a < nblk; a += (nblk < 12 ? 1 : 5))
        for (int b = a; b < nblk; b += (nblk < 12 ? 1 : 3)) {
          const int first = a + 1, last = b;          // perm_of(k): k + 1 .. nblk - 1; perm_upto(k): 0 .. k
          std::vector<int32_t> idx;
          const int c = g3h_gather_table(owner, P, first, last, &idx);
          CHECK((int)idx.size() == (last >= first ? last - first + 1 : 0));
          std::vector<int> seen(P * (c > 0 ? c : 1), 0), prev(P, -1);
          for (int I = first; I <= last; ++I) {
            const int t = idx[I - first], q = owner[I];
            CHECK(c > 0 && t >= q * c && t < (q + 1) * c);      // inside the owner's slots
            CHECK(!seen[t]);                                    // injective
            seen[t] = 1;
            CHECK(t > prev[q]);                                 // ascending inside a rank
            prev[q] = t;
          }
        }
    }
}

// the three staircase launches of a step of the multi-GPU sweep (g3h_step_segments), brute force: over every rank and
// step the cells (row block, column block) of a, d1 and d2 are exactly {I owned, I >= k+2, k+1 <= J <= I} plus the
// right-hand-side rows x {k+1 <= J < nblk}, each once; a segment is flagged where its last block is the diagonal one
static void test_step_segments() {
  const int64_t nb = 256;
  const int RHS = -1;       // the row "block" of the right-hand-side rows
  for (int P : {1, 2, 3, 5, 8})
    for (int nblk : {1, 2, 3, 7, 32, 33})
      for (int64_t rr : {(int64_t)0, (int64_t)128, (int64_t)384}) {
        std::vector<int> owner;
        g3h_deal(P, nblk, &owner);
        for (int rank = 0; rank < P; ++rank) {
          std::vector<int> mine;
          std::vector<int64_t> loff(nblk, -1);
          for (int I = 0; I < nblk; ++I)
            if (owner[I] == rank) { loff[I] = (int64_t)mine.size() * nb; mine.push_back(I); }
          const int64_t rows_mat = (int64_t)mine.size() * nb;
          for (int k = 0; k + 1 < nblk; ++k) {
            std::map<std::pair<int, int>, int> cover;
            for (G3hStep which : {G3H_STEP_A, G3H_STEP_D1, G3H_STEP_D2}) {
              const G3hStepSegments s = g3h_step_segments(mine, loff, nb, nblk, rows_mat, rr, k, which);
              CHECK(s.rows.size() == s.cols.size() && s.rows.size() == s.diag.size());
              if (s.rows.empty()) continue;
              CHECK(s.blk0 == (int)which && s.nblk >= 1 && k + 1 + s.blk0 + s.nblk <= nblk);   // inside the gather table of panel k
              int64_t row = s.lo;
              for (size_t i = 0; i < s.rows.size(); ++i) {
                int I = RHS;
                if (row < rows_mat) {          // a row block of the matrix: whole, and where the plan put it
                  CHECK(row % nb == 0 && s.rows[i] == nb);
                  I = mine[(size_t)(row / nb)];
                  CHECK(loff[I] == row);
                } else {
                  CHECK(row == rows_mat && s.rows[i] == rr && rr > 0 && i + 1 == s.rows.size());
                }
                CHECK(s.cols[i] > 0 && s.cols[i] % nb == 0 && s.cols[i] <= (int64_t)s.nblk * nb);
                const int J0 = k + 1 + s.blk0, J1 = J0 + (int)(s.cols[i] / nb) - 1;
                for (int J = J0; J <= J1; ++J) cover[{I, J}]++;
                CHECK((s.diag[i] != 0) == (J1 == I));
                row += s.rows[i];
              }
            }
            size_t want = 0;
            for (int I : mine)
              for (int J = k + 1; I >= k + 2 && J <= I; ++J) { CHECK((cover[{I, J}] == 1)); ++want; }
            for (int J = k + 1; rr > 0 && J < nblk; ++J) { CHECK((cover[{RHS, J}] == 1)); ++want; }
            CHECK(cover.size() == want);
          }
        }
      }
}

// the batched entry points' device buffer (g3h_member_layout) and the host expansion of a chain member (MemberProgs)
static void test_member_layout() {
  const size_t P = sizeof(g3_kernel_prog);
  CHECK(P % 8 == 0);
  for (int batch : {1, 2, 4096})
    for (int nfield : {0, 1, 7, (int)G3_MAX_FIELDS})
      for (int whole : {0, 1})
        for (size_t stat : {(size_t)0, (size_t)batch * 32})
          for (size_t tail : {(size_t)0, (size_t)1000}) {
            const G3hMemberLayout lo = g3h_member_layout(batch, nfield, whole, stat, tail);
            const size_t fbytes = whole ? 0 : (size_t)batch * nfield * 8, obytes = whole ? 0 : ((size_t)nfield * 4 + 15) / 16 * 16;
            // ordered, disjoint: every region ends where the next begins or before it
            CHECK(lo.progs == 0 && lo.progs + batch * P <= lo.stats && lo.stats + stat <= lo.tmpl);
            CHECK(lo.tmpl + (whole ? 0 : P) <= lo.fields && lo.fields + fbytes <= lo.offs && lo.offs + obytes <= lo.tail);
            CHECK(lo.stats % 8 == 0 && lo.tmpl % 8 == 0 && lo.fields % 8 == 0 && lo.offs % 4 == 0);
            CHECK(lo.tail % 256 == 0 && lo.tail - (lo.offs + obytes) < 256 && lo.total == lo.tail + tail);
            // the closed forms the three callers wrote out by hand: programs, [statistics], [template, fields, offsets table]
            CHECK(lo.stats == batch * P && lo.tmpl == batch * P + stat);
            CHECK(lo.fields == lo.tmpl + (whole ? 0 : P) && lo.offs == lo.fields + fbytes);
            CHECK(lo.tail == ((batch * P + stat + (whole ? 0 : P) + fbytes + obytes + 255) & ~(size_t)255));
          }
  // member(b) of the template form == the template patched by hand; of the whole form == the program itself
  std::mt19937 rng(13);
  g3_kernel_prog tmpl;
  memset(&tmpl, 0, sizeof(tmpl));
  tmpl.nleaf = G3_MAXLEAF;
  tmpl.nprod = G3_MAXPROD;
  tmpl.leaf[1].kind = G3_K_DOT;          // its exponent (freq[0]) is structure: never a valid field
  std::vector<int32_t> valid;
  for (int32_t off = -8; off < (int32_t)P + 16; off += 4)
    if (g3h_field_offset_ok_tmpl(&tmpl, off)) valid.push_back(off);
  CHECK(!valid.empty() && valid.size() <= (size_t)G3_MAX_FIELDS);
  CHECK(!g3h_field_offset_ok_tmpl(&tmpl, (int32_t)((char*)&tmpl.leaf[1].freq[0] - (char*)&tmpl)));
  for (int nfield : {0, 1, 7, (int)valid.size()})
    for (int batch : {1, 2, 5}) {
      std::vector<int32_t> offs(valid);
      std::shuffle(offs.begin(), offs.end(), rng);
      offs.resize(nfield);                 // distinct valid offsets, exactly nfield of them (no slack behind the arrays)
      std::vector<double> fields((size_t)batch * nfield);
      for (auto& v : fields) v = (double)(rng() % 1000) + 0.5;
      MemberProgs mp;
      mp.tmpl = &tmpl;
      mp.fields = fields.data();
      mp.offs = offs.data();
      mp.nfield = nfield;
      std::vector<g3_kernel_prog> whole((size_t)batch);
      for (int b = 0; b < batch; ++b) {
        g3_kernel_prog want = tmpl, got;
        memset(&got, 0xCD, sizeof(got));
        for (int i = 0; i < nfield; ++i) *(double*)((char*)&want + offs[i]) = fields[(size_t)b * nfield + i];
        mp.member(b, &got);
        CHECK(!memcmp(&got, &want, sizeof(got)));
        whole[b] = want;
      }
      MemberProgs mw;
      mw.progs = whole.data();
      for (int b = 0; b < batch; ++b) {
        g3_kernel_prog got;
        mw.member(b, &got);
        CHECK(!memcmp(&got, &whole[b], sizeof(got)));
      }
    }
}

// The argument checks of the nine entry points that run on a finished factor or on K^-1, composed from g3_host.h's group
// functions exactly as the entry points compose them (g3_grad.hip, g3_gp_grad.hip, g3_loo.hip): every status the GPU tests
// assert (test_gpu_dloo.py, test_gpu_loo.py, test_gpu_kernels.py), and per entry point two collisions -- two bad arguments at
// once -- with the status that wins.  The lower number wins except where the entry point has always tested out of order.
struct EntryArgs {
  const g3_kernel_prog* prog;     // one program, or the chain's programs
  int batch = 1;
  const g3_grad_map* map;
  const void *X, *L, *invd, *a, *Y, *Kinv, *alpha, *kdiag, *u, *G, *out;
  int64_t N = 100, ldx = 2, ldl = 128, kstride = 256 * 128, ldy = 128, ldc = 128, ldg = 128, row0 = 0, nrows = 100;
  int d = 2, dt = G3_F64;
  size_t es() const { return dt == G3_F64 ? 8 : 4; }
  bool dt_ok() const { return dt == G3_F64 || dt == G3_F32; }
};
static int args_gram_grad_head(const EntryArgs& a) {
  const int rc = g3h_args_prog(a.prog, a.map, 2);
  return rc ? rc : g3h_args_inputs(a.X, a.N, a.ldx, a.d, 4, true);
}
static int args_gram_grad(const EntryArgs& a) {
  if (const int rc = args_gram_grad_head(a)) return rc;
  if (!a.G && a.N > 0) return -9;
  if (a.ldg < a.N) return -10;
  if (!a.alpha && a.N > 0) return -11;
  return a.out ? 0 : -12;
}
static int args_gram_grad_rows(const EntryArgs& a) {
  if (const int rc = args_gram_grad_head(a)) return rc;
  if (a.row0 < 0 || a.row0 % 64) return -9;
  if (a.nrows < 0 || a.row0 + a.nrows > a.N) return -10;
  if (!a.G && a.nrows > 0) return -11;
  if (a.ldg < a.row0 + a.nrows) return -12;
  if (!a.alpha && a.N > 0) return -13;
  return a.out ? 0 : -14;
}
static int args_gram_vjp(const EntryArgs& a) {       // (G, ldg: Kbar and its leading dimension)
  if (const int rc = args_gram_grad_head(a)) return rc;
  if (!a.dt_ok()) return -8;
  if (!a.G && a.N > 0) return -9;
  if (a.ldg < a.N) return -10;
  return a.out ? 0 : -11;
}
static int args_gp_dlogp(const EntryArgs& a) {
  int rc = g3h_args_prog(a.prog, a.map, 2);
  if (!rc) rc = g3h_args_inputs(a.X, a.N, a.ldx, a.d, 4, false);
  if (!rc) rc = g3h_args_factor(a.L, a.N, false, a.ldl, nullptr, a.invd, a.a, a.es(), 8);
  if (!rc) rc = g3h_args_padded_out(a.Y, a.ldy, a.N, a.es(), 13);
  if (!rc) rc = g3h_args_padded_out(a.Kinv, a.ldc, a.N, a.es(), 15);
  if (rc) return rc;
  if (!a.alpha) return -17;
  return a.out ? 0 : -18;
}
static int args_gp_dlogp_batched(const EntryArgs& a) {
  int rc = g3h_args_progs(a.prog, a.batch, a.map, 2);
  if (!rc) rc = g3h_args_inputs(a.X, a.N, a.ldx, a.d, 5, false);
  if (!rc) rc = g3h_args_factor(a.L, a.N, false, a.ldl, &a.kstride, a.invd, a.a, a.es(), 9);
  if (rc) return rc;
  if (!a.Y) return -15;
  if (!a.Kinv) return -16;
  if (!a.alpha) return -17;
  return a.out ? 0 : -18;
}
static int args_gp_dloo(const EntryArgs& a) {
  int rc = g3h_args_prog(a.prog, a.map, 2);
  if (!rc) rc = g3h_args_inputs(a.X, a.N, a.ldx, a.d, 4, false);
  if (rc) return rc;
  if (!a.dt_ok()) return -12;
  rc = g3h_args_factor(a.L, a.N, false, a.ldl, nullptr, a.invd, a.a, a.es(), 8);
  if (!rc) rc = g3h_args_padded_out(a.Y, a.ldy, a.N, a.es(), 13);
  if (!rc) rc = g3h_args_padded_out(a.Kinv, a.ldc, a.N, a.es(), 15);
  if (rc) return rc;
  if (!a.alpha) return -17;
  if (!a.kdiag) return -18;
  if (!a.u) return -19;
  return a.out ? 0 : -20;
}
static int args_gp_dloo_batched(const EntryArgs& a) {       // the whole-programs body of g3_gp_dloo_batched_fields
  int rc = g3h_args_progs(a.prog, a.batch, a.map, 2);
  if (!rc) rc = g3h_args_inputs(a.X, a.N, a.ldx, a.d, 5, false);
  if (rc) return rc;
  if (!a.dt_ok()) return -14;
  rc = g3h_args_factor(a.L, a.N, false, a.ldl, &a.kstride, a.invd, a.a, a.es(), 9);
  if (rc) return rc;
  if (!a.Y) return -15;
  if (!a.Kinv) return -16;
  if (!a.alpha) return -17;
  if (!a.kdiag) return -18;
  if (!a.u) return -19;
  return a.out ? 0 : -20;
}
static int args_gp_loo(const EntryArgs& a) {
  if (!a.dt_ok()) return -7;
  int rc = g3h_args_factor(a.L, a.N, true, a.ldl, nullptr, a.invd, a.a, a.es(), 2);
  if (!rc) rc = g3h_args_padded_out(a.Y, a.ldy, a.N, a.es(), 8);
  if (rc) return rc;
  if (!a.alpha) return -10;
  return a.kdiag ? 0 : -11;
}
static int args_gp_loo_batched(const EntryArgs& a) {
  if (!a.dt_ok()) return -9;
  if (a.batch < 1 || a.batch > G3_MAX_BATCH) return -2;
  if (const int rc = g3h_args_factor(a.L, a.N, true, a.ldl, &a.kstride, a.invd, a.a, a.es(), 3)) return rc;
  if (g3h_roundup(a.N, G3H_LB) > 2 * G3H_LB && !a.Y) return -10;
  if (!a.alpha) return -11;
  return a.kdiag ? 0 : -12;
}

static void test_argument_groups() {
  g3_kernel_prog prog;                    // var * SE(x0, x1) + noise, as the GPU tests' compile_spec(('sum', SE, NOISE), 2)
  memset(&prog, 0, sizeof(prog));
  prog.nleaf = 2;
  prog.nprod = 2;
  prog.leaf[0].kind = G3_K_SE;
  prog.leaf[0].ndims = 2;
  prog.leaf[0].dims[1] = 1;
  prog.leaf[1].kind = G3_K_NOISE;
  for (int q = 0; q < 2; ++q) { prog.prod[q].nfac = 1; prog.prod[q].fac[0] = q; prog.prod[q].coef = 1.0; }
  g3_grad_map map;
  for (int l = 0; l < G3_MAXLEAF; ++l) map.var[l] = map.alpha[l] = map.rate[l] = map.freq[l] = -1;
  map.var[0] = 0; map.rate[0] = 1; map.var[1] = 3; map.nslots = 4;
  CHECK(!g3h_check_map(&prog, &map));
  g3_grad_map badmap = map;               // a slot outside the output
  badmap.var[0] = badmap.nslots;
  g3_kernel_prog badprog = prog;
  badprog.nprod = G3_MAXPROD + 1;
  char mem[8];
  const void* p = mem;                    // never dereferenced: the checks look at pointers, not through them
  EntryArgs ok;
  ok.prog = &prog; ok.map = &map;
  ok.X = ok.L = ok.invd = ok.a = ok.Y = ok.Kinv = ok.alpha = ok.kdiag = ok.u = ok.G = ok.out = p;
  auto with = [&](auto&& change) { EntryArgs a = ok; change(a); return a; };
#define ARGS(...) with([&](EntryArgs& a) { __VA_ARGS__; })
  for (auto f : {args_gram_grad, args_gram_grad_rows, args_gram_vjp, args_gp_dlogp, args_gp_dlogp_batched, args_gp_dloo,
                 args_gp_dloo_batched, args_gp_loo, args_gp_loo_batched}) {
    CHECK(f(ok) == 0);
    CHECK(f(ARGS(a.dt = G3_F32; a.ldl = a.ldy = a.ldc = 132)) == 0);      // rows of 4-byte elements: multiples of 4
  }
  // ---- g3_gp_dloo (test_gpu_dloo.py::test_argument_checks)
  CHECK(args_gp_dloo(ARGS(a.prog = nullptr)) == -2 && args_gp_dloo(ARGS(a.map = nullptr)) == -3);
  CHECK(args_gp_dloo(ARGS(a.X = nullptr)) == -4 && args_gp_dloo(ARGS(a.N = 0)) == -5 && args_gp_dloo(ARGS(a.ldx = 1)) == -6);
  CHECK(args_gp_dloo(ARGS(a.d = 0)) == -7 && args_gp_dloo(ARGS(a.L = nullptr)) == -8);
  CHECK(args_gp_dloo(ARGS(a.N = 129; a.ldy = a.ldc = 256)) == -9);       // ldl below roundup(N, 128)
  CHECK(args_gp_dloo(ARGS(a.invd = nullptr)) == -10 && args_gp_dloo(ARGS(a.a = nullptr)) == -11 && args_gp_dloo(ARGS(a.dt = 7)) == -12);
  CHECK(args_gp_dloo(ARGS(a.Y = nullptr)) == -13 && args_gp_dloo(ARGS(a.ldy = 127)) == -14 && args_gp_dloo(ARGS(a.Kinv = nullptr)) == -15);
  CHECK(args_gp_dloo(ARGS(a.ldc = 127)) == -16 && args_gp_dloo(ARGS(a.alpha = nullptr)) == -17 && args_gp_dloo(ARGS(a.kdiag = nullptr)) == -18);
  CHECK(args_gp_dloo(ARGS(a.u = nullptr)) == -19 && args_gp_dloo(ARGS(a.out = nullptr)) == -20);
  CHECK(args_gp_dloo(ARGS(a.map = &badmap)) == -3 && args_gp_dloo(ARGS(a.prog = &badprog)) == -2);
  CHECK(args_gp_dloo(ARGS(a.prog = &badprog; a.map = nullptr)) == -2);    // collisions
  CHECK(args_gp_dloo(ARGS(a.dt = 7; a.L = nullptr)) == -12);              // dt is tested before the factor
  CHECK(args_gp_dloo(ARGS(a.dt = 7; a.d = 0)) == -7);                     // ... and after the inputs
  CHECK(args_gp_dloo(ARGS(a.ldx = 1; a.d = 0)) == -7);                    // d before ldx, which is measured against it
  // ---- g3_gp_dloo_batched_fields: the whole-programs body's codes, three places further from -4 on
  auto many = [&](const EntryArgs& a) { return g3h_fields_status(args_gp_dloo_batched(a), -20); };
  CHECK(many(ARGS(a.batch = 0)) == -3 && many(ARGS(a.batch = G3_MAX_BATCH + 1)) == -3 && many(ARGS(a.map = nullptr)) == -7);
  CHECK(many(ARGS(a.X = nullptr)) == -8 && many(ARGS(a.N = 0)) == -9 && many(ARGS(a.ldx = 1)) == -10 && many(ARGS(a.d = 0)) == -11);
  CHECK(many(ARGS(a.L = nullptr)) == -12 && many(ARGS(a.ldl = 127)) == -13);
  CHECK(many(ARGS(a.kstride = 127 * 128)) == -14);                         // members would overlap
  CHECK(many(ARGS(a.invd = nullptr)) == -15 && many(ARGS(a.a = nullptr)) == -16 && many(ARGS(a.dt = 7)) == -17);
  CHECK(many(ARGS(a.Y = nullptr)) == -18 && many(ARGS(a.Kinv = nullptr)) == -19 && many(ARGS(a.alpha = nullptr)) == -20);
  CHECK(many(ARGS(a.kdiag = nullptr)) == -21 && many(ARGS(a.u = nullptr)) == -22 && many(ARGS(a.out = nullptr)) == -23);
  CHECK(g3h_fields_status(-2, -20) == -2 && g3h_fields_status(-3, -20) == -3 && g3h_fields_status(-21, -20) == -21);
  CHECK(g3h_fields_status(-100, -20) == -100 && g3h_fields_status(0, -20) == 0);      // G3_ERR_*: not argument numbers
  CHECK(args_gp_dloo_batched(ARGS(a.map = nullptr; a.prog = &badprog)) == -4);        // collisions: the missing map is refused
  CHECK(args_gp_dloo_batched(ARGS(a.map = &badmap; a.prog = &badprog)) == -2);        // before a member is looked at
  CHECK(args_gp_dloo_batched(ARGS(a.dt = 7; a.kstride = 1)) == -14);
  // ---- g3_gp_dlogp, g3_gp_dlogp_batched: the same numbers without dt, kdiag and u
  CHECK(args_gp_dlogp(ARGS(a.prog = nullptr)) == -2 && args_gp_dlogp(ARGS(a.map = &badmap)) == -3 && args_gp_dlogp(ARGS(a.N = 0)) == -5);
  CHECK(args_gp_dlogp(ARGS(a.ldl = 127)) == -9 && args_gp_dlogp(ARGS(a.ldy = 127)) == -14 && args_gp_dlogp(ARGS(a.ldc = 127)) == -16);
  CHECK(args_gp_dlogp(ARGS(a.alpha = nullptr)) == -17 && args_gp_dlogp(ARGS(a.out = nullptr)) == -18);
  CHECK(args_gp_dlogp(ARGS(a.dt = 7)) == 0);                               // no test of dt: anything but G3_F64 is float
  CHECK(args_gp_dlogp(ARGS(a.dt = G3_F32; a.ldl = 130)) == -9);            // ... whose rows are multiples of 4 elements
  CHECK(args_gp_dlogp(ARGS(a.invd = nullptr; a.Y = nullptr)) == -10 && args_gp_dlogp(ARGS(a.Kinv = nullptr; a.ldy = 127)) == -14);
  CHECK(args_gp_dlogp_batched(ARGS(a.prog = nullptr)) == -2 && args_gp_dlogp_batched(ARGS(a.batch = 0)) == -3);
  CHECK(args_gp_dlogp_batched(ARGS(a.map = nullptr)) == -4 && args_gp_dlogp_batched(ARGS(a.map = &badmap)) == -4);
  CHECK(args_gp_dlogp_batched(ARGS(a.kstride = 128 * 128 + 1)) == -11 && args_gp_dlogp_batched(ARGS(a.a = nullptr)) == -13);
  CHECK(args_gp_dlogp_batched(ARGS(a.Y = nullptr)) == -15 && args_gp_dlogp_batched(ARGS(a.out = nullptr)) == -18);
  CHECK(args_gp_dlogp_batched(ARGS(a.dt = 7)) == 0);
  CHECK(args_gp_dlogp_batched(ARGS(a.batch = 0; a.map = nullptr)) == -3 && args_gp_dlogp_batched(ARGS(a.ldl = 127; a.kstride = 1)) == -10);
  {   // the second member is looked at too
    g3_kernel_prog two[2] = {prog, badprog};
    CHECK(args_gp_dlogp_batched(ARGS(a.prog = two; a.batch = 2)) == -2 && args_gp_dlogp_batched(ARGS(a.prog = two; a.batch = 1)) == 0);
  }
  // ---- g3_gram_grad, g3_gram_grad_rows, g3_gram_vjp (test_gpu_kernels.py): N == 0 with null pointers is a valid call
  CHECK(args_gram_grad(ARGS(a.N = 10; a.ldx = 1)) == -6 && args_gram_grad(ARGS(a.N = 10; a.map = &badmap)) == -3);
  CHECK(args_gram_grad(ARGS(a.N = 0; a.X = a.G = a.alpha = nullptr)) == 0 && args_gram_grad(ARGS(a.X = nullptr)) == -4);
  CHECK(args_gram_grad(ARGS(a.N = -1)) == -5 && args_gram_grad(ARGS(a.G = nullptr)) == -9 && args_gram_grad(ARGS(a.ldg = 99)) == -10);
  CHECK(args_gram_grad(ARGS(a.alpha = nullptr)) == -11 && args_gram_grad(ARGS(a.out = nullptr)) == -12 && args_gram_grad(ARGS(a.dt = 7)) == 0);
  CHECK(args_gram_grad(ARGS(a.N = -1; a.X = nullptr)) == -5 && args_gram_grad(ARGS(a.d = 41; a.G = nullptr)) == -7);
  CHECK(args_gram_grad_rows(ARGS(a.row0 = 32)) == -9 && args_gram_grad_rows(ARGS(a.row0 = 64; a.nrows = 37)) == -10);
  CHECK(args_gram_grad_rows(ARGS(a.G = nullptr)) == -11 && args_gram_grad_rows(ARGS(a.ldg = 99)) == -12);
  CHECK(args_gram_grad_rows(ARGS(a.alpha = nullptr)) == -13 && args_gram_grad_rows(ARGS(a.out = nullptr)) == -14);
  CHECK(args_gram_grad_rows(ARGS(a.N = 0; a.nrows = 0; a.X = a.G = a.alpha = nullptr)) == 0);
  CHECK(args_gram_grad_rows(ARGS(a.prog = nullptr; a.row0 = 1)) == -2 && args_gram_grad_rows(ARGS(a.row0 = 1; a.nrows = -1)) == -9);
  CHECK(args_gram_vjp(ARGS(a.dt = 7)) == -8 && args_gram_vjp(ARGS(a.G = nullptr)) == -9 && args_gram_vjp(ARGS(a.ldg = 99)) == -10);
  CHECK(args_gram_vjp(ARGS(a.out = nullptr)) == -11 && args_gram_vjp(ARGS(a.N = 0; a.X = a.G = nullptr)) == 0);
  CHECK(args_gram_vjp(ARGS(a.dt = 7; a.ldx = 1)) == -6 && args_gram_vjp(ARGS(a.dt = 7; a.out = nullptr)) == -8);
  // ---- g3_gp_loo, g3_gp_loo_batched (test_gpu_loo.py::test_argument_checks): dt first of all, N between L and ldl
  CHECK(args_gp_loo(ARGS(a.L = nullptr)) == -2 && args_gp_loo(ARGS(a.N = 0)) == -3);
  CHECK(args_gp_loo(ARGS(a.N = 129; a.ldy = 256)) == -4);                  // ldl below roundup(N, 128)
  CHECK(args_gp_loo(ARGS(a.invd = nullptr)) == -5 && args_gp_loo(ARGS(a.a = nullptr)) == -6 && args_gp_loo(ARGS(a.dt = 7)) == -7);
  CHECK(args_gp_loo(ARGS(a.Y = nullptr)) == -8 && args_gp_loo(ARGS(a.ldy = 127)) == -9 && args_gp_loo(ARGS(a.alpha = nullptr)) == -10);
  CHECK(args_gp_loo(ARGS(a.kdiag = nullptr)) == -11);
  CHECK(args_gp_loo(ARGS(a.dt = 7; a.L = nullptr)) == -7 && args_gp_loo(ARGS(a.N = 0; a.ldl = 0; a.L = nullptr)) == -2);
  CHECK(args_gp_loo(ARGS(a.N = 0; a.ldl = 127)) == -3);
  CHECK(args_gp_loo_batched(ARGS(a.batch = 0; a.Y = nullptr)) == -2 && args_gp_loo_batched(ARGS(a.batch = 4097; a.Y = nullptr)) == -2);
  CHECK(args_gp_loo_batched(ARGS(a.L = nullptr)) == -3 && args_gp_loo_batched(ARGS(a.N = 0)) == -4 && args_gp_loo_batched(ARGS(a.ldl = 127)) == -5);
  CHECK(args_gp_loo_batched(ARGS(a.kstride = 127 * 128; a.Y = nullptr)) == -6);      // members would overlap
  CHECK(args_gp_loo_batched(ARGS(a.invd = nullptr)) == -7 && args_gp_loo_batched(ARGS(a.a = nullptr)) == -8 && args_gp_loo_batched(ARGS(a.dt = 7)) == -9);
  CHECK(args_gp_loo_batched(ARGS(a.N = 300; a.ldl = 384; a.kstride = 512 * 384; a.Y = nullptr)) == -10);   // N > 256 needs the Y workspace
  CHECK(args_gp_loo_batched(ARGS(a.N = 300; a.ldl = 384; a.kstride = 512 * 384; a.Y = a.alpha = a.kdiag = nullptr)) == -10);
  CHECK(args_gp_loo_batched(ARGS(a.Y = nullptr)) == 0);                    // ... and no other
  CHECK(args_gp_loo_batched(ARGS(a.Y = a.alpha = nullptr)) == -11 && args_gp_loo_batched(ARGS(a.Y = a.kdiag = nullptr)) == -12);
  CHECK(args_gp_loo_batched(ARGS(a.dt = 7; a.batch = 0)) == -9 && args_gp_loo_batched(ARGS(a.batch = 0; a.L = nullptr)) == -2);
#undef ARGS
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "deal")) {        // "deal P nblk": print the table (the Python twin must deal identically)
    std::vector<int> owner;
    g3h_deal(atoi(argv[2]), atoi(argv[3]), &owner);
    for (int q : owner) printf("%d ", q);
    printf("\n");
    return 0;
  }
  test_dealing();
  test_step_segments();
  test_rasters();
  test_trsm_ops();
  test_split_and_ladder();
  test_panel_bounds();
  test_match_and_validate();
  test_ring_and_jitter();
  test_member_layout();
  test_argument_groups();
  if (g_fail) { fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
  printf("host_asan ok\n");
  return 0;
}
