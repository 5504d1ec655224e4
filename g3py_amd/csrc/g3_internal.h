// Internal declarations shared by the libg3hip translation units (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "g3hip.h"
#include "g3_host.h"
#include "g3_reduce.h"

#define G3_LB 128   // diagonal block factored + inverted by ONE fused kernel; matrices are padded to it

#define G3_PROG_SLOTS 8
struct g3_ctx {
  int device;
  hipStream_t stream;      // stream work is enqueued on
  hipStream_t own_stream;  // created by the context
  hipStream_t side_stream; // low-priority stream carrying the bulk trailing updates (look-ahead)
  hipStream_t side_for;    // the stream the side stream's placement was probed against (g3i_ensure_side_stream)
  hipEvent_t* la_ev;       // event pool of the two-stream sweeps (g3i_ensure_events)
  int la_nev;
  bool in_sweep;           // a two-stream sweep owns the side stream and the event pool (g3_sweep_scope)
  G3hTune tune;            // tuning knobs, read from the environment once at g3_ctx_create
  unsigned long long gram_paths[3];   // Gram launches so far: compile-time table, generated at first use, interpreted
  unsigned long long grad_paths[3];   // the same for the gradient's kernel-parameter sums
  FILE* gemm_log;          // G3_GEMM_LOG=<file>: one line per MFMA GEMM / stripe-solve launch (scripts/launch_table.py)
  bool info_clean;         // d_info is known to be zero: left so by a synchronised evaluation (info_stream == nullptr and
                           // info_sync), or cleared on info_stream with no factorisation queued since (g3i_reset_info)
  bool info_sync;
  hipStream_t info_stream;
  bool adopted;            // stream belongs to the caller
  bool bulk_role;          // this context's stream carries bulk updates beside another context's chain (multi-GPU driver)
  // batch mode (g3_gp_factor_batched): every MFMA GEMM and diagonal-block launch of a sweep acts on
  // `batch` matrices at once (grid.y); operands inside the block-inverse buffer [bw_base, +bw_bytes)
  // are `bstride_w` elements apart, everything else `bstride` elements
  int batch;
  int64_t bstride, bstride_w;
  const char* bw_base;
  size_t bw_bytes;
  int64_t gram_diag_off;   // row offset of the block g3_gram_rows is building (0 otherwise)
  void* bbuf;              // device scratch of the batched entry points (programs, statistics)
  size_t bbuf_bytes;
  // small device scratch
  int* d_info;             // potrf info flag (one per batch member, G3_MAX_BATCH of them)
  double* d_stats;         // 64 doubles of reduction outputs
  g3_kernel_prog* d_prog;  // kernel programs (device copies, a ring of G3_PROG_SLOTS)
  hipEvent_t prog_ev[G3_PROG_SLOTS];   // recorded behind the launch that read the slot
  bool prog_busy[G3_PROG_SLOTS];
  int prog_next, prog_last;
  hipStream_t prog_stream;   // stream the last slot was uploaded / consumed on
  // pinned host mirrors
  int* h_info;
  double* h_stats;
  g3_kernel_prog* h_prog;
  // block inverses of the last factorisation
  void* invd;
  size_t invd_bytes;
  // padded workspace for g3_potrf_robust / g3_trsm on ragged sizes
  void* work;
  size_t work_bytes;
  // optional profiling: HIP-event pairs around tagged regions (g3_prof_*)
  bool prof_on;
  int prof_level;
  unsigned prof_skip;      // sampling counter of level 3
  hipEvent_t* prof_ev;
  int prof_cap, prof_n;          // events allocated / used
  struct { int e0, e1, tag; double work; }* prof_rec;
  int prof_nrec;
  char err[512];
};

// profiling tags
enum { G3_TAG_GEMM_BIG = 0, G3_TAG_GRAM = 1, G3_TAG_POTRF = 2, G3_TAG_TRSV = 3, G3_TAG_CROSS_GRAM = 4,
       G3_TAG_TRSM = 5, G3_TAG_REDUCE = 6, G3_TAG_GEMM_MID = 7, G3_TAG_GEMM_SMALL = 8, G3_TAG_LEAF = 9,
       G3_NTAGS = 10 };
int g3i_prof_begin(g3_ctx* ctx, int tag, double work);   // returns record index or -1
void g3i_prof_end(g3_ctx* ctx, int rec);

#define G3_HIP(call)                                                                          \
  do {                                                                                        \
    hipError_t _e = (call);                                                                   \
    if (_e != hipSuccess) {                                                                   \
      snprintf(ctx->err, sizeof(ctx->err), "%s:%d %s -> %s", __FILE__, __LINE__, #call,       \
               hipGetErrorString(_e));                                                        \
      return G3_ERR_HIP;                                                                      \
    }                                                                                         \
  } while (0)

#define G3_LAUNCH_CHECK()                                                                     \
  do {                                                                                        \
    hipError_t _e = hipGetLastError();                                                        \
    if (_e != hipSuccess) {                                                                   \
      snprintf(ctx->err, sizeof(ctx->err), "%s:%d launch -> %s", __FILE__, __LINE__,          \
               hipGetErrorString(_e));                                                        \
      return G3_ERR_HIP;                                                                      \
    }                                                                                         \
  } while (0)

// Every extern "C" entry runs with the context's device current and restores the caller's device
// on return, so contexts on different GPUs can be used from one process (one thread per context).
struct g3_dev_guard {
  int prev = -1;
  bool switched = false;
  explicit g3_dev_guard(const g3_ctx* ctx) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != ctx->device) switched = (hipSetDevice(ctx->device) == hipSuccess);
  }
  ~g3_dev_guard() {
    if (switched && prev >= 0) (void)hipSetDevice(prev);
  }
  g3_dev_guard(const g3_dev_guard&) = delete;
  g3_dev_guard& operator=(const g3_dev_guard&) = delete;
};
#define G3_MAX_DEVICES 64   // per-device caches of function attributes

static inline int g3_nbatch(const g3_ctx* ctx) { return ctx->batch > 1 ? ctx->batch : 1; }
// element stride between batch members for an operand at p (0 outside batch mode)
static inline int64_t g3_bstride_of(const g3_ctx* ctx, const void* p) {
  if (ctx->batch <= 1) return 0;
  const char* c = (const char*)p;
  return (ctx->bw_base && c >= ctx->bw_base && c < ctx->bw_base + ctx->bw_bytes) ? ctx->bstride_w : ctx->bstride;
}

// Batch mode for the launches issued while the object lives: members `stride` elements apart, operands inside
// [w_base, +w_bytes) `stride_w` apart.  Every way out of the scope leaves the context in single-member mode.
struct g3_batch_scope {
  g3_ctx* ctx;
  g3_batch_scope(g3_ctx* c, int batch, int64_t stride, int64_t stride_w, const void* w_base, size_t w_bytes) : ctx(c) {
    ctx->batch = batch;
    ctx->bstride = stride;
    ctx->bstride_w = stride_w;
    ctx->bw_base = (const char*)w_base;
    ctx->bw_bytes = w_bytes;
  }
  ~g3_batch_scope() {
    ctx->batch = 0;
    ctx->bw_base = nullptr;
  }
  g3_batch_scope(const g3_batch_scope&) = delete;
  g3_batch_scope& operator=(const g3_batch_scope&) = delete;
};

// launches issued now go to the low-priority bulk stream of the look-ahead sweep
static inline bool g3_on_bulk_stream(const g3_ctx* ctx) { return ctx->stream == ctx->side_stream; }

// ---- scaffold of the two-stream sweeps (potrf_lookahead and trsm_lookahead in g3_potrf.hip, g3i_potri in g3_grad.hip)
// The context's event pool holds at least `need` events.  Growing it destroys the events it held, so it is refused while a
// sweep is active: the sweep's event pointers would dangle.
int g3i_ensure_events(g3_ctx* ctx, int need);

// Launches issued while the object lives go to stream `s` (a sweep's bulk stream).  Every way out of the scope, the early
// return of G3_HIP included, puts the context back on the stream it was on.
struct g3_stream_scope {
  g3_ctx* ctx;
  hipStream_t prev;
  g3_stream_scope(g3_ctx* c, hipStream_t s) : ctx(c), prev(c->stream) { ctx->stream = s; }
  ~g3_stream_scope() { ctx->stream = prev; }
  g3_stream_scope(const g3_stream_scope&) = delete;
  g3_stream_scope& operator=(const g3_stream_scope&) = delete;
};

// A sweep with its chain on the context's stream and its bulk updates on `bulk`.  While the object lives the context is
// marked as inside a sweep: g3i_trsm_rlt then stays on one stream and the event pool cannot be regrown.  The constructor is
// the opening fork (bulk waits, through `ev`, for everything already queued on the chain's stream: Gram, memsets); check
// `rc` behind it.  join() is the closing one: the chain continues only after bulk has drained.  An error path needs no
// join, the caller abandons the sweep.  bulk == the chain's stream is the one-stream mode of a small g3i_potri: no sweep
// is marked, fork and join do nothing.
struct g3_sweep_scope {
  g3_ctx* ctx;
  hipStream_t chain, bulk;
  hipEvent_t ev;
  int rc;
  g3_sweep_scope(g3_ctx* c, hipStream_t bulk_, hipEvent_t ev_) : ctx(c), chain(c->stream), bulk(bulk_), ev(ev_) {
    if (bulk != chain) ctx->in_sweep = true;
    rc = wait(bulk, chain);
  }
  ~g3_sweep_scope() {
    if (bulk != chain) ctx->in_sweep = false;
  }
  int join() { return wait(chain, bulk); }
  g3_sweep_scope(const g3_sweep_scope&) = delete;
  g3_sweep_scope& operator=(const g3_sweep_scope&) = delete;

 private:
  int wait(hipStream_t waiter, hipStream_t on) {   // `waiter` goes on only after what is queued on `on` now
    if (bulk == chain) return G3_OK;
    G3_HIP(hipEventRecord(ev, on));
    G3_HIP(hipStreamWaitEvent(waiter, ev, 0));
    return G3_OK;
  }
};

static inline size_t g3_esize(g3_dtype dt) { return dt == G3_F64 ? 8 : 4; }
static inline int64_t g3_roundup(int64_t n, int64_t m) { return (n + m - 1) / m * m; }

// The library's one way from a g3_dtype to a type: f(T()) with T = double for G3_F64, float otherwise; returns what f returns.
//   return g3_by_dtype(dt, [&](auto t) { using T = decltype(t); return launch_t<T>(...); });
template <typename F>
static inline auto g3_by_dtype(g3_dtype dt, F&& f) {
  if (dt == G3_F64) return f(double());
  return f(float());
}

// a context on the caller's stream that creates no stream of its own; the low-priority side stream on first need
int g3i_ctx_create_on(int device, hipStream_t stream, g3_ctx** out);
int g3i_ensure_side_stream(g3_ctx* ctx);
void g3i_ctx_forget_stream(g3_ctx* ctx, hipStream_t s);     // s (synchronised) is about to be destroyed by its owner
// latency (us) of a one-wave kernel submitted on `a` while a dispatch-bound launch (its duration in *long_us) runs on `b`
bool g3i_probe_pair(hipStream_t a, hipStream_t b, unsigned* scratch, double* tiny_us, double* long_us, int reps);

// internal launchers (stream-ordered, no host sync)
int g3i_gemm_nt(g3_ctx* ctx, void* C, int64_t ldc, const void* A, int64_t lda, const void* B,
                int64_t ldb, int64_t m, int64_t n, int64_t k, double alpha, double beta,
                g3_dtype dt, int lower_only);
// wide = 1: force a tile that spans 128 output columns (C may then alias A when n == 128)
int g3i_gemm_nt_ex(g3_ctx* ctx, void* C, int64_t ldc, const void* A, int64_t lda, const void* B,
                   int64_t ldb, int64_t m, int64_t n, int64_t k, double alpha, double beta,
                   g3_dtype dt, int lower_only, int wide);
// C = alpha A V^T + beta C, V (n x n) lower triangular: column tile n0 reduces over K = n0 + BN only (C must not alias A)
int g3i_gemm_nt_ktri(g3_ctx* ctx, void* C, int64_t ldc, const void* A, int64_t lda, const void* V, int64_t ldv, int64_t m, int64_t n,
                     double alpha, double beta, g3_dtype dt);
// only elements with col <= row + diag_off (trapezoid; 0 = lower triangle of a diagonal-anchored C)
int g3i_gemm_nt_trap(g3_ctx* ctx, void* C, int64_t ldc, const void* A, int64_t lda, const void* B,
                     int64_t ldb, int64_t m, int64_t n, int64_t k, double alpha, double beta,
                     g3_dtype dt, int64_t diag_off);
// staircase: stacked row segments, segment s updates its first seg_cols[s] columns (one launch)
int g3i_gemm_nt_stair(g3_ctx* ctx, void* C, int64_t ldc, const void* A, int64_t lda, const void* B,
                      int64_t ldb, int64_t k, const int64_t* seg_rows, const int64_t* seg_cols, int nseg,
                      double alpha, double beta, g3_dtype dt, int64_t b_nb, const int32_t* b_perm, int nperm,
                      const int64_t* seg_diag = nullptr);
// one-launch stripe-local solve X <- X L^-T (n <= 1024); 1 = shape not covered, 0 = done
int g3i_trsm_stripe(g3_ctx* ctx, const void* L, int64_t n, int64_t ldl, void* X, int64_t m, int64_t ldx, const void* W,
                    g3_dtype dt);
int g3i_potrf(g3_ctx* ctx, void* A, int64_t n, int64_t ld, g3_dtype dt, void* invd);
int g3i_potrf_tall(g3_ctx* ctx, void* A, int64_t n, int64_t ld, g3_dtype dt, void* invd, int64_t E);
int g3i_trsm_rlt(g3_ctx* ctx, const void* L, int64_t n, int64_t ldl, void* B, int64_t m,
                 int64_t ldb, g3_dtype dt, const void* invd);
int g3i_trtri_blocks(g3_ctx* ctx, const void* L, int64_t n, int64_t ldl, g3_dtype dt, void* invd);
// V = L^-1 (n x n lower, n = 128 * 2^q <= 2048) from the 128-block inverses W; Vt and U are n x n scratch (Vt = V^T on return
// except for the last level); all compact (leading dimension n)
int g3i_trtri_full(g3_ctx* ctx, const void* L, int64_t n, const void* W, void* V, void* Vt, void* U, g3_dtype dt);
int g3i_reset_info(g3_ctx* ctx);
// the pivot flag of the factorisation queued last, read on the host (synchronises the context's stream)
int g3i_read_info(g3_ctx* ctx, int* info_host);
bool g3i_info_known_zero(const g3_ctx* ctx);
// g3_diag_stats / g3_logp_terms / g3_rows_dot_ss results left in device memory (no host synchronisation): 3 / 4 doubles
int g3i_diag_stats_dev(g3_ctx* ctx, const void* A, int64_t n, int64_t ld, g3_dtype dt, double* out_dev);
// (logp_terms for `batch` members: factors lstride, vectors a astride elements apart, four doubles each)
int g3i_logp_terms_dev(g3_ctx* ctx, const void* L, int64_t n, int64_t ld, const void* a, g3_dtype dt, double* out_dev, int batch = 1,
                       int64_t lstride = 0, int64_t astride = 0);
// batch members of at most 256 padded rows: factor + block inverses + a = L^-1 delta + the four logp scalars, one
// workgroup per member, one launch (g3_potrf.hip)
int g3i_small_factor_batched(g3_ctx* ctx, void* K, int64_t ld, int64_t kstride, void* W, int64_t wstride, const void* delta, int64_t ldd,
                             void* a, int64_t astride, double* dstats, int batch, int64_t n, int64_t np, g3_dtype dt);
// batch members of 384 ... 1024 padded rows: a group of workgroups per member factors it (and solves its right-hand-side rows)
// in ONE launch for the whole batch (g3_chainb.hip); ctl: g3i_coop_ctl_bytes(batch) of device scratch
size_t g3i_coop_ctl_bytes(int batch);
int g3i_coop_group(const g3_ctx* ctx, int batch, int64_t np);
int g3i_coop_factor_batched(g3_ctx* ctx, void* K, int64_t ld, int64_t kstride, void* W, int64_t wstride, unsigned* ctl, int batch,
                            int64_t np, g3_dtype dt);
int g3i_diag_add(g3_ctx* ctx, void* A, int64_t n, int64_t ld, g3_dtype dt, double value);
// A[0:rows, 0:cols) *= factor (stream-ordered)
int g3i_scale(g3_ctx* ctx, void* A, int64_t rows, int64_t cols, int64_t ld, g3_dtype dt, double factor);
int g3i_gram_grad(g3_ctx* ctx, const g3_kernel_prog* prog, const g3_grad_map* map, const void* X, int64_t N, int64_t ldx,
                  int d, g3_dtype dt, const void* G, int64_t ldg, const void* alpha, double* out_host,
                  int64_t row0 = 0, int64_t nrows = -1);
// generated gradient kernel (g3_gram_jit.hip); at most this many register accumulators per thread
#define G3_GRAD_JIT_MAXSLOTS 40
hipFunction_t g3i_grad_jit_function(g3_ctx* ctx, const g3_kernel_prog* prog_host, int d, g3_dtype dt, int* nslots);
int g3i_gram_grad_batched(g3_ctx* ctx, const g3_kernel_prog* progs, int batch, const g3_grad_map* map, const void* X, int64_t N,
                          int64_t ldx, int d, g3_dtype dt, const void* G, int64_t ldg, int64_t gstride, const void* alpha,
                          int64_t astride, double* out_host, int64_t row0 = 0, int64_t nrows = -1);
// g3i_gram_grad_batched may use the head of the context's workspace (g3_grad.hip::gram_grad_head) for `batch` members: what a
// caller keeps there across that call starts behind it.  The workspace grown to head + bytes, *behind = where those start
int g3i_reserve_behind_grad(g3_ctx* ctx, int batch, size_t bytes, char** behind);
// grid of a pass over the lower triangle (n >= 1) by workgroups of 256 columns, rows dealt over grid.y: enough to fill the chip
static inline dim3 g3_tril_rows_grid(int64_t n, unsigned members = 1) {
  const int64_t gx = (n + 255) / 256, gy = 16384 / gx;
  return dim3((unsigned)gx, (unsigned)(gy < 1 ? 1 : (gy > n ? n : gy)), members);
}
int g3i_rows_dot_ss_batched(g3_ctx* ctx, const void* V, int64_t m, int64_t n, int64_t ld, const void* a, g3_dtype dt, void* dot,
                            void* ss, int batch, int64_t vstride, int64_t astride, int64_t ostride);
// rows_dot_ss over the upper triangle of a square Y (npad x npad): rows [0, n) from their diagonal on, rows [n, npad) get 0
int g3i_rows_dot_ss_tri(g3_ctx* ctx, const void* Y, int64_t n, int64_t npad, int64_t ld, const void* a, g3_dtype dt, void* dot,
                        void* ss);
// ---- pieces of g3_gp_factor that g3_gp_append (g3_append.hip) shares (g3_api.hip)
// the right-hand-side block of a resumed factorisation: row 0 = [a[0:n0), delta[n0:n), 0 ...] over npad columns, rows 1 .. rows-1 zero
int g3i_append_rhs(g3_ctx* ctx, void* dst, int64_t ld, const void* a, const void* delta, int64_t n0, int64_t n, int64_t npad,
                   int64_t rows, g3_dtype dt);
// the finishing reduction of an evaluation: a[a_from:Np) <- the solved row `rhs`, st5 = [sum log L_ii, a^T a, #non-finite a, #bad
// diagonal entries] over the first N rows and the pivot flag, which is left cleared.  Synchronises the context's stream
int g3i_logp_finish(g3_ctx* ctx, const void* K, int64_t N, int64_t Np, int64_t ldk, const void* rhs, void* a, int64_t a_from, g3_dtype dt,
                    double st5[5]);
// [min, mean, max] of a device vector of n entries, on the host (synchronises the context's stream)
int g3i_vec_stats(g3_ctx* ctx, const void* v, int64_t n, g3_dtype dt, double out[3]);
int g3i_ensure_invd(g3_ctx* ctx, int64_t n, g3_dtype dt);
int g3i_ensure_work(g3_ctx* ctx, size_t bytes);
int g3i_upload_prog(g3_ctx* ctx, const g3_kernel_prog* prog, int slot, const g3_kernel_prog** dptr);
int g3i_gram_batched(g3_ctx* ctx, const g3_kernel_prog* dprogs, const g3_kernel_prog* first_host, int batch,
                     const void* X, int64_t n, int64_t ldx, int d, g3_dtype dt, void* K, int64_t ldk,
                     int64_t kstride, int64_t npad, unsigned flags);
// the same launch for the rectangular cross block K_b(X1, X2) (sym = 0) or the square covariance (sym = 1, X2 = X1)
int g3i_gram_rect_batched(g3_ctx* ctx, const g3_kernel_prog* dprogs, const g3_kernel_prog* first_host, int batch, const void* X1,
                          int64_t n1, int64_t ldx1, const void* X2, int64_t n2, int64_t ldx2, int d, g3_dtype dt, void* K,
                          int64_t ldk, int64_t kstride, int64_t n1pad, int64_t n2pad, unsigned flags, int sym);
// diag(K_b(X)) per member (device programs) into out + b * ostride
int g3i_gram_diag_batched(g3_ctx* ctx, const g3_kernel_prog* dprogs, int batch, const void* X, int64_t n, int64_t ldx, int d,
                          g3_dtype dt, void* out, int64_t ostride);
// batched posterior cross solve (g3_crossb.hip): Ks = batch x Mp x Np cross-Gram blocks (consumed), mu / ss batch x ostride
int g3i_cross_solve_batched(g3_ctx* ctx, void* Ks, int64_t sstride, const void* L, int64_t ldl, int64_t lstride, const void* W,
                            int64_t wstride, const void* a, int64_t astride, void* mu, void* ss, int64_t ostride, int64_t Mp,
                            int64_t N, int64_t Np, int batch, g3_dtype dt, int keepv = 0);
// CholeskyRobust for `batch` matrices of n <= 256 rows with the jitter schedule on the device (g3_drawsb.hip): one launch, no
// host round trip; wscr = g3i_robust_scratch_bytes of device memory, res_dev = batch x [tries, fallback, jitter] doubles
size_t g3i_robust_scratch_bytes(int batch, int64_t n, g3_dtype dt);
int g3i_potrf_robust_batched(g3_ctx* ctx, const void* K, int64_t ldk, int64_t kstride, void* L, int64_t ldl, int64_t lstride, int batch,
                             int64_t n, g3_dtype dt, int maxtries, void* wscr, double* res_dev);
// out[b] = loc[b] (+ mu[b]) + Lp_b Z[b]: Lp factors lstride apart, loc batch x M, mu batch x mustride or null, Z / out batch x M x S
int g3i_draws_batched(g3_ctx* ctx, const void* Lp, int64_t ldl, int64_t lstride, const void* loc, const void* mu, int64_t mustride,
                      const void* Z, void* out, int64_t M, int64_t S, int batch, g3_dtype dt);
// the Gram kernel generated for prog's structure (g3_gram_jit.hip); 0 = launched, 1 = none (the caller interprets)
int g3i_gram_jit(g3_ctx* ctx, const g3_kernel_prog* prog_host, const g3_kernel_prog* prog_dev, int batch, const void* X1, int64_t n1,
                 int64_t ldx1, const void* X2, int64_t n2, int64_t ldx2, int d, g3_dtype dt, void* K, int64_t ldk, int64_t n1pad,
                 int64_t n2pad, unsigned flags, int sym, int64_t kstride, int64_t diag_off, dim3 grid);
// C == nullptr: Y = L^-T alone, the K^-1 product is not run
int g3i_potri(g3_ctx* ctx, const void* L, int64_t n, int64_t ldl, const void* invd, g3_dtype dt, void* Y,
              int64_t ldy, void* C, int64_t ldc);
// that sweep for the `batch` members of one factorisation (g3_gp_grad.hip; batch > 1: batch mode, members kstride apart), every
// member's pivot flag cleared, recorded as one profiler region `tag` of `flops`
int g3i_kinv_sweep(g3_ctx* ctx, int batch, const void* L, int64_t np, int64_t ldl, int64_t kstride, const void* invd, g3_dtype dt,
                   void* Y, int64_t ldy, void* Kinv, int64_t ldc, int tag, double flops);
// that sweep with Kinv = Y Y^T, then alpha_b = Y_b a_b in one launch (vectors roundup(N,128) apart; one member: kstride 0)
int g3i_kinv_alpha(g3_ctx* ctx, int batch, const void* L, int64_t N, int64_t ldl, int64_t kstride, const void* invd, const void* a,
                   g3_dtype dt, void* Y, int64_t ldy, void* Kinv, int64_t ldc, void* alpha, int tag);
// What g3_gp_factor_batched queues behind its Gram launch, for `batch` prepared members in its layout (K: (Np + 128) x ldk each,
// kstride apart, identity-padded from N on; block inverses Np * 128 apart, a batch x Np, dstats four doubles per member): factor,
// a_b = L_b^-1 delta_b, the four scalars of g3_logp_terms.  Np <= 256: g3i_small_factor_batched, which reads the right-hand sides
// from delta (ldd apart); larger: the right-hand-side block of every member must hold [delta_b; 0], and the members go through the
// cooperative kernel (coop_ctl: its control words; null: never) or one lock-step sweep -- a batch of one is the single-matrix
// sweep.  The members' pivot flags are copied to flags_host (valid once the stream is synchronised) and, when flags_dev is
// given, there as well; the context's flags are left cleared.  No host synchronisation.
int g3i_factor_members(g3_ctx* ctx, int batch, int64_t N, int64_t Np, const void* delta, int64_t ldd, g3_dtype dt, void* K, int64_t ldk,
                       int64_t kstride, void* invd, void* a, double* dstats, unsigned* coop_ctl, int* flags_host, int* flags_dev);

// ---- the members of a chain (MemberProgs, g3_host.h) as the batched entry points use them
// Every member must be a valid program of ONE structure (whole programs), or the template and member 0 valid (template form:
// the fields' offsets cannot touch structure).  0 and *first = member 0, the structure all share; 1 = refuse (status -2).
static inline int g3i_validate_members(const MemberProgs& mp, int batch, int d, g3_kernel_prog* first) {
  mp.member(0, first);
  if (!mp.progs) return g3h_validate_prog(mp.tmpl, d) || g3h_validate_prog(first, d);
  for (int b = 0; b < batch; ++b)
    if (g3h_validate_prog(&mp.progs[b], d) || !g3h_same_structure(&mp.progs[0], &mp.progs[b])) return 1;
  return 0;
}

// Device copies of the members' programs in ctx->bbuf (laid out by g3h_member_layout): whole programs in one copy, or the
// template and the batch x nfield doubles that differ, expanded on the device -- a chain row costs nfield doubles of PCIe,
// not a 6 KB program.  Queued on ctx->stream without a wait: the host arrays must stay until the caller has synchronised.
struct g3_dev_members {
  g3_kernel_prog* progs;
  double* stats;   // stat_bytes behind the programs
  void* tail;      // tail_bytes, 256-byte aligned
};
int g3i_upload_members(g3_ctx* ctx, const MemberProgs& mp, int batch, size_t stat_bytes, size_t tail_bytes, g3_dev_members* out);

// The *_batched_fields entry points: the template form's own argument checks, then `call(members)` -- the implementation the
// whole-programs entry point shares, whose checks number their arguments as that entry point does (g3h_fields_status maps
// the codes lo .. -4).  check_batch: batch is refused here, before the fields (g3_gp_factor_batched_fields leaves it to the
// shared checks, after them).
template <typename F>
static inline int g3i_fields_call(const g3_kernel_prog* tmpl, int batch, bool check_batch, const double* fields,
                                  const int32_t* offsets, int nfield, int lo, F&& call) {
  if (!tmpl) return -2;
  if (check_batch && (batch < 1 || batch > G3_MAX_BATCH)) return -3;
  if (nfield < 0 || nfield > G3_MAX_FIELDS) return -6;
  if (nfield && (!fields || !offsets)) return -4;
  for (int i = 0; i < nfield; ++i)
    if (!g3h_field_offset_ok_tmpl(tmpl, offsets[i])) return -5;
  MemberProgs mp;
  mp.tmpl = tmpl;
  mp.fields = fields;
  mp.offs = offsets;
  mp.nfield = nfield;
  return g3h_fields_status(call(mp), lo);
}
