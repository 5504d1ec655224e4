// Context, device memory, element-wise / reduction kernels and the fused hot-path entry
// points of libg3hip (see include/g3hip.h for the contract of each function).
#include "g3_internal.h"
#include "g3_host.h"
#include <stdlib.h>

// ----------------------------------------------------------------------------- context
extern "C" int g3_version(void) { return 106; }

static int ctx_create_impl(int device, hipStream_t on_stream, g3_ctx** out);
extern "C" int g3_ctx_create(int device, g3_ctx** out) { return ctx_create_impl(device, nullptr, out); }
// A context that works on the caller's stream and creates NO stream of its own (the side stream of a two-stream sweep is
// created the first time one is needed, g3i_ensure_side_stream).  The multi-GPU driver's look-ahead and bulk contexts are
// made this way: HIP maps streams onto a few hardware queues per priority, and every idle stream a process holds shifts
// which of the streams that matter end up sharing one.
int g3i_ctx_create_on(int device, hipStream_t stream, g3_ctx** out) { return stream ? ctx_create_impl(device, stream, out) : -3; }
// ---- stream placement probe (shared with the multi-GPU driver, g3_dist.hip::pick_streams).  Two HIP streams whose hardware
// queues sit on the same compute pipe disturb each other: while the pipe dispatches a CU-filling launch of one, every small
// kernel of the other waits ~100 us instead of ~35 (and most of the launch when they share the QUEUE).  HIP decides the
// placement from the process's stream history and offers no way to ask, so it is measured.
#include <time.h>
__global__ void probe_long_kernel(int iters) {
  for (int i = 0; i < iters; ++i) __builtin_amdgcn_s_sleep(127);
}
__global__ void probe_tiny_kernel(unsigned* out) {
  if (threadIdx.x == 0 && out) *out = 1u;
}
static double probe_now_us() {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec * 1e6 + (double)ts.tv_nsec * 1e-3;
}
// latency (us) of a one-wave kernel submitted on `a` while the dispatch-bound kernel runs on `b`, and that kernel's duration
bool g3i_probe_pair(hipStream_t a, hipStream_t b, unsigned* scratch, double* tiny_us, double* long_us, int reps) {
  double best = 1e30, lbest = 1e30;
  for (int rep = 0; rep < reps; ++rep) {
    if (hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess) return false;
    const double t0 = probe_now_us();
    hipLaunchKernelGGL(probe_long_kernel, dim3(32768), dim3(256), 0, b, 12);
    // let the long kernel get going, then submit the small one and wait for it
    while (probe_now_us() - t0 < 100.0) {}
    const double t1 = probe_now_us();
    hipLaunchKernelGGL(probe_tiny_kernel, dim3(1), dim3(64), 0, a, scratch);
    if (hipStreamSynchronize(a) != hipSuccess) return false;
    const double t2 = probe_now_us();
    if (hipStreamSynchronize(b) != hipSuccess) return false;
    const double t3 = probe_now_us();
    if (t2 - t1 < best) best = t2 - t1;
    if (t3 - t0 < lbest) lbest = t3 - t0;
  }
  *tiny_us = best;
  *long_us = lbest;
  return hipGetLastError() == hipSuccess;
}


// The low-priority side stream of the two-stream sweeps: (re)chosen, by the probe above, the first time a sweep needs it with
// the stream the context currently works on -- four low-priority candidates (the context's own side stream among them), the
// first whose queue does not share a pipe with the chain's stream wins.  ~7 ms once per (context, stream); G3_PROBE=0 keeps
// whatever the runtime dealt.
int g3i_ensure_side_stream(g3_ctx* ctx) {
  if (ctx->side_stream && (ctx->side_for == ctx->stream || !ctx->tune.probe)) return G3_OK;
  int lo = 0, hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
  if (!ctx->side_stream) G3_HIP(hipStreamCreateWithPriority(&ctx->side_stream, hipStreamNonBlocking, lo));
  ctx->side_for = ctx->stream;
  if (!ctx->tune.probe) return G3_OK;
  const int NL = 4;
  hipStream_t L[NL] = {ctx->side_stream, nullptr, nullptr, nullptr};
  for (int i = 1; i < NL; ++i)
    if (hipStreamCreateWithPriority(&L[i], hipStreamNonBlocking, lo) != hipSuccess) L[i] = nullptr;
  double t[NL], base = 1e30, tl = 0;
  bool ok = true;
  unsigned* scratch = (unsigned*)(ctx->d_stats + 63);   // (the last word of the reduction scratch: no reduction uses it)
  for (int i = 0; i < NL && ok; ++i) {
    t[i] = 1e30;
    if (!L[i]) continue;
    ok = g3i_probe_pair(ctx->stream, L[i], scratch, &t[i], &tl, 2);
    if (t[i] < base) base = t[i];
  }
  int pick = 0;
  if (ok) {
    const double limit = base * 2.0 > base + 40.0 ? base * 2.0 : base + 40.0;
    for (int i = 0; i < NL; ++i)
      if (L[i] && t[i] <= limit) { pick = i; break; }
    if (ctx->tune.probe > 1)
      fprintf(stderr, "libg3hip placement: side stream candidates %.0f %.0f %.0f %.0f us beside the chain's stream -> %d\n", t[0], t[1], t[2], t[3], pick);
  }
  for (int i = 0; i < NL; ++i)
    if (L[i] && i != pick) (void)hipStreamDestroy(L[i]);
  ctx->side_stream = L[pick];
  return G3_OK;
}

// The event pool of the two-stream sweeps.  la_nev counts the events that exist, whichever way out is taken:
// g3_ctx_destroy walks them.
int g3i_ensure_events(g3_ctx* ctx, int need) {
  if (ctx->la_nev >= need) return G3_OK;
  if (ctx->in_sweep) {
    snprintf(ctx->err, sizeof(ctx->err), "the event pool cannot grow (%d -> %d) inside a two-stream sweep", ctx->la_nev, need);
    return G3_ERR_HIP;
  }
  for (; ctx->la_nev > 0; --ctx->la_nev) (void)hipEventDestroy(ctx->la_ev[ctx->la_nev - 1]);
  free(ctx->la_ev);
  ctx->la_ev = (hipEvent_t*)calloc((size_t)need, sizeof(hipEvent_t));
  if (!ctx->la_ev) return G3_ERR_NOMEM;
  for (; ctx->la_nev < need; ++ctx->la_nev) G3_HIP(hipEventCreateWithFlags(&ctx->la_ev[ctx->la_nev], hipEventDisableTiming));
  return G3_OK;
}

static int ctx_create_impl(int device, hipStream_t on_stream, g3_ctx** out) {
  if (!out) return -2;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return G3_ERR_HIP;
  if (device < 0 || device >= ndev) return -1;
  g3_ctx* ctx = new (std::nothrow) g3_ctx();
  if (!ctx) return G3_ERR_NOMEM;
  memset(ctx, 0, sizeof(*ctx));
  ctx->device = device;
  int prev_dev = -1;                       // like every other entry: the caller's current device is restored
  if (hipGetDevice(&prev_dev) != hipSuccess) prev_dev = -1;
  hipError_t e = hipSetDevice(device);
  int lo = 0, hi = 0;
  if (e == hipSuccess) (void)hipDeviceGetStreamPriorityRange(&lo, &hi);   // lo = least priority, hi = greatest
  // the chain runs on the context's stream at the greatest priority, the bulk updates on the side stream at the least:
  // measured, a bulk stream WITHOUT the low priority costs 2 % (N = 8192) to 10 % (N = 32768) of the step
  if (!on_stream) {
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&ctx->own_stream, hipStreamNonBlocking, hi);
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&ctx->side_stream, hipStreamNonBlocking, lo);
  }
  ctx->tune = g3h_tune_from_env();
  {
    const char* lg = getenv("G3_GEMM_LOG");
    ctx->gemm_log = (lg && *lg) ? fopen(lg, "a") : nullptr;
  }
  if (e == hipSuccess) e = hipMalloc((void**)&ctx->d_info, G3_MAX_BATCH * sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void**)&ctx->d_stats, 64 * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&ctx->d_prog, G3_PROG_SLOTS * sizeof(g3_kernel_prog));
  if (e == hipSuccess) e = hipHostMalloc((void**)&ctx->h_info, G3_MAX_BATCH * sizeof(int), hipHostMallocDefault);
  if (e == hipSuccess) e = hipHostMalloc((void**)&ctx->h_stats, 64 * sizeof(double), hipHostMallocDefault);
  if (e == hipSuccess) e = hipHostMalloc((void**)&ctx->h_prog, G3_PROG_SLOTS * sizeof(g3_kernel_prog), hipHostMallocDefault);
  for (int i = 0; i < G3_PROG_SLOTS && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&ctx->prog_ev[i], hipEventDisableTiming);
  ctx->prog_last = -1;
  if (e == hipSuccess) e = hipMemset(ctx->d_info, 0, G3_MAX_BATCH * sizeof(int));
  if (e != hipSuccess) {
    g3_ctx_destroy(ctx);
    if (prev_dev >= 0 && prev_dev != device) (void)hipSetDevice(prev_dev);
    return G3_ERR_HIP;
  }
  ctx->stream = on_stream ? on_stream : ctx->own_stream;
  ctx->adopted = on_stream != nullptr;
  *out = ctx;
  if (prev_dev >= 0 && prev_dev != device) (void)hipSetDevice(prev_dev);
  return G3_OK;
}

extern "C" int g3_ctx_destroy(g3_ctx* ctx) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->d_info) (void)hipFree(ctx->d_info);
  if (ctx->d_stats) (void)hipFree(ctx->d_stats);
  if (ctx->d_prog) (void)hipFree(ctx->d_prog);
  for (int i = 0; i < G3_PROG_SLOTS; ++i) if (ctx->prog_ev[i]) (void)hipEventDestroy(ctx->prog_ev[i]);
  if (ctx->h_info) (void)hipHostFree(ctx->h_info);
  if (ctx->h_stats) (void)hipHostFree(ctx->h_stats);
  if (ctx->h_prog) (void)hipHostFree(ctx->h_prog);
  if (ctx->invd) (void)hipFree(ctx->invd);
  if (ctx->work) (void)hipFree(ctx->work);
  if (ctx->bbuf) (void)hipFree(ctx->bbuf);
  if (ctx->prof_ev) {
    for (int i = 0; i < ctx->prof_cap; ++i) if (ctx->prof_ev[i]) (void)hipEventDestroy(ctx->prof_ev[i]);
    free(ctx->prof_ev);
  }
  if (ctx->prof_rec) free(ctx->prof_rec);
  if (ctx->la_ev) {
    for (int i = 0; i < ctx->la_nev; ++i) (void)hipEventDestroy(ctx->la_ev[i]);
    free(ctx->la_ev);
  }
  if (ctx->gemm_log) fclose(ctx->gemm_log);
  if (ctx->side_stream) (void)hipStreamDestroy(ctx->side_stream);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
  delete ctx;
  return G3_OK;
}

// A stream the context has worked on is about to be destroyed by its owner (the multi-GPU driver's chain stream): the caller
// has synchronised it; forget every reference -- the program ring records its events on the stream a slot was consumed on
void g3i_ctx_forget_stream(g3_ctx* ctx, hipStream_t s) {
  if (!ctx || !s) return;
  g3h_ring_forget(ctx->prog_busy, G3_PROG_SLOTS, &ctx->prog_last, ctx->prog_stream == s,
                  [&](int i) { return hipEventQuery(ctx->prog_ev[i]) == hipSuccess; });
  if (ctx->prog_stream == s) ctx->prog_stream = nullptr;
  if (ctx->info_stream == s) {
    ctx->info_clean = false;
    ctx->info_stream = nullptr;
  }
  if (ctx->side_for == s) ctx->side_for = nullptr;
}

extern "C" int g3_ctx_set_stream(g3_ctx* ctx, void* s) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  G3_HIP(hipStreamSynchronize(ctx->stream));
  // the old stream is drained: every slot of the program ring is free, and nothing may be recorded on (or
  // waited for from) a stream the caller is about to destroy
  for (int i = 0; i < G3_PROG_SLOTS; ++i) ctx->prog_busy[i] = false;
  ctx->prog_last = -1;
  ctx->prog_stream = nullptr;
  ctx->stream = s ? (hipStream_t)s : ctx->own_stream;
  ctx->adopted = (s != nullptr);
  return G3_OK;
}

// ----------------------------------------------------------------------------- profiling
extern "C" int g3_prof_enable(g3_ctx* ctx, int on) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (on && !ctx->prof_ev) {
    ctx->prof_cap = 16384;
    ctx->prof_ev = (hipEvent_t*)calloc(ctx->prof_cap, sizeof(hipEvent_t));
    ctx->prof_rec = (decltype(ctx->prof_rec))calloc(ctx->prof_cap / 2, sizeof(*ctx->prof_rec));
    if (!ctx->prof_ev || !ctx->prof_rec) return G3_ERR_NOMEM;
    for (int i = 0; i < ctx->prof_cap; ++i) G3_HIP(hipEventCreate(&ctx->prof_ev[i]));
  }
  ctx->prof_on = on != 0;
  ctx->prof_level = on;
  return G3_OK;
}
extern "C" int g3_prof_reset(g3_ctx* ctx) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  G3_HIP(hipStreamSynchronize(ctx->stream));
  ctx->prof_n = 0;
  ctx->prof_nrec = 0;
  return G3_OK;
}
int g3i_prof_begin(g3_ctx* ctx, int tag, double work) {
  if (!ctx->prof_on || ctx->prof_n + 2 > ctx->prof_cap) return -1;
  // level 1 (default): phases and the large GEMM launches only; level 2 adds every small launch
  const bool minor = tag == G3_TAG_GEMM_SMALL || tag == G3_TAG_LEAF || tag == G3_TAG_GEMM_MID;
  if (ctx->prof_level < 2 && minor) return -1;
  // level 3: like 2, but only every 16th of the small launches is timed (an unbiased sample that
  // keeps the event traffic out of launch-bound loops such as the multi-GPU driver's)
  if (ctx->prof_level == 3 && minor && (ctx->prof_skip++ & 15) != 0) return -1;
  const int r = ctx->prof_nrec++;
  ctx->prof_rec[r].e0 = ctx->prof_n++;
  ctx->prof_rec[r].e1 = ctx->prof_n++;
  ctx->prof_rec[r].tag = tag;
  ctx->prof_rec[r].work = work;
  (void)hipEventRecord(ctx->prof_ev[ctx->prof_rec[r].e0], ctx->stream);
  return r;
}
void g3i_prof_end(g3_ctx* ctx, int rec) {
  if (rec < 0) return;
  (void)hipEventRecord(ctx->prof_ev[ctx->prof_rec[rec].e1], ctx->stream);
}
extern "C" int g3_prof_collect(g3_ctx* ctx, double* out) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (!out) return -2;
  G3_HIP(hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < 3 * G3_PROF_NTAGS; ++i) out[i] = 0.0;
  for (int r = 0; r < ctx->prof_nrec; ++r) {
    float ms = 0.f;
    G3_HIP(hipEventElapsedTime(&ms, ctx->prof_ev[ctx->prof_rec[r].e0], ctx->prof_ev[ctx->prof_rec[r].e1]));
    const int t = ctx->prof_rec[r].tag;
    out[3 * t] += 1.0;
    out[3 * t + 1] += (double)ms;
    out[3 * t + 2] += ctx->prof_rec[r].work;
  }
  return G3_OK;
}

extern "C" int g3_ctx_sync(g3_ctx* ctx) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  G3_HIP(hipStreamSynchronize(ctx->stream));
  return G3_OK;
}

extern "C" const char* g3_last_error(g3_ctx* ctx) { return ctx ? ctx->err : "null context"; }

extern "C" int g3_malloc(g3_ctx* ctx, size_t bytes, void** dev) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (!dev) return -3;
  *dev = nullptr;
  if (bytes == 0) return G3_OK;
  G3_HIP(hipSetDevice(ctx->device));
  G3_HIP(hipMalloc(dev, bytes));
  return G3_OK;
}
extern "C" int g3_free(g3_ctx* ctx, void* dev) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (!dev) return G3_OK;
  G3_HIP(hipStreamSynchronize(ctx->stream));
  G3_HIP(hipFree(dev));
  return G3_OK;
}
extern "C" int g3_memcpy_h2d(g3_ctx* ctx, void* dev, const void* host, size_t bytes) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (bytes == 0) return G3_OK;
  if (!dev) return -2;
  if (!host) return -3;
  G3_HIP(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, ctx->stream));
  G3_HIP(hipStreamSynchronize(ctx->stream));  // host buffer is borrowed only for the call
  return G3_OK;
}
extern "C" int g3_memcpy_d2h(g3_ctx* ctx, void* host, const void* dev, size_t bytes) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (bytes == 0) return G3_OK;
  if (!host) return -2;
  if (!dev) return -3;
  G3_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
  G3_HIP(hipStreamSynchronize(ctx->stream));
  return G3_OK;
}
extern "C" int g3_memcpy_d2d(g3_ctx* ctx, void* dst, const void* src, size_t bytes) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (bytes == 0) return G3_OK;
  if (!dst) return -2;
  if (!src) return -3;
  G3_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  return G3_OK;
}
extern "C" int g3_memset(g3_ctx* ctx, void* dev, int byte, size_t bytes) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (bytes == 0) return G3_OK;
  if (!dev) return -2;
  G3_HIP(hipMemsetAsync(dev, byte, bytes, ctx->stream));
  return G3_OK;
}
// 16 bytes per thread, rows dealt over grid.y: the runtime's rectangular copy moves an 8 MB block at 0.5 TB/s
// (30 us, measured in the multi-GPU driver's trace), this one is bound by HBM
__global__ void __launch_bounds__(256) copy2d_kernel(char* __restrict__ dst, size_t dpitch, const char* __restrict__ src, size_t spitch,
                                                     size_t row_bytes, int64_t rows) {
  const size_t c = ((size_t)blockIdx.x * 256 + threadIdx.x) * 16;
  if (c >= row_bytes) return;
  for (int64_t r = blockIdx.y; r < rows; r += gridDim.y)
    *reinterpret_cast<uint4*>(dst + r * dpitch + c) = *reinterpret_cast<const uint4*>(src + r * spitch + c);
}

extern "C" int g3_copy2d(g3_ctx* ctx, void* dst, int64_t ldd, const void* src, int64_t lds,
                         int64_t rows, int64_t cols, g3_dtype dt) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (rows == 0 || cols == 0) return G3_OK;
  if (!dst) return -2;
  if (!src) return -4;
  if (rows < 0) return -6;
  if (cols < 0 || cols > ldd || cols > lds) return -7;
  const size_t es = g3_esize(dt);
  const size_t rb = (size_t)cols * es, dp = (size_t)ldd * es, sp = (size_t)lds * es;
  if (((rb | dp | sp | (uintptr_t)dst | (uintptr_t)src) & 15) == 0) {
    const unsigned gx = (unsigned)((rb / 16 + 255) / 256);
    int64_t gy = 8192 / gx;
    gy = gy < 1 ? 1 : (gy > rows ? rows : gy);
    hipLaunchKernelGGL(copy2d_kernel, dim3(gx, (unsigned)gy), dim3(256), 0, ctx->stream, (char*)dst, dp, (const char*)src, sp, rb, rows);
    G3_LAUNCH_CHECK();
    return G3_OK;
  }
  G3_HIP(hipMemcpy2DAsync(dst, dp, src, sp, rb, (size_t)rows, hipMemcpyDeviceToDevice, ctx->stream));
  return G3_OK;
}

// ----------------------------------------------------------------------------- small kernels
// one workgroup (1024 threads): out = [min, mean, max] of diag(A); optionally applies
// tt_to_cov's lift  A_ii += (1e-6f - min) when min <= 0  (tensors.py:95-98)
template <typename T>
__global__ void __launch_bounds__(1024)
diag_stats_kernel(T* A, int64_t n, int64_t ld, double* out, int lift, int64_t bstride) {
  A += (int64_t)blockIdx.x * bstride;            // batch member (grid.x)
  if (out) out += 3 * blockIdx.x;
  __shared__ double s_min[16], s_max[16], s_sum[16];
  __shared__ double s_m;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double mn = 1.0 / 0.0, mx = -1.0 / 0.0, sm = 0.0;
  bool first = true;
  for (int64_t i = tid; i < n; i += 1024) {
    const double v = (double)A[i * ld + i];
    if (first) { mn = v; mx = v; first = false; }
    else { mn = (v < mn || v != v) ? v : mn; mx = (v > mx || v != v) ? v : mx; }
    sm += v;
  }
  mn = wave_min(mn); mx = wave_max(mx); sm = wave_sum(sm);
  if (lane == 0) { s_min[wave] = mn; s_max[wave] = mx; s_sum[wave] = sm; }
  __syncthreads();
  if (tid == 0) {
    const double a = waves_min<16>(s_min), b = waves_max<16>(s_max), c = waves_sum<16>(s_sum);
    if (out) { out[0] = a; out[1] = c / (double)n; out[2] = b; }
    s_m = a;
  }
  __syncthreads();
  if (lift) {
    const T m = (T)s_m;
    if (!(m > T(0))) {
      const T add = (T)1e-6f - m;
      for (int64_t i = tid; i < n; i += 1024) A[i * ld + i] += add;
    }
  }
}

template <typename T>
__global__ void diag_add_kernel(T* A, int64_t n, int64_t ld, T v, int64_t bstride) {
  A += (int64_t)blockIdx.y * bstride;            // batch member (grid.y)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) A[i * ld + i] += v;
}

template <typename T>
__global__ void scrub_kernel(T* A, int64_t n2, int64_t ld) {
  const int64_t i = blockIdx.y;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n2; j += (int64_t)gridDim.x * blockDim.x) {
    T v = A[i * ld + j];
    if (v != v) A[i * ld + j] = T(0);
    else if (__builtin_isinf(v)) A[i * ld + j] = (T)1e10f;
  }
}

// out[0] = sum log L_ii ; out[1] = sum a_i^2 ; out[2] = #non-finite a ; out[3] = #bad diag
template <typename T>
__global__ void __launch_bounds__(1024)
logp_terms_kernel(const T* L, int64_t n, int64_t ld, const T* a, double* out, int64_t bstride, int64_t astride) {
  L += (int64_t)blockIdx.x * bstride;            // batch member (grid.x)
  if (a) a += (int64_t)blockIdx.x * astride;
  out += 4 * blockIdx.x;
  __shared__ double red[4][16];
  const int tid = threadIdx.x;
  LogpTerms t;
  for (int64_t i = tid; i < n; i += 1024) {
    t.diag((double)L[i * ld + i]);
    if (a) t.rhs((double)a[i]);
  }
  t.to_waves<16>(red, tid & 63, tid >> 6);
  if (tid == 0)
    for (int k = 0; k < 4; ++k) out[k] = waves_sum<16>(red[k]);
}

// The tail of one evaluation in ONE launch (small problems are bound by the number of launches, ~5 us each):
// a_dst <- a_src (the solved right-hand-side row, npad entries; from entry a_from on: an append leaves the entries of the
// rows it did not touch unwritten), the four scalars of logp_terms_kernel over its first n entries, and the pivot flag handed
// over and cleared: out[4] = *info, *info = 0.
template <typename T>
__global__ void __launch_bounds__(1024)
logp_finish_kernel(const T* L, int64_t n, int64_t npad, int64_t ld, const T* __restrict__ a_src, T* __restrict__ a_dst,
                   int64_t a_from, double* out, int* info) {
  __shared__ double red[4][16];
  const int tid = threadIdx.x;
  LogpTerms t;
  for (int64_t i = tid; i < npad; i += 1024) {
    const T av = a_src[i];
    if (i >= a_from) a_dst[i] = av;
    if (i < n) {
      t.diag((double)L[i * ld + i]);
      t.rhs((double)av);
    }
  }
  t.to_waves<16>(red, tid & 63, tid >> 6);
  if (tid == 0) {
    for (int k = 0; k < 4; ++k) out[k] = waves_sum<16>(red[k]);
    out[4] = (double)*info;
    *info = 0;
  }
}

// one workgroup (256 threads) per row of V: dot with a, and sum of squares
template <typename T>
__global__ void __launch_bounds__(256)
rows_dot_ss_kernel(const T* __restrict__ V, int64_t n, int64_t ld, const T* __restrict__ a,
                   T* __restrict__ dot, T* __restrict__ ss, int64_t vstride, int64_t astride, int64_t ostride, int64_t tri) {
  __shared__ double sd[4], sq[4];
  // grid.y = batch member: V, a and the outputs vstride / astride / ostride elements apart (0, 0, 0 for one problem)
  V += (int64_t)blockIdx.y * vstride;
  if (a) a += (int64_t)blockIdx.y * astride;
  if (dot) dot += (int64_t)blockIdx.y * ostride;
  if (ss) ss += (int64_t)blockIdx.y * ostride;
  // tri > 0: V is upper triangular and square, row i is read from column i on (nothing left of the diagonal is touched) and
  // the rows [n, tri) of the padding get zeros.  tri == 0: the whole row.  Either way thread t takes every 256th column from
  // the start of what is read, so the summation order of a row is fixed
  const int64_t i = blockIdx.x;
  if (tri > 0 && i >= n) {
    if (threadIdx.x == 0) {
      if (dot) dot[i] = T(0);
      if (ss) ss[i] = T(0);
    }
    return;
  }
  const T* v = V + i * ld;
  double d = 0, q = 0;
  for (int64_t j = (tri > 0 ? i : 0) + threadIdx.x; j < n; j += 256) {
    const double x = (double)v[j];
    if (a) d += x * (double)a[j];
    q += x * x;
  }
  d = wave_sum(d); q = wave_sum(q);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { sd[wave] = d; sq[wave] = q; }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (dot) dot[blockIdx.x] = (T)(sd[0] + sd[1] + sd[2] + sd[3]);
    if (ss) ss[blockIdx.x] = (T)(sq[0] + sq[1] + sq[2] + sq[3]);
  }
}

// cnt doubles of the context's reduction scratch, from `off` on, to the host (synchronises the context's stream)
static int fetch_stats(g3_ctx* ctx, double* out, int cnt, int off = 0) {
  G3_HIP(hipMemcpyAsync(ctx->h_stats + off, ctx->d_stats + off, cnt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  G3_HIP(hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < cnt; ++i) out[i] = ctx->h_stats[off + i];
  return G3_OK;
}

// one workgroup per member, members `stride` elements apart (one problem: 1 member, stride 0)
static int diag_stats_launch(g3_ctx* ctx, void* A, int64_t n, int64_t ld, g3_dtype dt, double* dout, int lift, int members = 1,
                             int64_t stride = 0) {
  g3_by_dtype(dt, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((diag_stats_kernel<T>), dim3(members), dim3(1024), 0, ctx->stream, (T*)A, n, ld, dout, lift, stride);
  });
  G3_LAUNCH_CHECK();
  return G3_OK;
}

extern "C" int g3_cov_lift(g3_ctx* ctx, void* K, int64_t n, int64_t ld, g3_dtype dt) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (!K) return -2;
  if (n < 0) return -3;
  if (ld < n) return -4;
  if (n == 0) return G3_OK;
  return diag_stats_launch(ctx, K, n, ld, dt, nullptr, 1);
}

extern "C" int g3_diag_stats(g3_ctx* ctx, const void* A, int64_t n, int64_t ld, g3_dtype dt, double out[3]) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (!A) return -2;
  if (n <= 0) return -3;
  if (ld < n) return -4;
  if (!out) return -6;
  int rc = diag_stats_launch(ctx, const_cast<void*>(A), n, ld, dt, ctx->d_stats + 8, 0);
  if (rc) return rc;
  return fetch_stats(ctx, out, 3, 8);
}

int g3i_diag_stats_dev(g3_ctx* ctx, const void* A, int64_t n, int64_t ld, g3_dtype dt, double* out_dev) {
  return diag_stats_launch(ctx, const_cast<void*>(A), n, ld, dt, out_dev, 0);
}

extern "C" int g3_diag_add(g3_ctx* ctx, void* A, int64_t n, int64_t ld, g3_dtype dt, double value) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (!A) return -2;
  if (n < 0) return -3;
  if (ld < n) return -4;
  if (n == 0) return G3_OK;
  return g3i_diag_add(ctx, A, n, ld, dt, value);
}

template <typename T>
__global__ void scale_kernel(T* A, int64_t rows, int64_t cols, int64_t ld, T f) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t i = blockIdx.y;
  if (j < cols && i < rows) A[i * ld + j] *= f;
}
int g3i_scale(g3_ctx* ctx, void* A, int64_t rows, int64_t cols, int64_t ld, g3_dtype dt, double factor) {
  if (rows <= 0 || cols <= 0) return G3_OK;
  const dim3 grid((unsigned)((cols + 255) / 256), (unsigned)rows);
  g3_by_dtype(dt, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((scale_kernel<T>), grid, dim3(256), 0, ctx->stream, (T*)A, rows, cols, ld, (T)factor);
  });
  G3_LAUNCH_CHECK();
  return G3_OK;
}

// stream-ordered; in batch mode every member gets the same increment
int g3i_diag_add(g3_ctx* ctx, void* A, int64_t n, int64_t ld, g3_dtype dt, double value) {
  const dim3 grid((unsigned)((n + 255) / 256), (unsigned)g3_nbatch(ctx));
  g3_by_dtype(dt, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((diag_add_kernel<T>), grid, dim3(256), 0, ctx->stream, (T*)A, n, ld, (T)value, g3_bstride_of(ctx, A));
  });
  G3_LAUNCH_CHECK();
  return G3_OK;
}

extern "C" int g3_scrub(g3_ctx* ctx, void* A, int64_t n1, int64_t n2, int64_t ld, g3_dtype dt) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (!A) return -2;
  if (n1 < 0) return -3;
  if (n2 < 0) return -4;
  if (ld < n2) return -5;
  if (n1 == 0 || n2 == 0) return G3_OK;
  const dim3 grid((unsigned)((n2 + 255) / 256 > 64 ? 64 : (n2 + 255) / 256), (unsigned)n1);
  g3_by_dtype(dt, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((scrub_kernel<T>), grid, dim3(256), 0, ctx->stream, (T*)A, n2, ld);
  });
  G3_LAUNCH_CHECK();
  return G3_OK;
}

// one workgroup per member: factors `lstride`, vectors a `astride` elements apart, four doubles each into out_dev
int g3i_logp_terms_dev(g3_ctx* ctx, const void* L, int64_t n, int64_t ld, const void* a, g3_dtype dt, double* out_dev, int batch,
                       int64_t lstride, int64_t astride) {
  g3_by_dtype(dt, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((logp_terms_kernel<T>), dim3(batch), dim3(1024), 0, ctx->stream, (const T*)L, n, ld, (const T*)a, out_dev,
                       lstride, astride);
  });
  G3_LAUNCH_CHECK();
  return G3_OK;
}

extern "C" int g3_logp_terms(g3_ctx* ctx, const void* L, int64_t n, int64_t ld, const void* a,
                             g3_dtype dt, double out[4]) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (!L) return -2;
  if (n <= 0) return -3;
  if (ld < n) return -4;
  if (!out) return -7;
  int rc = g3i_logp_terms_dev(ctx, L, n, ld, a, dt, ctx->d_stats);
  if (rc) return rc;
  return fetch_stats(ctx, out, 4);
}

// batch of SMALL problems (a chain of hyper-parameter vectors at N <= 1024): one workgroup per member walks its m rows, a
// wave per row -- m x batch workgroups of one row each cost more in dispatch than in arithmetic (0.58 ms for 4096 x 128 rows)
template <typename T>
__global__ void __launch_bounds__(256)
rows_dot_ss_member_kernel(const T* __restrict__ V, int64_t m, int64_t n, int64_t ld, const T* __restrict__ a,
                          T* __restrict__ dot, T* __restrict__ ss, int64_t vstride, int64_t astride, int64_t ostride) {
  V += (int64_t)blockIdx.x * vstride;
  if (a) a += (int64_t)blockIdx.x * astride;
  if (dot) dot += (int64_t)blockIdx.x * ostride;
  if (ss) ss += (int64_t)blockIdx.x * ostride;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t r = wave; r < m; r += 4) {
    const T* v = V + r * ld;
    double d = 0, q = 0;
    for (int64_t j = lane; j < n; j += 64) {
      const double x = (double)v[j];
      if (a) d += x * (double)a[j];
      q += x * x;
    }
    d = wave_sum(d); q = wave_sum(q);
    if (lane == 0) {
      if (dot) dot[r] = (T)d;
      if (ss) ss[r] = (T)q;
    }
  }
}

static int rows_dot_ss_launch(g3_ctx* ctx, const void* V, int64_t m, int64_t n, int64_t ld, const void* a,
                              g3_dtype dt, void* dot, void* ss, int batch = 1, int64_t vstride = 0, int64_t astride = 0,
                              int64_t ostride = 0, int64_t tri = 0) {
  if (m == 0) return G3_OK;
  g3_by_dtype(dt, [&](auto t) {
    using T = decltype(t);
    if (batch > 1 && m <= 1024 && tri == 0)
      hipLaunchKernelGGL((rows_dot_ss_member_kernel<T>), dim3((unsigned)batch), dim3(256), 0, ctx->stream, (const T*)V, m, n, ld,
                         (const T*)a, (T*)dot, (T*)ss, vstride, astride, ostride);
    else
      hipLaunchKernelGGL((rows_dot_ss_kernel<T>), dim3((unsigned)m, (unsigned)batch), dim3(256), 0, ctx->stream, (const T*)V, n, ld,
                         (const T*)a, (T*)dot, (T*)ss, vstride, astride, ostride, tri);
  });
  G3_LAUNCH_CHECK();
  return G3_OK;
}

int g3i_rows_dot_ss_batched(g3_ctx* ctx, const void* V, int64_t m, int64_t n, int64_t ld, const void* a, g3_dtype dt, void* dot,
                            void* ss, int batch, int64_t vstride, int64_t astride, int64_t ostride) {
  return rows_dot_ss_launch(ctx, V, m, n, ld, a, dt, dot, ss, batch, vstride, astride, ostride);
}

// the upper-triangular, square case (Y = L^-T of g3_gp_loo): rows [0, n) from their diagonal on, rows [n, npad) written as 0
int g3i_rows_dot_ss_tri(g3_ctx* ctx, const void* Y, int64_t n, int64_t npad, int64_t ld, const void* a, g3_dtype dt, void* dot,
                        void* ss) {
  return rows_dot_ss_launch(ctx, Y, npad, n, ld, a, dt, dot, ss, 1, 0, 0, 0, npad);
}

extern "C" int g3_rows_dot_ss(g3_ctx* ctx, const void* V, int64_t m, int64_t n, int64_t ld,
                              const void* a, g3_dtype dt, void* dot, void* ss) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (!V) return -2;
  if (m < 0) return -3;
  if (n < 0) return -4;
  if (ld < n) return -5;
  return rows_dot_ss_launch(ctx, V, m, n, ld, a, dt, dot, ss);
}

// ----------------------------------------------------------------------------- fused path
template <typename T>
__global__ void pad_row_kernel(T* dst, int64_t ld, const T* src, int64_t n, int64_t npad, int64_t rows,
                               int64_t dstride, int64_t sstride) {
  // dst is rows x npad (row stride ld): row 0 = [src, 0...], other rows 0; grid.y = batch member
  dst += (int64_t)blockIdx.y * dstride;
  src += (int64_t)blockIdx.y * sstride;
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= npad) return;
  for (int64_t r = 0; r < rows; ++r) dst[r * ld + j] = (r == 0 && j < n) ? src[j] : T(0);
}
// the right-hand-side block [src; 0] per member: blocks `dstride`, vectors src `sstride` elements apart
// The right-hand-side block of a resumed factorisation (g3_gp_append): rows x npad at dst, row 0 = [a[0:n0), delta[n0:n), 0 ...]
// -- what the sweep would have left in the first n0 columns, and the new entries it has yet to solve -- other rows 0.
template <typename T>
__global__ void append_rhs_kernel(T* dst, int64_t ld, const T* __restrict__ a, const T* __restrict__ delta, int64_t n0, int64_t n,
                                  int64_t npad, int64_t rows) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= npad) return;
  const T top = j < n0 ? a[j] : (j < n ? delta[j] : T(0));
  for (int64_t r = 0; r < rows; ++r) dst[r * ld + j] = r == 0 ? top : T(0);
}
int g3i_append_rhs(g3_ctx* ctx, void* dst, int64_t ld, const void* a, const void* delta, int64_t n0, int64_t n, int64_t npad,
                   int64_t rows, g3_dtype dt) {
  g3_by_dtype(dt, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((append_rhs_kernel<T>), dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, ctx->stream, (T*)dst, ld,
                       (const T*)a, (const T*)delta, n0, n, npad, rows);
  });
  G3_LAUNCH_CHECK();
  return G3_OK;
}

static int pad_row_launch(g3_ctx* ctx, void* dst, int64_t ld, const void* src, int64_t n, int64_t npad, int64_t rows, g3_dtype dt,
                          int batch = 1, int64_t dstride = 0, int64_t sstride = 0) {
  g3_by_dtype(dt, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((pad_row_kernel<T>), dim3((unsigned)((npad + 255) / 256), batch), dim3(256), 0, ctx->stream, (T*)dst, ld,
                       (const T*)src, n, npad, rows, dstride, sstride);
  });
  G3_LAUNCH_CHECK();
  return G3_OK;
}

// The tail of an evaluation (logp_finish_kernel): queued by the launch, its five doubles -- the four scalars and the pivot
// flag -- brought to the host by the fetch, which synchronises.
static int logp_finish_launch(g3_ctx* ctx, const void* K, int64_t N, int64_t Np, int64_t ldk, const void* rhs, void* a, int64_t a_from,
                              g3_dtype dt) {
  g3_by_dtype(dt, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((logp_finish_kernel<T>), dim3(1), dim3(1024), 0, ctx->stream, (const T*)K, N, Np, ldk, (const T*)rhs, (T*)a,
                       a_from, ctx->d_stats, ctx->d_info);
  });
  G3_LAUNCH_CHECK();
  return G3_OK;
}
static int logp_finish_fetch(g3_ctx* ctx, double st5[5]) {
  const int r = fetch_stats(ctx, st5, 5);
  if (!r) { ctx->info_clean = true; ctx->info_sync = true; }      // the kernel left the pivot flag cleared, and the host has waited for it
  return r;
}
int g3i_logp_finish(g3_ctx* ctx, const void* K, int64_t N, int64_t Np, int64_t ldk, const void* rhs, void* a, int64_t a_from, g3_dtype dt,
                    double st5[5]) {
  const int pr = g3i_prof_begin(ctx, G3_TAG_REDUCE, 0.0);
  const int r = logp_finish_launch(ctx, K, N, Np, ldk, rhs, a, a_from, dt);
  g3i_prof_end(ctx, pr);
  return r ? r : logp_finish_fetch(ctx, st5);
}
// min, mean and max of a device vector on the host (synchronises): the diagonal statistics at a leading dimension of 0
int g3i_vec_stats(g3_ctx* ctx, const void* v, int64_t n, g3_dtype dt, double out[3]) {
  const int rc = diag_stats_launch(ctx, const_cast<void*>(v), n, 0, dt, ctx->d_stats + 8, 0);
  return rc ? rc : fetch_stats(ctx, out, 3, 8);
}

// Shared implementation of g3_gp_factor / g3_gp_factor_predict.  K_dev is a tall buffer:
//   rows [0, Np)            the covariance, then its factor (lower triangle)
//   rows [Np, Np+128)       right-hand-side block whose first row is delta -> a = L^-1 delta
//   rows [Np+128, +Mp)      K(Xs, X) -> V = K(Xs, X) L^-T            (only when M > 0)
// The right-hand-side rows are carried through the factorisation itself (g3i_potrf_tall): the
// panel solves and trailing updates that factor K also perform the forward substitutions.
static int gp_factor_impl(g3_ctx* ctx, const g3_kernel_prog* prog, const void* X, int64_t N, int64_t ldx, int d,
                          const void* delta, g3_dtype dt, void* K, int64_t ldk, void* invd, void* a, double out[6],
                          const g3_kernel_prog* prog_cross, const void* Xs, int64_t M, int64_t ldxs, void* mu,
                          void* ss) {
  const int64_t Np = g3_roundup(N, G3_LB), RB = 128, Mp = M > 0 ? g3_roundup(M, 128) : 0;
  const int64_t E = RB + Mp;
  const size_t es = g3_esize(dt);
  const double es_d = (double)es;
  char* rhs = (char*)K + (size_t)Np * ldk * es;            // delta block
  char* Vp = rhs + (size_t)RB * ldk * es;                  // cross-covariance rows
  int rc = G3_OK;
  const unsigned gflags = G3_GRAM_LOWER | G3_GRAM_SCRUB | G3_GRAM_PAD_EYE;
  auto build_rhs = [&]() -> int {
    const int r0 = pad_row_launch(ctx, rhs, ldk, delta, N, Np, RB, dt);
    if (r0) return r0;
    if (M > 0) {
      // V = tt_to_num(cov(Xs, X))  (elliptical.py:78-79)
      const int pr = g3i_prof_begin(ctx, G3_TAG_CROSS_GRAM, (double)(N + M) * d * es_d + (double)N * M * es_d);
      int r = g3_gram(ctx, prog_cross, Xs, M, ldxs, X, N, ldx, d, dt, Vp, ldk, Mp, Np, G3_GRAM_SCRUB);
      g3i_prof_end(ctx, pr);
      if (r) return r;
    }
    return G3_OK;
  };
  // K = tt_to_cov(cov(X))  (elliptical.py:70-71), lower triangle only
  auto build = [&]() -> int {
    // algorithmic bytes of the lower-triangle Gram: N d s read + N(N+1)/2 s written
    const int pr = g3i_prof_begin(ctx, G3_TAG_GRAM, (double)N * d * es_d + 0.5 * (double)N * (N + 1) * es_d);
    int r = g3_gram(ctx, prog, X, N, ldx, nullptr, 0, 0, d, dt, K, ldk, Np, Np, gflags);
    if (r) return r;
    r = g3_cov_lift(ctx, K, N, ldk, dt);
    g3i_prof_end(ctx, pr);
    if (r) return r;
    return build_rhs();
  };
  auto factor = [&]() -> int {
    const int pr = g3i_prof_begin(ctx, G3_TAG_POTRF, (double)N * N * N / 3.0 + (double)N * N * (1 + M));
    const int r = g3i_potrf_tall(ctx, K, Np, ldk, dt, invd, E);
    g3i_prof_end(ctx, pr);
    return r;
  };
  // scalars of the evaluation: log-determinant, quadratic form, guards (and mean / sum of squares per query)
  double st4[5];
  auto finish = [&]() -> int {
    const int pr = g3i_prof_begin(ctx, G3_TAG_REDUCE, 2.0 * N * M);
    int r = logp_finish_launch(ctx, K, N, Np, ldk, rhs, a, 0, dt);
    if (r) return r;
    if (M > 0 && (mu || ss)) r = rows_dot_ss_launch(ctx, Vp, M, N, ldk, a, dt, mu, ss);
    g3i_prof_end(ctx, pr);
    if (r) return r;
    return logp_finish_fetch(ctx, st4);  // the one host synchronisation of a successful evaluation
  };
  rc = build();
  if (rc) return rc;
  // first attempt: the pivot flag comes back with the reductions -- one round trip per evaluation instead of two
  // (the reductions of a failed factorisation are simply discarded)
  rc = factor();
  if (rc) return rc;
  rc = finish();
  if (rc) return rc;
  int info = (int)st4[4];
  double tries = 0, fallback = 0;
  const int info0 = info;
  if (info != 0) {
    // jitter schedule of CholeskyRobust._cholesky (tensors.py:203-213); the Gram is rebuilt
    // instead of kept: it costs one HBM pass, a copy would cost the same plus 8 N^2 bytes
    rc = build();
    if (rc) return rc;
    double st[3];
    rc = g3_diag_stats(ctx, K, N, ldk, dt, st);
    if (rc) return rc;
    G3hJitter jit(st[1], st[0]);
    bool ok = false;
    for (int t = 0; t < G3hJitter::max_tries(); ++t) {
      tries += 1;
      if (t > 0) {
        rc = build();
        if (rc) return rc;
      }
      rc = g3_diag_add(ctx, K, N, ldk, dt, jit.value());
      if (rc) return rc;
      rc = factor();
      if (!rc) rc = g3i_read_info(ctx, &info);
      if (rc) return rc;
      if (info == 0) { ok = true; break; }
      jit.next();
    }
    if (!ok) {
      fallback = 1;
      // 1e-10 * I (tensors.py:221); right-hand sides are solved against it separately
      G3_HIP(hipMemset2DAsync(K, (size_t)ldk * es, 0, (size_t)Np * es, (size_t)Np, ctx->stream));
      rc = g3_diag_add(ctx, K, N, ldk, dt, (double)1e-10f);
      if (rc) return rc;
      if (Np > N) {
        rc = g3_diag_add(ctx, (char*)K + (size_t)N * (ldk + 1) * es, Np - N, ldk, dt, 1.0);
        if (rc) return rc;
      }
      rc = g3i_reset_info(ctx);
      if (rc) return rc;
      rc = g3i_trtri_blocks(ctx, K, Np, ldk, dt, invd);
      if (rc) return rc;
      rc = build_rhs();
      if (rc) return rc;
      rc = g3i_trsm_rlt(ctx, K, Np, ldk, rhs, E, ldk, dt, invd);
      if (rc) return rc;
    }
  }
  if (info0 != 0) {          // the jitter path produced a new factor: its scalars replace the discarded ones
    rc = finish();
    if (rc) return rc;
  }
  out[0] = st4[0];
  out[1] = st4[1];
  out[2] = st4[2];
  out[3] = tries;
  out[4] = fallback;
  out[5] = (double)info0;
  return G3_OK;
}

// ---------------------------------------------------------------------------------------
// Batched evaluation: the caller pattern of logp_chain / fixed_logp / find_MAP restarts
// (stochastic.py:515-564, 740-771: a Python loop, "TODO: Vectorized" in the reference) --
// many hyper-parameter vectors on the same inputs.  All `batch` covariances are built by one
// Gram launch (grid.z) and factored by ONE sweep whose GEMM / diagonal-block launches carry the
// batch in grid.y, so a problem too small to fill 256 CUs on its own still does.
//
// ctx->bbuf is ONE buffer shared by the batched entry points: g3_gp_factor_batched keeps its device programs, statistics
// and cooperative-kernel control words in it, g3_gp_cross_batched its device programs and, for Np > 1024, one member's V.
// Each call lays it out afresh from offset 0 and has queued its last use on ctx->stream when it returns, so the next call's
// writes, on the same stream, come after.  Growing it frees (hipFree waits for the device) and reallocates, so nothing may
// keep a pointer into it across calls or across a second ensure_bbuf within one call.
static int ensure_bbuf(g3_ctx* ctx, size_t bytes) {
  if (ctx->bbuf_bytes >= bytes) return G3_OK;
  if (ctx->bbuf) (void)hipFree(ctx->bbuf);
  ctx->bbuf = nullptr;
  ctx->bbuf_bytes = 0;
  G3_HIP(hipMalloc(&ctx->bbuf, bytes));
  ctx->bbuf_bytes = bytes;
  return G3_OK;
}

__global__ void __launch_bounds__(256) expand_progs_kernel(g3_kernel_prog* dst, const g3_kernel_prog* tmpl,
                                                          const double* fields, const int32_t* offs, int nfield) {
  const uint32_t* s = (const uint32_t*)tmpl;
  uint32_t* o = (uint32_t*)(dst + blockIdx.x);
  for (unsigned i = threadIdx.x; i < sizeof(g3_kernel_prog) / 4; i += 256) o[i] = s[i];
  __syncthreads();
  for (int i = threadIdx.x; i < nfield; i += 256)
    *(double*)((char*)o + offs[i]) = fields[(size_t)blockIdx.x * nfield + i];
}

int g3i_upload_members(g3_ctx* ctx, const MemberProgs& mp, int batch, size_t stat_bytes, size_t tail_bytes, g3_dev_members* out) {
  const G3hMemberLayout lo = g3h_member_layout(batch, mp.nfield, mp.progs != nullptr, stat_bytes, tail_bytes);
  int rc = ensure_bbuf(ctx, lo.total);
  if (rc) return rc;
  char* base = (char*)ctx->bbuf;
  out->progs = (g3_kernel_prog*)(base + lo.progs);
  out->stats = (double*)(base + lo.stats);
  out->tail = base + lo.tail;
  if (mp.progs) {
    G3_HIP(hipMemcpyAsync(out->progs, mp.progs, (size_t)batch * sizeof(g3_kernel_prog), hipMemcpyHostToDevice, ctx->stream));
    return G3_OK;
  }
  G3_HIP(hipMemcpyAsync(base + lo.tmpl, mp.tmpl, sizeof(g3_kernel_prog), hipMemcpyHostToDevice, ctx->stream));
  if (mp.nfield) {
    G3_HIP(hipMemcpyAsync(base + lo.fields, mp.fields, (size_t)batch * mp.nfield * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    G3_HIP(hipMemcpyAsync(base + lo.offs, mp.offs, (size_t)mp.nfield * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  }
  hipLaunchKernelGGL(expand_progs_kernel, dim3(batch), dim3(256), 0, ctx->stream, out->progs, (const g3_kernel_prog*)(base + lo.tmpl),
                     (const double*)(base + lo.fields), (const int32_t*)(base + lo.offs), mp.nfield);
  G3_LAUNCH_CHECK();
  return G3_OK;
}

// the members' pivot flags of the factorisation just queued -> ctx->h_info (valid once the stream is synchronised), and the
// device flags cleared for the next call: through g3i_reset_info inside the sweep's batch mode, else all `batch` directly
static int read_member_flags(g3_ctx* ctx, int batch, bool in_batch_mode, int* flags_host, int* flags_dev) {
  if (hipMemcpyAsync(flags_host, ctx->d_info, sizeof(int) * batch, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
    return G3_ERR_HIP;
  if (flags_dev && hipMemcpyAsync(flags_dev, ctx->d_info, sizeof(int) * batch, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)
    return G3_ERR_HIP;
  if (in_batch_mode) return g3i_reset_info(ctx);
  return hipMemsetAsync(ctx->d_info, 0, sizeof(int) * batch, ctx->stream) != hipSuccess ? G3_ERR_HIP : G3_OK;
}

int g3i_factor_members(g3_ctx* ctx, int batch, int64_t N, int64_t Np, const void* delta, int64_t ldd, g3_dtype dt, void* K, int64_t ldk,
                       int64_t kstride, void* invd, void* a, double* dstats, unsigned* coop_ctl, int* flags_host, int* flags_dev) {
  const int64_t RB = 128, wstride = Np * G3_LB;
  const size_t es = g3_esize(dt);
  char* rhs = (char*)K + (size_t)Np * ldk * es;
  const bool small = Np <= 2 * G3_LB;       // one workgroup per member does the whole evaluation (g3i_small_factor_batched)
  int rc;
  const int pr = g3i_prof_begin(ctx, G3_TAG_POTRF, (double)batch * ((double)N * N * N / 3.0 + (double)N * N));
  if (small) {
    rc = g3i_small_factor_batched(ctx, K, ldk, kstride, invd, wstride, delta, ldd, a, Np, dstats, batch, N, Np, dt);
    g3i_prof_end(ctx, pr);
    if (!rc) rc = read_member_flags(ctx, batch, false, flags_host, flags_dev);
  } else if (coop_ctl && Np <= ctx->tune.coop_max_n && batch >= ctx->tune.coop_min_batch) {
    // long chains of medium members: a group of workgroups per member, the whole batch in ONE launch (g3_chainb.hip): 1.2 -
    // 1.3x the lock-step sweep below at N <= 512, 1.08x at 768 - 1024; short batches (< ~200 members) stay with the sweep,
    // whose launches are at least as wide as the batch (profiles/r05_chain_medium.txt)
    rc = g3i_coop_factor_batched(ctx, K, ldk, kstride, invd, wstride, coop_ctl, batch, Np, dt);
    g3i_prof_end(ctx, pr);
    if (!rc) rc = read_member_flags(ctx, batch, false, flags_host, flags_dev);
  } else {
    // one sweep factors every member; a member whose pivot fails only stops its own launches
    g3_batch_scope mode(ctx, batch, kstride, wstride, invd, (size_t)batch * wstride * es);
    rc = g3i_potrf_tall(ctx, K, Np, ldk, dt, invd, RB);
    g3i_prof_end(ctx, pr);
    if (!rc) rc = read_member_flags(ctx, batch, true, flags_host, flags_dev);
  }
  if (rc) return rc;
  if (!small) {
    // a_b = first row of the solved right-hand-side block; log det and a^T a per member
    G3_HIP(hipMemcpy2DAsync(a, (size_t)Np * es, rhs, (size_t)kstride * es, (size_t)Np * es, (size_t)batch,
                            hipMemcpyDeviceToDevice, ctx->stream));
    rc = g3i_logp_terms_dev(ctx, K, N, ldk, a, dt, dstats, batch, kstride, Np);
  }
  return rc;
}

static int gp_factor_batched_impl(g3_ctx* ctx, const MemberProgs& mp, int batch, const void* X, int64_t N,
                                  int64_t ldx, int d, const void* delta, int64_t ldd, g3_dtype dt, void* K,
                                  int64_t ldk, int64_t kstride, void* invd, void* a, double* out) {
  if (batch < 1 || batch > G3_MAX_BATCH) return -3;
  if (!X) return -4;
  if (N <= 0) return -5;
  if (d < 1 || d > G3_MAXCOLS) return -7;
  if (ldx < d) return -6;
  if (!delta) return -8;
  if (ldd < N) return -9;
  if (!K) return -11;
  const int64_t Np = g3_roundup(N, G3_LB), RB = 128;
  const size_t es = g3_esize(dt);
  const int64_t al = 16 / (int64_t)es;
  if (ldk < Np || ldk % al) return -12;
  if (kstride < (Np + RB) * ldk || kstride % al) return -13;
  if (!invd) return -14;
  if (!a) return -15;
  if (!out) return -16;
  g3_kernel_prog first;                     // the structure every member shares
  if (g3i_validate_members(mp, batch, d, &first)) return -2;
  if (batch == 1)
    return gp_factor_impl(ctx, &first, X, N, ldx, d, delta, dt, K, ldk, invd, a, out, nullptr, nullptr, 0, 0, nullptr,
                          nullptr);
  // device copies of the programs, then the per-member statistics; behind them the cooperative kernel's control words
  const size_t sbytes = (size_t)batch * 4 * sizeof(double);
  g3_dev_members dm;
  int rc = g3i_upload_members(ctx, mp, batch, sbytes, g3i_coop_ctl_bytes(batch), &dm);
  if (rc) return rc;
  double* dstats = dm.stats;
  const int64_t wstride = Np * G3_LB;
  // K_b = tt_to_cov(cov(X)) (elliptical.py:70-71), right-hand-side block = [delta_b; 0]
  char* rhs = (char*)K + (size_t)Np * ldk * es;
  const bool small = Np <= 2 * G3_LB;       // one workgroup per member does the whole evaluation (g3i_small_factor_batched)
  int pr = g3i_prof_begin(ctx, G3_TAG_GRAM, (double)batch * ((double)N * d + 0.5 * (double)N * (N + 1)) * es);
  rc = g3i_gram_batched(ctx, dm.progs, &first, batch, X, N, ldx, d, dt, K, ldk, kstride, Np,
                        G3_GRAM_LOWER | G3_GRAM_SCRUB | G3_GRAM_PAD_EYE);
  if (!rc) rc = diag_stats_launch(ctx, K, N, ldk, dt, nullptr, 1, batch, kstride);
  if (!rc && !small) rc = pad_row_launch(ctx, rhs, ldk, delta, N, Np, RB, dt, batch, kstride, ldd);
  g3i_prof_end(ctx, pr);
  if (rc) return rc;
  rc = g3i_factor_members(ctx, batch, N, Np, delta, ldd, dt, K, ldk, kstride, invd, a, dstats, (unsigned*)dm.tail, ctx->h_info, nullptr);
  if (rc) return rc;
  double* hst = (double*)malloc(sbytes);
  if (!hst) return G3_ERR_NOMEM;
  if (hipMemcpyAsync(hst, dstats, sbytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess) {
    free(hst);
    snprintf(ctx->err, sizeof(ctx->err), "g3_gp_factor_batched: statistics copy failed");
    return G3_ERR_HIP;
  }
  int* infos = (int*)malloc(sizeof(int) * batch);
  if (!infos) { free(hst); return G3_ERR_NOMEM; }
  memcpy(infos, ctx->h_info, sizeof(int) * batch);
  for (int b = 0; b < batch && !rc; ++b) {
    double* o = out + 6 * b;
    if (infos[b] == 0) {
      o[0] = hst[4 * b]; o[1] = hst[4 * b + 1]; o[2] = hst[4 * b + 2];
      o[3] = 0; o[4] = 0; o[5] = 0;
    } else {
      // CholeskyRobust's jitter schedule (tensors.py:203-222) for this member alone
      g3_kernel_prog mine;
      mp.member(b, &mine);
      rc = gp_factor_impl(ctx, &mine, X, N, ldx, d, (const char*)delta + (size_t)b * ldd * es, dt,
                          (char*)K + (size_t)b * kstride * es, ldk, (char*)invd + (size_t)b * wstride * es,
                          (char*)a + (size_t)b * Np * es, o, nullptr, nullptr, 0, 0, nullptr, nullptr);
    }
  }
  free(hst);
  free(infos);
  return rc;
}

extern "C" int g3_gp_factor_batched(g3_ctx* ctx, const g3_kernel_prog* progs, int batch, const void* X, int64_t N,
                                    int64_t ldx, int d, const void* delta, int64_t ldd, g3_dtype dt, void* K,
                                    int64_t ldk, int64_t kstride, void* invd, void* a, double* out) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (!progs) return -2;
  MemberProgs mp;
  mp.progs = progs;
  return gp_factor_batched_impl(ctx, mp, batch, X, N, ldx, d, delta, ldd, dt, K, ldk, kstride, invd, a, out);
}

extern "C" int g3_gp_factor_batched_fields(g3_ctx* ctx, const g3_kernel_prog* tmpl, int batch, const double* fields,
                                           const int32_t* offsets, int nfield, const void* X, int64_t N, int64_t ldx,
                                           int d, const void* delta, int64_t ldd, g3_dtype dt, void* K, int64_t ldk,
                                           int64_t kstride, void* invd, void* a, double* out) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  return g3i_fields_call(tmpl, batch, false, fields, offsets, nfield, -16, [&](const MemberProgs& mp) {
    return gp_factor_batched_impl(ctx, mp, batch, X, N, ldx, d, delta, ldd, dt, K, ldk, kstride, invd, a, out);
  });
}

extern "C" int g3_gp_factor(g3_ctx* ctx, const g3_kernel_prog* prog, const void* X, int64_t N,
                            int64_t ldx, int d, const void* delta, g3_dtype dt, void* K, int64_t ldk,
                            void* invd, void* a, double out[6]) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (!prog) return -2;
  if (!X) return -3;
  if (N <= 0) return -4;
  if (!delta) return -7;
  if (!K) return -9;
  const int64_t Np = g3_roundup(N, G3_LB);
  if (ldk < Np || ldk % (16 / (int64_t)g3_esize(dt))) return -10;
  if (!invd) return -11;
  if (!a) return -12;
  if (!out) return -13;
  return gp_factor_impl(ctx, prog, X, N, ldx, d, delta, dt, K, ldk, invd, a, out, nullptr, nullptr, 0, 0, nullptr,
                        nullptr);
}

extern "C" int g3_gp_factor_predict(g3_ctx* ctx, const g3_kernel_prog* prog, const g3_kernel_prog* prog_cross,
                                    const void* X, int64_t N, int64_t ldx, int d, const void* delta,
                                    const void* Xs, int64_t M, int64_t ldxs, g3_dtype dt, void* K, int64_t ldk,
                                    void* invd, void* a, void* mu, void* ss, double out[6]) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (!prog) return -2;
  if (!prog_cross) return -3;
  if (!X) return -4;
  if (N <= 0) return -5;
  if (!delta) return -8;
  if (!Xs) return -9;
  if (M <= 0) return -10;
  if (!K) return -13;
  const int64_t Np = g3_roundup(N, G3_LB);
  if (ldk < Np || ldk % (16 / (int64_t)g3_esize(dt))) return -14;
  if (!invd) return -15;
  if (!a) return -16;
  if (!out) return -19;
  return gp_factor_impl(ctx, prog, X, N, ldx, d, delta, dt, K, ldk, invd, a, out, prog_cross, Xs, M, ldxs, mu, ss);
}

// One member's posterior cross pieces: V = tt_to_num(cov(Xs, X))  (elliptical.py:78-79), V <- V L^-T, then the row sums
// mu = V a, ss = |rows of V|^2 where asked for.  g3_gp_cross, and the batched entry points for members beyond their
// one-launch solve (Np > 1024); `tags`: only g3_gp_cross records the profiler's regions.
static int cross_single(g3_ctx* ctx, const g3_kernel_prog* prog, const void* Xs, int64_t M, int64_t ldxs, const void* X, int64_t N,
                        int64_t ldx, int d, const void* L, int64_t ldl, const void* invd, const void* a, g3_dtype dt, void* V,
                        int64_t ldv, void* mu, void* ss, bool tags) {
  const int64_t Np = g3_roundup(N, G3_LB), Mp = g3_roundup(M, 128);
  const double es_d = (double)g3_esize(dt);
  int pr = tags ? g3i_prof_begin(ctx, G3_TAG_CROSS_GRAM, (double)(N + M) * d * es_d + (double)N * M * es_d) : -1;
  int rc = g3_gram(ctx, prog, Xs, M, ldxs, X, N, ldx, d, dt, V, ldv, Mp, Np, G3_GRAM_SCRUB);
  g3i_prof_end(ctx, pr);
  if (rc) return rc;
  rc = g3i_reset_info(ctx);
  if (rc) return rc;
  pr = tags ? g3i_prof_begin(ctx, G3_TAG_TRSM, (double)N * N * M) : -1;
  rc = g3i_trsm_rlt(ctx, L, Np, ldl, V, Mp, ldv, dt, invd);
  g3i_prof_end(ctx, pr);
  if (rc) return rc;
  if (mu || ss) {
    pr = tags ? g3i_prof_begin(ctx, G3_TAG_REDUCE, 2.0 * N * M) : -1;
    rc = rows_dot_ss_launch(ctx, V, M, N, ldv, a, dt, mu, ss);
    g3i_prof_end(ctx, pr);
  }
  return rc;
}

extern "C" int g3_gp_cross(g3_ctx* ctx, const g3_kernel_prog* prog, const void* Xs, int64_t M,
                           int64_t ldxs, const void* X, int64_t N, int64_t ldx, int d, const void* L,
                           int64_t ldl, const void* invd, const void* a, g3_dtype dt, void* V, int64_t ldv,
                           void* mu, void* ss) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (!prog) return -2;
  if (!Xs) return -3;
  if (M <= 0) return -4;
  if (!X) return -6;
  if (N <= 0) return -7;
  if (!L) return -10;
  const int64_t Np = g3_roundup(N, G3_LB);
  const int64_t al = 16 / (int64_t)g3_esize(dt);
  if (ldl < Np || ldl % al) return -11;
  if (!V) return -14;
  if (ldv < Np || ldv % al) return -15;
  if (!invd) return -12;
  return cross_single(ctx, prog, Xs, M, ldxs, X, N, ldx, d, L, ldl, invd, a, dt, V, ldv, mu, ss, true);
}

// ---------------------------------------------------------------------------------------
// g3_gp_cross for every member of a chain after ONE g3_gp_factor_batched sweep: what the reference's average / particles
// (g3py/bayesian/models.py:489-543) get from a Python loop of single predictions over the rows of a trace.  The members'
// rectangular cross-Gram blocks come from one Gram launch with the member in grid.z (generated kernel or interpreter), the
// block forward solves and the row sums from one launch of g3_crossb.hip with the member in grid.y; V never leaves the
// library.  The cross-Gram workspace is the context's, at most G3_CROSSB_WORK bytes of it: longer chains go through in
// several (Gram, solve) launch pairs.
#define G3_CROSSB_WORK ((size_t)256 << 20)
static int gp_cross_batched_impl(g3_ctx* ctx, const MemberProgs& mp, int batch, const void* Xs, int64_t M, int64_t ldxs,
                                 const void* X, int64_t N, int64_t ldx, int d, const void* L, int64_t ldl, int64_t kstride,
                                 const void* invd, const void* a, g3_dtype dt, void* mu, void* ss, void* kdiag) {
  if (batch < 1 || batch > G3_MAX_BATCH) return -3;
  if (!Xs) return -4;
  if (M <= 0) return -5;
  if (!X) return -7;
  if (N <= 0) return -8;
  if (d < 1 || d > G3_MAXCOLS) return -10;
  if (ldxs < d) return -6;
  if (ldx < d) return -9;
  if (dt != G3_F64 && dt != G3_F32) return -16;
  g3_kernel_prog first;
  if (g3i_validate_members(mp, batch, d, &first)) return -2;
  const int64_t Np = g3_roundup(N, G3_LB), Mp = g3_roundup(M, 128);
  const size_t es = g3_esize(dt);
  const int64_t al = 16 / (int64_t)es;
  const bool solve = mu || ss;
  if (solve) {
    if (!L) return -11;
    if (ldl < Np || ldl % al) return -12;
    if (kstride < Np * ldl || kstride % al) return -13;
    if (!invd) return -14;
    if (mu && !a) return -15;
  }
  if (!solve && !kdiag) return G3_OK;
  // device copies of the members' programs; members beyond the one-launch solve keep their V (Mp x Np) behind them in the
  // same context buffer
  const bool big = solve && Np > 1024;
  g3_dev_members dm;
  int rc = g3i_upload_members(ctx, mp, batch, 0, big ? (size_t)Mp * Np * es : 0, &dm);
  if (rc) return rc;
  const g3_kernel_prog* dprogs = dm.progs;
  G3_HIP(hipStreamSynchronize(ctx->stream));          // the host arrays are borrowed for the call only
  if (kdiag) {
    rc = g3i_gram_diag_batched(ctx, dprogs, batch, Xs, M, ldxs, d, dt, kdiag, Mp);
    if (rc) return rc;
  }
  if (!solve) return G3_OK;
  const int64_t wstride = Np * G3_LB;
  if (!big) {
    const size_t per = (size_t)Mp * Np * es;
    int64_t cb = (int64_t)(G3_CROSSB_WORK / per);
    cb = cb < 1 ? 1 : (cb > batch ? batch : cb);
    rc = g3i_ensure_work(ctx, (size_t)cb * per);
    if (rc) return rc;
    for (int64_t b0 = 0; b0 < batch; b0 += cb) {
      const int nb = (int)(batch - b0 < cb ? batch - b0 : cb);
      // Ks_b = tt_to_num(cov_b(Xs, X))  (elliptical.py:78-79): NOISE contributes nothing to a cross block
      int pr = g3i_prof_begin(ctx, G3_TAG_CROSS_GRAM, (double)nb * ((double)(N + M) * d + (double)N * M) * es);
      rc = g3i_gram_rect_batched(ctx, dprogs + b0, &first, nb, Xs, M, ldxs, X, N, ldx, d, dt, ctx->work, Np, Mp * Np, Mp, Np,
                                 G3_GRAM_SCRUB, 0);
      g3i_prof_end(ctx, pr);
      if (rc) return rc;
      pr = g3i_prof_begin(ctx, G3_TAG_TRSM, (double)nb * (double)N * N * M);
      rc = g3i_cross_solve_batched(ctx, ctx->work, Mp * Np, (const char*)L + (size_t)b0 * kstride * es, ldl, kstride,
                                   (const char*)invd + (size_t)b0 * wstride * es, wstride,
                                   a ? (const char*)a + (size_t)b0 * Np * es : nullptr, Np,
                                   mu ? (char*)mu + (size_t)b0 * Mp * es : nullptr, ss ? (char*)ss + (size_t)b0 * Mp * es : nullptr,
                                   Mp, Mp, N, Np, nb, dt);
      g3i_prof_end(ctx, pr);
      if (rc) return rc;
    }
    return G3_OK;
  }
  // members beyond the one-launch solve: the single-member path (Gram, recursive solve, row sums) once per member
  for (int b = 0; b < batch; ++b) {
    g3_kernel_prog mine;
    mp.member(b, &mine);
    rc = cross_single(ctx, &mine, Xs, M, ldxs, X, N, ldx, d, (const char*)L + (size_t)b * kstride * es, ldl,
                      (const char*)invd + (size_t)b * wstride * es, a ? (const char*)a + (size_t)b * Np * es : nullptr, dt, dm.tail, Np,
                      mu ? (char*)mu + (size_t)b * Mp * es : nullptr, ss ? (char*)ss + (size_t)b * Mp * es : nullptr, false);
    if (rc) return rc;
  }
  return G3_OK;
}

extern "C" int g3_gp_cross_batched(g3_ctx* ctx, const g3_kernel_prog* progs, int batch, const void* Xs, int64_t M, int64_t ldxs,
                                   const void* X, int64_t N, int64_t ldx, int d, const void* L, int64_t ldl, int64_t kstride,
                                   const void* invd, const void* a, g3_dtype dt, void* mu, void* ss, void* kdiag) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (!progs) return -2;
  MemberProgs mp;
  mp.progs = progs;
  return gp_cross_batched_impl(ctx, mp, batch, Xs, M, ldxs, X, N, ldx, d, L, ldl, kstride, invd, a, dt, mu, ss, kdiag);
}

// The members as g3_gp_factor_batched_fields takes them: template + per-member doubles, expanded on the device by the same
// kernel, so the two forms hand the launches the same programs and give the same bits.
extern "C" int g3_gp_cross_batched_fields(g3_ctx* ctx, const g3_kernel_prog* tmpl, int batch, const double* fields,
                                          const int32_t* offsets, int nfield, const void* Xs, int64_t M, int64_t ldxs,
                                          const void* X, int64_t N, int64_t ldx, int d, const void* L, int64_t ldl,
                                          int64_t kstride, const void* invd, const void* a, g3_dtype dt, void* mu, void* ss,
                                          void* kdiag) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  return g3i_fields_call(tmpl, batch, true, fields, offsets, nfield, -19, [&](const MemberProgs& mp) {
    return gp_cross_batched_impl(ctx, mp, batch, Xs, M, ldxs, X, N, ldx, d, L, ldl, kstride, invd, a, dt, mu, ss, kdiag);
  });
}


// ---------------------------------------------------------------------------------------
// One joint draw of the curve per chain member after ONE g3_gp_factor_batched sweep (models.py:521-543: `particles`, a
// loop of single sampler calls in the reference -> gaussian.py:89-97, elliptical.py:86-92 per row).  Per launch group:
//   Ks_b -> V_b        one rectangular Gram launch, one solve launch that keeps V (g3_crossb.hip), mu_b on the way
//   C_b = P_b - V_b V_b^T   one square Gram launch (scrubbed and lifted per member with the noise kernel, as
//                      _prior_gram / tt_to_cov do), then the lower triangle through the batched MFMA GEMM of the
//                      factorisation sweep (member in grid.y; V and C have different strides: V plays the part of the
//                      block-inverse region of ctx->batch mode)
//   Lp_b               the device-side jitter schedule (g3_drawsb.hip), or the single call per member beyond 256 rows
//   out_b              loc_b + mu_b + Lp_b Z_b, one launch
// Everything lives in the context's workspace, G3_CROSSB_WORK bytes of it at most per group.
static int gp_draws_batched_impl(g3_ctx* ctx, const MemberProgs& mp, int batch, const void* Xs, int64_t M, int64_t ldxs,
                                 const void* X, int64_t N, int64_t ldx, int d, const void* L, int64_t ldl, int64_t kstride,
                                 const void* invd, const void* a, g3_dtype dt, int lift, const void* loc, const void* Z, int64_t S,
                                 void* out, void* C_out, void* Lp_out, int maxtries, int* tries_host, int* fallback_host,
                                 double* jitter_host) {
  if (batch < 1 || batch > G3_MAX_BATCH) return -3;
  if (!Xs) return -4;
  if (M <= 0) return -5;
  if (d < 1 || d > G3_MAXCOLS) return -10;
  if (ldxs < d) return -6;
  if (dt != G3_F64 && dt != G3_F32) return -16;
  const bool post = L != nullptr;
  const int64_t Np = post ? g3_roundup(N, G3_LB) : 0, Mp = g3_roundup(M, 128);
  const size_t es = g3_esize(dt);
  const int64_t al = 16 / (int64_t)es;
  if (post) {
    if (!X) return -7;
    if (N <= 0) return -8;
    if (ldx < d) return -9;
    if (ldl < Np || ldl % al) return -12;
    if (kstride < Np * ldl || kstride % al) return -13;
    if (!invd) return -14;
    if (!a) return -15;
  }
  if (!loc) return -18;
  if (!Z) return -19;
  if (S <= 0) return -20;
  if (!out) return -21;
  if (maxtries < 0) return -24;
  g3_kernel_prog first;
  if (g3i_validate_members(mp, batch, d, &first)) return -2;
  // device copies of the members' programs, as g3_gp_cross_batched makes them
  g3_dev_members dm;
  int rc = g3i_upload_members(ctx, mp, batch, 0, 0, &dm);
  if (rc) return rc;
  const g3_kernel_prog* dprogs = dm.progs;
  G3_HIP(hipStreamSynchronize(ctx->stream));          // the host arrays are borrowed for the call only
  // the workspace of one launch group of cb members: [scratch of the single robust call] V C Lp mu loc Z out res [inverses]
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const bool fused = Mp <= 2 * G3_LB;                 // the device-side schedule; larger members: g3_potrf_robust one by one
  const bool big = post && Np > 1024;                 // beyond the one-launch solve: g3_gp_cross's path per member
  const size_t v1 = post ? (size_t)Mp * Np * es : 0, c1 = (size_t)Mp * Mp * es, m1 = (size_t)Mp * es, l1 = (size_t)M * es,
               z1 = (size_t)M * S * es, r1 = 3 * sizeof(double);
  const size_t per = v1 + (C_out ? 0 : c1) + (Lp_out ? 0 : c1) + m1 + l1 + 2 * z1 + r1;
  // the parts that do not grow with the group count against the cap too: the single robust call's copy, or the fused kernel's
  // scratch for the block inverses (one slot per workgroup, at most the group's size)
  const size_t fixed = (fused ? up(g3i_robust_scratch_bytes(batch, M, dt)) : up(c1)) + 9 * 256;      // + the regions' alignment
  int64_t cb = G3_CROSSB_WORK > fixed ? (int64_t)((G3_CROSSB_WORK - fixed) / per) : 0;
  cb = cb < 1 ? 1 : (cb > batch ? batch : cb);
  const size_t o_scr = 0, o_v = o_scr + (fused ? 0 : up(c1)), o_c = o_v + up(cb * v1), o_l = o_c + (C_out ? 0 : up(cb * c1)),
               o_mu = o_l + (Lp_out ? 0 : up(cb * c1)), o_loc = o_mu + up(cb * m1), o_z = o_loc + up(cb * l1),
               o_out = o_z + up(cb * z1), o_res = o_out + up(cb * z1), o_w = o_res + up(cb * r1),
               total = o_w + (fused ? up(g3i_robust_scratch_bytes((int)cb, M, dt)) : 0);
  rc = g3i_ensure_work(ctx, total);
  if (rc) return rc;
  char* wk = (char*)ctx->work;
  const int64_t wstride = Np * G3_LB;
  double* hres = (double*)malloc((size_t)cb * r1);
  if (!hres) return G3_ERR_NOMEM;
  for (int64_t b0 = 0; b0 < batch && !rc; b0 += cb) {
    const int nb = (int)(batch - b0 < cb ? batch - b0 : cb);
    char* V = wk + o_v;
    char* Cb = C_out ? (char*)C_out + (size_t)b0 * c1 : wk + o_c;
    char* Lp = Lp_out ? (char*)Lp_out + (size_t)b0 * c1 : wk + o_l;
    char* mu = post ? wk + o_mu : nullptr;
    const g3_kernel_prog* dp = dprogs + b0;
    g3_kernel_prog mine;
    mp.member((int)b0, &mine);
    if (hipMemcpyAsync(wk + o_loc, (const char*)loc + (size_t)b0 * l1, (size_t)nb * l1, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(wk + o_z, (const char*)Z + (size_t)b0 * z1, (size_t)nb * z1, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
      snprintf(ctx->err, sizeof(ctx->err), "g3_gp_draws_batched: upload of loc / Z failed");
      rc = G3_ERR_HIP;
      break;
    }
    if (post && !big) {
      int pr = g3i_prof_begin(ctx, G3_TAG_CROSS_GRAM, (double)nb * ((double)(N + M) * d + (double)N * M) * es);
      rc = g3i_gram_rect_batched(ctx, dp, &mine, nb, Xs, M, ldxs, X, N, ldx, d, dt, V, Np, Mp * Np, Mp, Np, G3_GRAM_SCRUB, 0);
      g3i_prof_end(ctx, pr);
      if (rc) break;
      pr = g3i_prof_begin(ctx, G3_TAG_TRSM, (double)nb * (double)N * N * M);
      rc = g3i_cross_solve_batched(ctx, V, Mp * Np, (const char*)L + (size_t)b0 * kstride * es, ldl, kstride,
                                   (const char*)invd + (size_t)b0 * wstride * es, wstride, (const char*)a + (size_t)b0 * Np * es, Np,
                                   mu, nullptr, Mp, Mp, N, Np, nb, dt, 1);
      g3i_prof_end(ctx, pr);
      if (rc) break;
    } else if (post) {
      for (int b = 0; b < nb && !rc; ++b) {
        g3_kernel_prog pb;
        mp.member((int)b0 + b, &pb);
        rc = cross_single(ctx, &pb, Xs, M, ldxs, X, N, ldx, d, (const char*)L + (size_t)(b0 + b) * kstride * es, ldl,
                          (const char*)invd + (size_t)(b0 + b) * wstride * es, (const char*)a + (size_t)(b0 + b) * Np * es, dt,
                          V + (size_t)b * v1, Np, mu + (size_t)b * m1, nullptr, false);
      }
      if (rc) break;
    }
    // P_b = prog_b(Xs, Xs); with the noise kernel tt_to_cov: scrubbed, non-positive diagonal lifted (elliptical.py:70,74)
    int pr = g3i_prof_begin(ctx, G3_TAG_GRAM, (double)nb * ((double)M * d + 0.5 * (double)M * (M + 1)) * es);
    rc = g3i_gram_batched(ctx, dp, &mine, nb, Xs, M, ldxs, d, dt, Cb, Mp, Mp * Mp, Mp, G3_GRAM_LOWER | (lift ? G3_GRAM_SCRUB : 0u));
    if (!rc && lift) rc = diag_stats_launch(ctx, Cb, M, Mp, dt, nullptr, 1, nb, Mp * Mp);
    g3i_prof_end(ctx, pr);
    if (rc) break;
    if (post) {
      // batch mode first: g3i_reset_info then clears the flags of all nb members; V plays the block-inverse region
      g3_batch_scope mode(ctx, nb, Mp * Mp, Mp * Np, V, (size_t)nb * v1);
      rc = g3i_reset_info(ctx);
      if (!rc) rc = g3i_gemm_nt(ctx, Cb, Mp, V, Np, V, Np, Mp, Mp, Np, -1.0, 1.0, dt, 1);          // lower(C_b) -= V_b V_b^T  (elliptical.py:86-91)
      if (rc) break;
    }
    int* tr = tries_host ? tries_host + b0 : nullptr;
    int* fb = fallback_host ? fallback_host + b0 : nullptr;
    double* jt = jitter_host ? jitter_host + b0 : nullptr;
    if (fused) {
      pr = g3i_prof_begin(ctx, G3_TAG_POTRF, (double)nb * (double)M * M * M / 3.0);
      rc = g3i_potrf_robust_batched(ctx, Cb, Mp, Mp * Mp, Lp, Mp, Mp * Mp, nb, M, dt, maxtries, wk + o_w, (double*)(wk + o_res));
      g3i_prof_end(ctx, pr);
      if (rc) break;
    } else {
      // the single call works in the first bytes of the context's workspace: o_scr keeps them free for it
      if (hipMemsetAsync(Lp, 0, (size_t)nb * c1, ctx->stream) != hipSuccess) { rc = G3_ERR_HIP; break; }
      for (int b = 0; b < nb && !rc; ++b)
        rc = g3_potrf_robust(ctx, Cb + (size_t)b * c1, Mp, Lp + (size_t)b * c1, Mp, M, dt, maxtries, tr ? tr + b : nullptr,
                             fb ? fb + b : nullptr, jt ? jt + b : nullptr);
      if (rc) break;
    }
    rc = g3i_draws_batched(ctx, Lp, Mp, Mp * Mp, wk + o_loc, mu, Mp, wk + o_z, wk + o_out, M, S, nb, dt);
    if (rc) break;
    hipError_t e = hipMemcpyAsync((char*)out + (size_t)b0 * z1, wk + o_out, (size_t)nb * z1, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && fused) e = hipMemcpyAsync(hres, wk + o_res, (size_t)nb * r1, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
      snprintf(ctx->err, sizeof(ctx->err), "g3_gp_draws_batched: download failed: %s", hipGetErrorString(e));
      rc = G3_ERR_HIP;
      break;
    }
    if (fused)
      for (int b = 0; b < nb; ++b) {
        if (tr) tr[b] = (int)hres[3 * b];
        if (fb) fb[b] = (int)hres[3 * b + 1];
        if (jt) jt[b] = hres[3 * b + 2];
      }
  }
  free(hres);
  return rc;
}

extern "C" int g3_gp_draws_batched(g3_ctx* ctx, const g3_kernel_prog* progs, int batch, const void* Xs, int64_t M, int64_t ldxs,
                                   const void* X, int64_t N, int64_t ldx, int d, const void* L, int64_t ldl, int64_t kstride,
                                   const void* invd, const void* a, g3_dtype dt, int lift, const void* loc, const void* Z, int64_t S,
                                   void* out, void* C_dev, void* Lp_dev, int maxtries, int* tries_host, int* fallback_host,
                                   double* jitter_host) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (!progs) return -2;
  MemberProgs mp;
  mp.progs = progs;
  return gp_draws_batched_impl(ctx, mp, batch, Xs, M, ldxs, X, N, ldx, d, L, ldl, kstride, invd, a, dt, lift, loc, Z, S, out, C_dev,
                               Lp_dev, maxtries, tries_host, fallback_host, jitter_host);
}

extern "C" int g3_gp_draws_batched_fields(g3_ctx* ctx, const g3_kernel_prog* tmpl, int batch, const double* fields,
                                          const int32_t* offsets, int nfield, const void* Xs, int64_t M, int64_t ldxs,
                                          const void* X, int64_t N, int64_t ldx, int d, const void* L, int64_t ldl,
                                          int64_t kstride, const void* invd, const void* a, g3_dtype dt, int lift, const void* loc,
                                          const void* Z, int64_t S, void* out, void* C_dev, void* Lp_dev, int maxtries,
                                          int* tries_host, int* fallback_host, double* jitter_host) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  return g3i_fields_call(tmpl, batch, true, fields, offsets, nfield, -24, [&](const MemberProgs& mp) {
    return gp_draws_batched_impl(ctx, mp, batch, Xs, M, ldxs, X, N, ldx, d, L, ldl, kstride, invd, a, dt, lift, loc, Z, S, out, C_dev,
                                 Lp_dev, maxtries, tries_host, fallback_host, jitter_host);
  });
}

// draws = loc + L Z  (gaussian.py:92-95).  Z^T and the product live in the context's workspace.
template <typename T>
static int gp_sample_t(g3_ctx* ctx, const T* L, int64_t M, int64_t ldl, const T* loc, const T* Z, int64_t S, T* out) {
  const int64_t Mp = g3_roundup(M, 128), Sp = g3_roundup(S, 64);
  const size_t zt_bytes = (size_t)Sp * Mp * sizeof(T), c_bytes = (size_t)Mp * Sp * sizeof(T);
  int rc = g3i_ensure_work(ctx, zt_bytes + c_bytes);
  if (rc) return rc;
  T* Zt_dev = (T*)ctx->work;
  T* C_dev = (T*)((char*)ctx->work + zt_bytes);
  // Z^T, zero padded, assembled on the host (M x S is small next to the M x M factor)
  T* zt = (T*)calloc((size_t)Sp * Mp, sizeof(T));
  if (!zt) return G3_ERR_NOMEM;
  for (int64_t i = 0; i < M; ++i)
    for (int64_t s = 0; s < S; ++s) zt[s * Mp + i] = Z[i * S + s];
  hipError_t e = hipMemcpyAsync(Zt_dev, zt, zt_bytes, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  free(zt);
  if (e != hipSuccess) {
    snprintf(ctx->err, sizeof(ctx->err), "g3_gp_sample: upload of Z failed: %s", hipGetErrorString(e));
    return G3_ERR_HIP;
  }
  rc = g3i_reset_info(ctx);
  if (rc) return rc;
  const g3_dtype dt = sizeof(T) == 8 ? G3_F64 : G3_F32;
  rc = g3i_gemm_nt(ctx, C_dev, Sp, L, ldl, Zt_dev, Mp, Mp, Sp, Mp, 1.0, 0.0, dt, 0);      // C = L (Z^T)^T
  if (rc) return rc;
  T* c = (T*)malloc(c_bytes);
  if (!c) return G3_ERR_NOMEM;
  e = hipMemcpyAsync(c, C_dev, c_bytes, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    free(c);
    snprintf(ctx->err, sizeof(ctx->err), "g3_gp_sample: download failed: %s", hipGetErrorString(e));
    return G3_ERR_HIP;
  }
  for (int64_t i = 0; i < M; ++i)
    for (int64_t s = 0; s < S; ++s) out[i * S + s] = loc[i] + c[i * Sp + s];
  free(c);
  return G3_OK;
}

extern "C" int g3_gp_sample(g3_ctx* ctx, const void* L_dev, int64_t M, int64_t ldl, const void* loc_host,
                            const void* Z_host, int64_t S, g3_dtype dt, void* out_host) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (!L_dev) return -2;
  if (M <= 0) return -3;
  const int64_t Mp = g3_roundup(M, 128), al = 16 / (int64_t)g3_esize(dt);
  if (ldl < Mp || ldl % al) return -4;
  if (!loc_host) return -5;
  if (!Z_host) return -6;
  if (S <= 0) return -7;
  if (!out_host) return -9;
  return g3_by_dtype(dt, [&](auto t) {
    using T = decltype(t);
    return gp_sample_t<T>(ctx, (const T*)L_dev, M, ldl, (const T*)loc_host, (const T*)Z_host, S, (T*)out_host);
  });
}
