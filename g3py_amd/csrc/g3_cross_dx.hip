// Gradients of the posterior location and variance with respect to the query inputs (g3_gp_cross_dx, g3_gram_diag_dx).
//
// With k_j = prog_cross(x*, x_j), A = K^-1 of the factored covariance, alpha = A delta and w = A k (row i of W = V Y^T,
// V = K(Xs, X) L^-T from g3_gp_cross and Y = L^-T from g3_gp_loo):
//     d loc  / d x*_c = d m / d x*_c + sum_j alpha_j d1_c k_j                    dmu[i][c] = the sum
//     d diag / d x*_c = d kss / d x*_c - 2 sum_j w_j d1_c k_j                    dss[i][c] = the doubled sum
//     d kss  / d x_c  = 2 d1_c prog(x, x')|x' = x                                g3_gram_diag_dx
// In the reference this is one tt.grad(..., space) through the graph of elliptical.py:81-97.  d1_c, the partial with respect to
// column c of the first argument, and the product rule over a program's factors are g3_kernel_dx.h's.
//   g3_gp_cross_dx   W = V Y^T as ONE MFMA product over the padded sizes (2 N^2 M flops; V's padding columns are zero and Y's
//                    padding is the identity, so W's padding columns are zero and the plain product is exact), then one pass
//                    over the M x N pairs (cross_dx_kernel) that reads W once and re-evaluates the kernel expression per pair,
//                    and a small launch that adds the column splits in a fixed order.  No atomics: two calls give the same bits.
//   g3_gram_diag_dx  the pair function at x' = x, doubled, one thread per query row.
//
// cross_dx_kernel.  A workgroup of 4 waves owns CD_ROWS = 4 query rows, one per wave, and one split of the columns
// (blockIdx.y); a lane owns one column of a 64-column tile, so a wave reads 512 contiguous bytes of its row of W and
// every tile of X is staged in LDS once for the four rows.  The splits are what fills the chip when M is 1 .. 64 (an
// optimiser's query): about CD_BLOCKS workgroups are asked for whatever M is, each split a whole number of tiles.
// A lane's 2 * width running sums (dmu and dss of `width` columns of x*, in fp64 for both dtypes) are indexed by the column
// a leaf's `dims` names -- data, not code -- so they cannot live in registers without a select chain per update; they are
// thread-private in LDS, slot-major (a wave touches 64 consecutive doubles: conflict-free), as gram_grad_kernel keeps its
// sums, and a query of more than CD_MAXW = 8 columns takes ceil(d / 8) launches over column windows [lo, lo + width).
// LDS per workgroup: the program (6 KiB) + X tile 64 x (d | 1) doubles (2.5 KiB at d = 4, 20.5 KiB at d = 40) + the four
// query rows + alpha 0.5 KiB + the sums 4 KiB x width (16 KiB at d = 4, 32 KiB from d = 8 on) + 2 KiB x nleaf of leaf
// values when a product has several factors: 25 KiB for SE d = 4, 41 KiB from d = 8 on, at most 77 KiB (2 workgroups per
// CU).  Registers: 152 VGPRs, no scratch (the interpreter's switch over 15 leaf kinds in fp64) -- 3 waves per SIMD, that
// is 3 workgroups per CU, which is the bound up to 53 KiB of LDS.  Measured (profiles/predict_dx.md): the pass is bound by
// the interpreter's arithmetic, not by the read of W -- 46 G pairs/s for SE d = 4 in fp64, 0.37 TB/s of W -- and is a
// twelfth of the product in front of it.
// At the end a wave sums each slot over its lanes and writes partial[split][row][slot]; cross_dx_reduce_kernel adds the
// splits in order and writes the M x width block of the outputs in the caller's dtype.
#include "g3_internal.h"
#include "g3_kernel_dx.h"

#define CD_T 64            // columns per tile (one per lane)
#define CD_ROWS 4          // query rows per workgroup (one per wave)
#define CD_THREADS 256
#define CD_MAXW 8          // columns of x* per launch
#define CD_BLOCKS 2048     // workgroups asked for: the column splits make up what the row groups leave

// thread-private sums in LDS, slot-major: [dmu of width columns][dss of width columns][CD_THREADS]
struct CrossDxAcc {
  double* acc;
  int lo, width, tid;
  double wm, ws;       // alpha_j and 2 W_ij
  bool mu, ss;
  __device__ __forceinline__ void operator()(int c, double t) const {
    const unsigned s = (unsigned)(c - lo);
    if (s >= (unsigned)width) return;
    if (mu) acc[s * CD_THREADS + tid] += wm * t;
    if (ss) acc[(width + s) * CD_THREADS + tid] += ws * t;
  }
};

template <typename T>
__global__ void __launch_bounds__(CD_THREADS)
cross_dx_kernel(const g3_kernel_prog* __restrict__ prog, const T* __restrict__ Xs, int64_t M, int64_t ldxs,
                const T* __restrict__ X, int64_t N, int64_t ldx, int d, const T* __restrict__ alpha, const T* __restrict__ W,
                int64_t ldw, double* __restrict__ partial, int lo, int width, int64_t chunk, int nlv) {
  // alpha == nullptr: no dmu; W == nullptr: no dss.  chunk: columns per split, a multiple of CD_T.  nlv: the leaves' values are
  // kept (a product has several factors), that many per thread
  extern __shared__ __attribute__((aligned(16))) char smem_cd[];
  const int dp = d | 1;
  double* xi_s = (double*)smem_cd;            // CD_ROWS x dp
  double* xj_s = xi_s + CD_ROWS * dp;         // CD_T x dp
  double* aj_s = xj_s + CD_T * dp;            // CD_T
  double* acc_s = aj_s + CD_T;                // 2 width x CD_THREADS
  double* lv_s = acc_s + 2 * width * CD_THREADS;   // nlv x CD_THREADS
  __shared__ g3_kernel_prog sp;               // read many times per pair with data-dependent indices: kept in LDS
  __shared__ double qconst[G3_MAXLEAF];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int e = tid; e < (int)(sizeof(g3_kernel_prog) / 4); e += CD_THREADS)
    reinterpret_cast<int*>(&sp)[e] = reinterpret_cast<const int*>(prog)[e];
  for (int s = 0; s < 2 * width; ++s) acc_s[s * CD_THREADS + tid] = 0.0;
  const int64_t i0 = (int64_t)blockIdx.x * CD_ROWS;
  for (int e = tid; e < CD_ROWS * d; e += CD_THREADS) {
    const int r = e / d, c = e - r * d;
    xi_s[r * dp + c] = i0 + r < M ? (double)Xs[(i0 + r) * ldxs + c] : 0.0;
  }
  __syncthreads();
  if (tid == 0) (void)prog_qconst(sp, qconst);
  const bool multi = nlv > 0;
  const int64_t i = i0 + wv;
  const double* xi = xi_s + wv * dp;
  const int64_t jb = (int64_t)blockIdx.y * chunk, je = jb + chunk < N ? jb + chunk : N;
  for (int64_t j0 = jb; j0 < je; j0 += CD_T) {
    __syncthreads();          // (the first: qconst is published; later: every wave is done with the tile before)
    for (int e = tid; e < CD_T * d; e += CD_THREADS) {
      const int r = e / d, c = e - r * d;
      xj_s[r * dp + c] = j0 + r < N ? (double)X[(j0 + r) * ldx + c] : 0.0;
    }
    if (tid < CD_T) aj_s[tid] = (alpha != nullptr && j0 + tid < N) ? (double)alpha[j0 + tid] : 0.0;
    __syncthreads();
    const int64_t j = j0 + lane;
    if (i >= M || j >= N) continue;
    const CrossDxAcc add{acc_s, lo, width, tid, aj_s[lane], W != nullptr ? 2.0 * (double)W[i * ldw + j] : 0.0,
                         alpha != nullptr, W != nullptr};
    prog_d1(sp, qconst, multi, xi, xj_s + lane * dp, false, lv_s + tid, CD_THREADS, add);
  }
  // a wave's lanes hold the sums of one query row over this split's columns
  if (i < M) {
    double* out = partial + ((size_t)blockIdx.y * M + i) * (2 * width);
    for (int s = 0; s < 2 * width; ++s) {
      const double v = wave_sum(acc_s[s * CD_THREADS + tid]);
      if (lane == 0) out[s] = v;
    }
  }
}

// dmu[i][lo + c] = sum over the splits, in order, of partial[split][i][c]; dss the same from slot width + c
template <typename T>
__global__ void __launch_bounds__(256)
cross_dx_reduce_kernel(const double* __restrict__ partial, int nsplit, int64_t M, int lo, int width, T* __restrict__ dmu,
                       T* __restrict__ dss, int64_t ldg) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= M * width) return;
  const int64_t i = e / width;
  const int c = (int)(e - i * width);
  double m = 0.0, s = 0.0;
  for (int q = 0; q < nsplit; ++q) {
    const double* p = partial + ((size_t)q * M + i) * (2 * width);
    m += p[c];
    s += p[width + c];
  }
  if (dmu) dmu[i * ldg + lo + c] = (T)m;
  if (dss) dss[i * ldg + lo + c] = (T)s;
}

// one thread per query row: d prog(x, x) / d x_c = 2 d1_c prog(x, x')|x' = x on the square-case diagonal
struct DiagDxAcc {
  double* acc;         // [d][64]
  int tid;
  __device__ __forceinline__ void operator()(int c, double t) const { acc[c * 64 + tid] += 2.0 * t; }
};

template <typename T>
__global__ void __launch_bounds__(64)
gram_diag_dx_kernel(const g3_kernel_prog* __restrict__ prog, const T* __restrict__ Xs, int64_t M, int64_t ldxs, int d,
                    T* __restrict__ dk, int64_t ldg, int nlv) {
  extern __shared__ __attribute__((aligned(16))) char smem_dd[];
  const int dp = d | 1;
  double* x_s = (double*)smem_dd;             // 64 x dp
  double* acc_s = x_s + 64 * dp;              // d x 64
  double* lv_s = acc_s + d * 64;              // nlv x 64
  __shared__ g3_kernel_prog sp;
  __shared__ double qconst[G3_MAXLEAF];
  const int tid = threadIdx.x;
  for (int e = tid; e < (int)(sizeof(g3_kernel_prog) / 4); e += 64)
    reinterpret_cast<int*>(&sp)[e] = reinterpret_cast<const int*>(prog)[e];
  __syncthreads();
  if (tid == 0) (void)prog_qconst(sp, qconst);
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 64 + tid;
  if (i >= M) return;
  double* xi = x_s + tid * dp;
  for (int c = 0; c < d; ++c) {
    xi[c] = (double)Xs[i * ldxs + c];
    acc_s[c * 64 + tid] = 0.0;
  }
  prog_d1(sp, qconst, nlv > 0, xi, xi, true, lv_s + tid, 64, DiagDxAcc{acc_s, tid});
  for (int c = 0; c < d; ++c) dk[i * ldg + c] = (T)acc_s[c * 64 + tid];
}

static int prog_nlv(const g3_kernel_prog* prog) {
  for (int p = 0; p < prog->nprod; ++p)
    if (prog->prod[p].nfac > 1) return prog->nleaf;
  return 0;
}

static size_t cross_dx_lds(int d, int width, int nlv) {
  return ((size_t)(CD_ROWS + CD_T) * (d | 1) + CD_T + (size_t)(2 * width + nlv) * CD_THREADS) * sizeof(double);
}

template <typename T>
static int cross_dx_pass(g3_ctx* ctx, const g3_kernel_prog* dprog, int nlv, const T* Xs, int64_t M, int64_t ldxs, const T* X, int64_t N,
                         int64_t ldx, int d, const T* alpha, const T* W, int64_t ldw, T* dmu, T* dss, int64_t ldg) {
  auto kern = cross_dx_kernel<T>;
  static bool attr_set[G3_MAX_DEVICES] = {};
  const int dev_slot = ctx->device & (G3_MAX_DEVICES - 1);
  if (!attr_set[dev_slot]) {
    G3_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)cross_dx_lds(G3_MAXCOLS, CD_MAXW, G3_MAXLEAF)));
    attr_set[dev_slot] = true;
  }
  // the splits: whole tiles, as many as bring the grid to about CD_BLOCKS workgroups
  const int64_t groups = (M + CD_ROWS - 1) / CD_ROWS, tiles = (N + CD_T - 1) / CD_T;
  int64_t want = CD_BLOCKS / groups;
  want = want < 1 ? 1 : (want > tiles ? tiles : want);
  const int64_t chunk = (tiles + want - 1) / want * CD_T;
  const int64_t nsplit = (N + chunk - 1) / chunk;
  const int wmax = d < CD_MAXW ? d : CD_MAXW;
  int rc = g3i_ensure_work(ctx, (size_t)nsplit * M * 2 * wmax * sizeof(double));
  if (rc) return rc;
  double* partial = (double*)ctx->work;
  for (int lo = 0; lo < d; lo += CD_MAXW) {
    const int width = d - lo < CD_MAXW ? d - lo : CD_MAXW;
    hipLaunchKernelGGL(kern, dim3((unsigned)groups, (unsigned)nsplit), dim3(CD_THREADS), cross_dx_lds(d, width, nlv), ctx->stream,
                       dprog, Xs, M, ldxs, X, N, ldx, d, alpha, W, ldw, partial, lo, width, chunk, nlv);
    G3_LAUNCH_CHECK();
    hipLaunchKernelGGL((cross_dx_reduce_kernel<T>), dim3((unsigned)((M * width + 255) / 256)), dim3(256), 0, ctx->stream, partial,
                       (int)nsplit, M, lo, width, dmu, dss, ldg);
    G3_LAUNCH_CHECK();
  }
  return G3_OK;
}

extern "C" int g3_gp_cross_dx(g3_ctx* ctx, const g3_kernel_prog* prog, const void* Xs, int64_t M, int64_t ldxs, const void* X,
                              int64_t N, int64_t ldx, int d, g3_dtype dt, const void* alpha, const void* V, int64_t ldv,
                              const void* Y, int64_t ldy, void* W, int64_t ldw, void* dmu, void* dss, int64_t ldg) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (!prog) return -2;
  if (!Xs) return -3;
  if (M <= 0) return -4;
  if (d < 1 || d > G3_MAXCOLS) return -9;          // (before the leading dimensions, which are measured against it)
  if (ldxs < d) return -5;
  if (!X) return -6;
  if (N <= 0) return -7;
  if (ldx < d) return -8;
  if (g3h_validate_prog(prog, d)) return -2;
  if (dt != G3_F64 && dt != G3_F32) return -10;
  if (!dmu && !dss) return -18;                    // (before the inputs: which of them are needed depends on the outputs)
  if (dmu && !alpha) return -11;
  const int64_t Np = g3_roundup(N, G3_LB), Mp = g3_roundup(M, G3_LB);
  const int64_t al = 16 / (int64_t)g3_esize(dt);
  if (dss) {
    if (!V) return -12;
    if (ldv < Np || ldv % al) return -13;
    if (!Y) return -14;
    if (ldy < Np || ldy % al) return -15;
    if (!W) return -16;
    if (ldw < Np || ldw % al) return -17;
  }
  if (ldg < d) return -20;
  int rc;
  if (dss) {
    rc = g3i_reset_info(ctx);                      // (the product is a no-op behind a failed pivot's flag)
    if (rc) return rc;
    rc = g3i_gemm_nt(ctx, W, ldw, V, ldv, Y, ldy, Mp, Np, Np, 1.0, 0.0, dt, 0);
    if (rc) return rc;
  }
  const g3_kernel_prog* dprog;
  rc = g3i_upload_prog(ctx, prog, 0, &dprog);
  if (rc) return rc;
  const int rec = g3i_prof_begin(ctx, G3_TAG_REDUCE, 4.0 * (double)M * (double)N * d);
  rc = g3_by_dtype(dt, [&](auto t) {
    using T = decltype(t);
    return cross_dx_pass<T>(ctx, dprog, prog_nlv(prog), (const T*)Xs, M, ldxs, (const T*)X, N, ldx, d, dmu ? (const T*)alpha : nullptr,
                            dss ? (const T*)W : nullptr, ldw, (T*)dmu, (T*)dss, ldg);
  });
  g3i_prof_end(ctx, rec);
  return rc;
}

extern "C" int g3_gram_diag_dx(g3_ctx* ctx, const g3_kernel_prog* prog, const void* Xs, int64_t M, int64_t ldxs, int d, g3_dtype dt,
                               void* dk, int64_t ldg) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (!prog) return -2;
  if (!Xs) return -3;
  if (M <= 0) return -4;
  if (d < 1 || d > G3_MAXCOLS) return -6;
  if (ldxs < d) return -5;
  if (g3h_validate_prog(prog, d)) return -2;
  if (dt != G3_F64 && dt != G3_F32) return -7;
  if (!dk) return -8;
  if (ldg < d) return -9;
  const g3_kernel_prog* dprog;
  int rc = g3i_upload_prog(ctx, prog, 0, &dprog);
  if (rc) return rc;
  const int nlv = prog_nlv(prog);
  const size_t lds = ((size_t)64 * (d | 1) + (size_t)(d + nlv) * 64) * sizeof(double);
  g3_by_dtype(dt, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((gram_diag_dx_kernel<T>), dim3((unsigned)((M + 63) / 64)), dim3(64), lds, ctx->stream, dprog, (const T*)Xs, M,
                       ldxs, d, (T*)dk, ldg, nlv);
  });
  G3_LAUNCH_CHECK();
  return G3_OK;
}
