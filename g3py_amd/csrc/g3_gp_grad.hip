// The fused gradient entry points on a finished factor, for one member or a chain's members in the grid: K^-1 and alpha from what
// g3_gp_factor(_batched) left (g3i_kinv_alpha), then g3_gram_grad's kernel-parameter sums (g3_grad.hip) with K^-1 as the weight
// (g3_gp_dlogp*: log marginal likelihood) or with the weight below (g3_gp_dloo*: leave-one-out score, no counterpart in the reference).
//
// The leave-one-out weight.  With A = K^-1 of the factored covariance, alpha = A delta and c = diag A, the part of g3_gp_loo's
// score that depends on the parameters is F = sum_i [1/2 log c_i - 1/2 alpha_i^2 / c_i] and
//     dF = sum_ij W_ij dK_ij - u . d delta,    W = -A diag(q) A + 1/2 (u alpha^T + alpha u^T),
//     q_i = 1/2 (1 / c_i + alpha_i^2 / c_i^2),  u = A b,  b_i = alpha_i / c_i.
// g3_gram_grad's kernels sum 1/2 (alpha_i alpha_j - G_ij) dK_ij; with a zero alpha and
//     G = -2 W = M M^T - u alpha^T - alpha u^T,   M = A diag(s),  s_j = sqrt(c_j + alpha_j^2) / c_j,
//     u = M t,  t_j = alpha_j / sqrt(c_j + alpha_j^2)
// they give sum_ij W_ij dK_ij per slot.  Every O(n^3) step is one of the library's own -- the K^-1 sweep of g3_gp_dlogp
// (g3i_potri, 2 n^3 / 3) and ONE lower-triangular MFMA product (g3i_gemm_nt, n^3) -- and so are the two matrix-vector
// products (rows_dot_ss) and the sums (g3i_gram_grad_batched).  New here is the data movement around them:
//   dloo_weight_kernel   one pass over the lower triangle of K^-1 that writes the full square M (the product's operand must
//                        be dense), kdiag and t;
//   dloo_rank2_kernel    the rank-two part as one small pass over the lower triangle of G (not a second thin product: 2 n^2
//                        flops need no zero-padded panels and no second read of M).
// M, t and the zero alpha live in the context's workspace BEHIND the head the gradient kernels use (g3i_reserve_behind_grad), as
// g3_gram_vjp places its weight.
#include <optional>
#include <vector>

#include "g3_internal.h"

#define DL_T 64          // tile edge of the mirror
#define DL_THREADS 256
#define DL_GROUP_BYTES ((size_t)256 << 20)      // the members' M of one launch group

// ---- the prologue: K^-1 and alpha of every member
int g3i_kinv_sweep(g3_ctx* ctx, int batch, const void* L, int64_t np, int64_t ldl, int64_t kstride, const void* invd, g3_dtype dt,
                   void* Y, int64_t ldy, void* Kinv, int64_t ldc, int tag, double flops) {
  std::optional<g3_batch_scope> mode;       // one member: the plain single-member launches
  if (batch > 1) mode.emplace(ctx, batch, kstride, np * G3_LB, invd, (size_t)batch * np * G3_LB * g3_esize(dt));
  // in batch mode: EVERY member's pivot flag (a member whose first factorisation failed was re-run through the jitter
  // schedule on its own, and its flag of the batched sweep must not turn this sweep's launches into no-ops for it)
  int rc = g3i_reset_info(ctx);
  if (rc) return rc;
  const int rec = g3i_prof_begin(ctx, tag, flops);
  rc = g3i_potri(ctx, L, np, ldl, invd, dt, Y, ldy, Kinv, ldc);
  g3i_prof_end(ctx, rec);
  return rc;
}

// `batch` members after one factorisation sweep (L, Y, Kinv kstride elements apart, block inverses Np * 128, vectors Np; one member:
// kstride 0): Y = L^-T and Kinv = Y Y^T in ONE sweep recorded under `tag`, alpha_b = Y_b a_b (rows of Y dotted with a) in one launch
int g3i_kinv_alpha(g3_ctx* ctx, int batch, const void* L, int64_t N, int64_t ldl, int64_t kstride, const void* invd, const void* a,
                   g3_dtype dt, void* Y, int64_t ldy, void* Kinv, int64_t ldc, void* alpha, int tag) {
  const int64_t Np = g3_roundup(N, G3_LB);
  const int rc = g3i_kinv_sweep(ctx, batch, L, Np, ldl, kstride, invd, dt, Y, ldy, Kinv, ldc, tag, 2.0 * (double)batch * (double)N * N * N / 3.0);
  if (rc) return rc;
  return g3i_rows_dot_ss_batched(ctx, Y, Np, Np, ldy, a, dt, alpha, nullptr, batch, kstride, Np, Np);
}

// The _fields form of a batched entry point: its own checks, then `body(progs)`, the whole-programs implementation, on the members
// expanded here (the gradient kernels need each member's parameters on the host -- fast-path matching: 6 KB per member)
template <typename F>
static int fields_call_expanded(const g3_kernel_prog* tmpl, int batch, const double* fields, const int32_t* offsets, int nfield, int lo,
                                F&& body) {
  return g3i_fields_call(tmpl, batch, true, fields, offsets, nfield, lo, [&](const MemberProgs& mp) {
    std::vector<g3_kernel_prog> progs((size_t)batch);
    for (int b = 0; b < batch; ++b) mp.member(b, &progs[b]);
    return body(progs.data());
  });
}

// ---- dlogp: 1/2 sum_ij (alpha alpha^T - K^-1)_ij dK_ij / dtheta
// the prologue, then the kernel-parameter sums of all members in launches that carry the member in grid.y and ONE copy back
// (a chain of 4096 members: 3 launches instead of 12 288 and 4096 host waits)
static int dlogp_core(g3_ctx* ctx, const g3_kernel_prog* progs, int batch, const g3_grad_map* map, const void* X, int64_t N,
                      int64_t ldx, int d, const void* L, int64_t ldl, int64_t kstride, const void* invd, const void* a, g3_dtype dt,
                      void* Y, int64_t ldy, void* Kinv, int64_t ldc, void* alpha, double* out_host) {
  const int rc = g3i_kinv_alpha(ctx, batch, L, N, ldl, kstride, invd, a, dt, Y, ldy, Kinv, ldc, alpha, G3_TAG_POTRF);
  if (rc) return rc;
  return g3i_gram_grad_batched(ctx, progs, batch, map, X, N, ldx, d, dt, Kinv, ldc, kstride, alpha, g3_roundup(N, G3_LB), out_host);
}

extern "C" int g3_gp_dlogp(g3_ctx* ctx, const g3_kernel_prog* prog, const g3_grad_map* map, const void* X_dev,
                           int64_t N, int64_t ldx, int d, const void* L_dev, int64_t ldl, const void* invd_dev,
                           const void* a_dev, g3_dtype dt, void* Y_dev, int64_t ldy, void* Kinv_dev, int64_t ldc,
                           void* alpha_dev, double* out_host) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  const size_t es = g3_esize(dt);
  int rc = g3h_args_prog(prog, map, 2);
  if (!rc) rc = g3h_args_inputs(X_dev, N, ldx, d, 4, false);
  if (!rc) rc = g3h_args_factor(L_dev, N, false, ldl, nullptr, invd_dev, a_dev, es, 8);
  if (!rc) rc = g3h_args_padded_out(Y_dev, ldy, N, es, 13);
  if (!rc) rc = g3h_args_padded_out(Kinv_dev, ldc, N, es, 15);
  if (rc) return rc;
  if (!alpha_dev) return -17;
  if (!out_host) return -18;
  return dlogp_core(ctx, prog, 1, map, X_dev, N, ldx, d, L_dev, ldl, 0, invd_dev, a_dev, dt, Y_dev, ldy, Kinv_dev, ldc, alpha_dev, out_host);
}

// Batched dlogp: `batch` factorisations produced by ONE g3_gp_factor_batched sweep (members kstride
// elements apart in L_dev, diagonal-block inverses Npad*128 apart, a_dev batch x Npad) -- the caller
// pattern of fixed_dlogp / find_MAP restarts (g3py/processes/stochastic.py:554-564: a Python loop
// over single gradients in the reference).  Y_dev / Kinv_dev: batch members, kstride apart, ld = ldl.
extern "C" int g3_gp_dlogp_batched(g3_ctx* ctx, const g3_kernel_prog* progs, int batch, const g3_grad_map* map,
                                   const void* X_dev, int64_t N, int64_t ldx, int d, const void* L_dev, int64_t ldl,
                                   int64_t kstride, const void* invd_dev, const void* a_dev, g3_dtype dt, void* Y_dev,
                                   void* Kinv_dev, void* alpha_dev, double* out_host) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  int rc = g3h_args_progs(progs, batch, map, 2);
  if (!rc) rc = g3h_args_inputs(X_dev, N, ldx, d, 5, false);
  if (!rc) rc = g3h_args_factor(L_dev, N, false, ldl, &kstride, invd_dev, a_dev, g3_esize(dt), 9);
  if (rc) return rc;
  if (!Y_dev) return -15;
  if (!Kinv_dev) return -16;
  if (!alpha_dev) return -17;
  if (!out_host) return -18;
  return dlogp_core(ctx, progs, batch, map, X_dev, N, ldx, d, L_dev, ldl, kstride, invd_dev, a_dev, dt, Y_dev, ldl, Kinv_dev, ldl,
                    alpha_dev, out_host);
}

// g3_gp_dlogp_batched with the members given as in g3_gp_factor_batched_fields: a template plus the doubles that differ per member
extern "C" int g3_gp_dlogp_batched_fields(g3_ctx* ctx, const g3_kernel_prog* tmpl, int batch, const double* fields,
                                          const int32_t* offsets, int nfield, const g3_grad_map* map, const void* X_dev,
                                          int64_t N, int64_t ldx, int d, const void* L_dev, int64_t ldl, int64_t kstride,
                                          const void* invd_dev, const void* a_dev, g3_dtype dt, void* Y_dev, void* Kinv_dev,
                                          void* alpha_dev, double* out_host) {
  if (!ctx) return -1;
  return fields_call_expanded(tmpl, batch, fields, offsets, nfield, -18, [&](const g3_kernel_prog* progs) {
    return g3_gp_dlogp_batched(ctx, progs, batch, map, X_dev, N, ldx, d, L_dev, ldl, kstride, invd_dev, a_dev, dt, Y_dev, Kinv_dev,
                               alpha_dev, out_host);
  });
}

// ---- dloo: sum_ij W_ij dK_ij / dtheta

// M (np x np, compact, members mstride apart) = mirror(Kinv) diag(s) for the member in grid.z, from the lower triangle of
// Kinv (leading dimension ldc, members cstride apart); nothing above its diagonal is loaded (it may be NaN).  Rows and
// columns [n, np) of M are the identity, written here and not copied: every element of M is written.  One 64 x 64 tile of the
// lower triangle per workgroup (tiles above the diagonal leave at once); it writes the tile itself and, through an LDS tile
// whose rows are padded by one element (conflict-free column reads, as tril_transpose_pad_kernel in g3_vjp.hip), its mirror
// image, so both global sides move rows of 64 contiguous elements.  The diagonal tiles also write kdiag = diag Kinv and t
// (and clear alpha's padding), 0 from n on.  s is formed in double from the diagonal and alpha, once per tile column.
template <typename T>
__global__ void __launch_bounds__(DL_THREADS)
dloo_weight_kernel(const T* __restrict__ Kinv, int64_t ldc, int64_t cstride, T* __restrict__ alpha, int64_t vstride, int64_t n,
                   int64_t np, T* __restrict__ M, int64_t mstride, T* __restrict__ kdiag, T* __restrict__ t) {
  if (blockIdx.x > blockIdx.y) return;
  __shared__ T tile[DL_T][DL_T + 1];
  __shared__ T sc[2][DL_T];          // s of the tile's columns [0] and of its rows [1] (the mirror's columns)
  const int64_t b = blockIdx.z;
  Kinv += b * cstride;
  alpha += b * vstride;
  kdiag += b * vstride;
  t += b * vstride;
  M += b * mstride;
  const bool diag = blockIdx.x == blockIdx.y;
  const int64_t i0 = (int64_t)blockIdx.y * DL_T, j0 = (int64_t)blockIdx.x * DL_T;
  const int c = threadIdx.x & (DL_T - 1), r0 = threadIdx.x >> 6;
  if (r0 < 2) {
    const int64_t k = (r0 == 0 ? j0 : i0) + c;
    double s = 1.0, ck = 0.0, tk = 0.0;
    if (k < n) {
      ck = (double)Kinv[k * ldc + k];
      const double ak = (double)alpha[k], h = sqrt(ck + ak * ak);
      s = h / ck;
      tk = ak / h;
    }
    sc[r0][c] = (T)s;
    if (diag && r0 == 0) {
      kdiag[k] = (T)ck;
      t[k] = (T)tk;
      if (k >= n) alpha[k] = T(0);
    }
  }
  for (int r = r0; r < DL_T; r += DL_THREADS / DL_T) {
    const int64_t i = i0 + r, j = j0 + c;
    T v = T(0);
    if (i < n) {
      if (j <= i) v = Kinv[i * ldc + j];
    } else if (i == j) {
      v = T(1);
    }
    tile[r][c] = v;
  }
  __syncthreads();
  if (diag) {
    for (int r = r0; r < DL_T; r += DL_THREADS / DL_T) M[(i0 + r) * np + j0 + c] = (c <= r ? tile[r][c] : tile[c][r]) * sc[0][c];
  } else {
    for (int r = r0; r < DL_T; r += DL_THREADS / DL_T) {
      M[(i0 + r) * np + j0 + c] = tile[r][c] * sc[0][c];
      M[(j0 + r) * np + i0 + c] = tile[c][r] * sc[1][c];
    }
  }
}

// G_ij -= u_i alpha_j + alpha_i u_j on the lower triangle (j <= i < n) of the member in grid.z; nothing else is touched
template <typename T>
__global__ void __launch_bounds__(DL_THREADS)
dloo_rank2_kernel(T* __restrict__ G, int64_t ldg, int64_t gstride, const T* __restrict__ u, const T* __restrict__ alpha,
                  int64_t vstride, int64_t n) {
  const int64_t j = (int64_t)blockIdx.x * DL_THREADS + threadIdx.x;
  if (j >= n) return;
  const int64_t b = blockIdx.z;
  G += b * gstride;
  u += b * vstride;
  alpha += b * vstride;
  const T uj = u[j], aj = alpha[j];
  for (int64_t i = blockIdx.y; i < n; i += gridDim.y)
    if (j <= i) G[i * ldg + j] -= u[i] * aj + alpha[i] * uj;
}

// `batch` members after one factorisation sweep: L, Y and Kinv kstride elements apart, block inverses Np * 128, vectors Np
static int dloo_core(g3_ctx* ctx, const g3_kernel_prog* progs, int batch, const g3_grad_map* map, const void* X, int64_t N,
                     int64_t ldx, int d, const void* L, int64_t ldl, int64_t kstride, const void* invd, const void* a, g3_dtype dt,
                     void* Y, int64_t ldy, void* Kinv, int64_t ldc, void* alpha, void* kdiag, void* u, double* out_host) {
  const size_t es = g3_esize(dt);
  const int64_t Np = g3_roundup(N, G3_LB);
  const size_t mat = (size_t)Np * Np * es;
  const int gmax = DL_GROUP_BYTES / mat < 1 ? 1 : (int)(DL_GROUP_BYTES / mat);
  const int group = batch < gmax ? batch : gmax;
  const size_t zbytes = (size_t)g3_roundup((int64_t)((size_t)Np * es), 256), tbytes = (size_t)g3_roundup((int64_t)((size_t)batch * Np * es), 256);
  char* zero;
  int rc = g3i_reserve_behind_grad(ctx, batch, zbytes + tbytes + (size_t)group * mat, &zero);
  if (rc) return rc;
  char* t = zero + zbytes;
  char* M = t + tbytes;
  rc = g3i_kinv_alpha(ctx, batch, L, N, ldl, kstride, invd, a, dt, Y, ldy, Kinv, ldc, alpha, G3_TAG_TRSM);
  if (rc) return rc;
  G3_HIP(hipMemsetAsync(zero, 0, (size_t)Np * es, ctx->stream));
  const unsigned nt = (unsigned)(Np / DL_T);
  for (int b0 = 0; b0 < batch; b0 += group) {
    const int nb = batch - b0 < group ? batch - b0 : group;
    char* Yg = (char*)Y + (size_t)b0 * kstride * es;
    const size_t voff = (size_t)b0 * Np * es;
    int rec = g3i_prof_begin(ctx, G3_TAG_REDUCE, (double)nb * (double)N * N);
    g3_by_dtype(dt, [&](auto ty) {
      using T = decltype(ty);
      hipLaunchKernelGGL((dloo_weight_kernel<T>), dim3(nt, nt, (unsigned)nb), dim3(DL_THREADS), 0, ctx->stream,
                         (const T*)((const char*)Kinv + (size_t)b0 * kstride * es), ldc, kstride, (T*)((char*)alpha + voff), Np, N, Np,
                         (T*)M, Np * Np, (T*)((char*)kdiag + voff), (T*)(t + voff));
    });
    g3i_prof_end(ctx, rec);
    G3_LAUNCH_CHECK();
    rc = g3i_rows_dot_ss_batched(ctx, M, Np, Np, Np, t + voff, dt, (char*)u + voff, nullptr, nb, Np * Np, Np, Np);   // u = M t
    if (rc) return rc;
    {
      std::optional<g3_batch_scope> mode;     // C = the members' Y (kstride apart), both operands = their M (Np^2 apart)
      if (nb > 1) mode.emplace(ctx, nb, kstride, Np * Np, M, (size_t)nb * mat);
      rc = g3i_gemm_nt(ctx, Yg, ldy, M, Np, M, Np, Np, Np, Np, 1.0, 0.0, dt, 1);                     // G = M M^T, lower
    }
    if (rc) return rc;
    rec = g3i_prof_begin(ctx, G3_TAG_REDUCE, (double)nb * (double)N * N);
    g3_by_dtype(dt, [&](auto ty) {
      using T = decltype(ty);
      hipLaunchKernelGGL((dloo_rank2_kernel<T>), g3_tril_rows_grid(N, (unsigned)nb), dim3(DL_THREADS), 0, ctx->stream, (T*)Yg, ldy,
                         kstride, (const T*)((const char*)u + voff), (const T*)((const char*)alpha + voff), Np, N);
    });
    g3i_prof_end(ctx, rec);
    G3_LAUNCH_CHECK();
  }
  return g3i_gram_grad_batched(ctx, progs, batch, map, X, N, ldx, d, dt, Y, ldy, kstride, zero, 0, out_host);
}

extern "C" int g3_gp_dloo(g3_ctx* ctx, const g3_kernel_prog* prog, const g3_grad_map* map, const void* X_dev, int64_t N, int64_t ldx,
                          int d, const void* L_dev, int64_t ldl, const void* invd_dev, const void* a_dev, g3_dtype dt, void* Y_dev,
                          int64_t ldy, void* Kinv_dev, int64_t ldc, void* alpha_dev, void* kdiag_dev, void* u_dev, double* out_host) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  const size_t es = g3_esize(dt);
  int rc = g3h_args_prog(prog, map, 2);
  if (!rc) rc = g3h_args_inputs(X_dev, N, ldx, d, 4, false);
  if (rc) return rc;
  if (dt != G3_F64 && dt != G3_F32) return -12;       // (before the factor's sizes, which need the element size)
  rc = g3h_args_factor(L_dev, N, false, ldl, nullptr, invd_dev, a_dev, es, 8);
  if (!rc) rc = g3h_args_padded_out(Y_dev, ldy, N, es, 13);
  if (!rc) rc = g3h_args_padded_out(Kinv_dev, ldc, N, es, 15);
  if (rc) return rc;
  if (!alpha_dev) return -17;
  if (!kdiag_dev) return -18;
  if (!u_dev) return -19;
  if (!out_host) return -20;
  return dloo_core(ctx, prog, 1, map, X_dev, N, ldx, d, L_dev, ldl, 0, invd_dev, a_dev, dt, Y_dev, ldy, Kinv_dev, ldc, alpha_dev,
                   kdiag_dev, u_dev, out_host);
}

extern "C" int g3_gp_dloo_batched_fields(g3_ctx* ctx, const g3_kernel_prog* tmpl, int batch, const double* fields,
                                         const int32_t* offsets, int nfield, const g3_grad_map* map, const void* X_dev, int64_t N,
                                         int64_t ldx, int d, const void* L_dev, int64_t ldl, int64_t kstride, const void* invd_dev,
                                         const void* a_dev, g3_dtype dt, void* Y_dev, void* Kinv_dev, void* alpha_dev,
                                         void* kdiag_dev, void* u_dev, double* out_host) {
  if (!ctx) return -1;
  // the body sees the members as whole programs; its checks number their arguments as g3_gp_dlogp_batched does (shifted by the call)
  return fields_call_expanded(tmpl, batch, fields, offsets, nfield, -20, [&](const g3_kernel_prog* progs) -> int {
    g3_dev_guard _dg(ctx);
    int rc = g3h_args_progs(progs, batch, map, 2);
    if (!rc) rc = g3h_args_inputs(X_dev, N, ldx, d, 5, false);
    if (rc) return rc;
    if (dt != G3_F64 && dt != G3_F32) return -14;
    rc = g3h_args_factor(L_dev, N, false, ldl, &kstride, invd_dev, a_dev, g3_esize(dt), 9);
    if (rc) return rc;
    if (!Y_dev) return -15;
    if (!Kinv_dev) return -16;
    if (!alpha_dev) return -17;
    if (!kdiag_dev) return -18;
    if (!u_dev) return -19;
    if (!out_host) return -20;
    return dloo_core(ctx, progs, batch, map, X_dev, N, ldx, d, L_dev, ldl, kstride, invd_dev, a_dev, dt, Y_dev, ldl, Kinv_dev, ldl,
                     alpha_dev, kdiag_dev, u_dev, out_host);
  });
}
