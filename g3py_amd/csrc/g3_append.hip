// Appending observations to a factored covariance without a refit (include/g3hip_online.h): g3_gp_append resumes the
// factorisation of g3_gp_factor at a block row, g3_gp_cross_append extends the cross solve of g3_gp_cross by the new columns.
//
// A lower Cholesky factor is built from its leading principal submatrices, so with N0 rows factored and N1 wanted, every row
// of L, of the block inverses and of a = L^-1 delta below n0 = rounddown(N0, 128) is already what a factorisation of all N1
// rows would produce.  What is left is the block row [n0, Np1), Np1 = roundup(N1, 128), r = Np1 - n0 rows:
//
//   rows      K[n0:Np1, 0:Np1)  <- the covariance                              g3_gram_rows (square-case NOISE / WN, identity padding)
//   rhs       K[Np1:Np1+128, :) <- [a[0:n0), delta[n0:N1), 0 ...; 0]           one small launch (g3i_append_rhs)
//   panel     K[n0:Np1, 0:n0)   <- K[n0:Np1, 0:n0) L[0:n0, 0:n0)^-T            g3i_trsm_rlt, in place
//   update    K[n0:Np1+128, n0:Np1) -= K[n0:Np1+128, 0:n0) K[n0:Np1, 0:n0)^T   ONE g3i_gemm_nt over the r + 128 stacked rows: the
//                                                                              Schur update of the corner and the forward
//                                                                              substitution of the right-hand side together
//   corner    K[n0:Np1, n0:Np1) <- its factor, the rhs rows ride along         g3i_potrf_tall, E = 128
//   finish    a[n0:Np1), log det, a^T a, guards over all N1 rows               the finishing reduction of g3_gp_factor
//
// about N0^2 r flops for the panel and r^2 (N0 + r / 3) for the rest, against N1^3 / 3 for the refit.  The rows of the old last
// block, when N0 is no multiple of 128, are recomputed with the rest: that replaces their identity padding without a special
// case.  Nothing below row n0 is written, and nothing is read that the call has not written or the precondition does not
// cover: the strict upper triangle, the new rows and the columns from Np1 on may hold anything.
//
// The reference's data-dependent rules act on the WHOLE matrix, so where one would have acted the append declines and the
// caller refits: tt_to_cov lifts the diagonal by (1e-6 - min) when its minimum is not positive (tensors.py:95-98) -- checked
// first, on g3_gram_diag of all N1 points, before anything is written -- and the jitter schedule of CholeskyRobust
// (tensors.py:203-213) restarts from the whole matrix -- a failed pivot of the corner is reported, not repaired.
#include "g3_internal.h"
#include "g3hip_online.h"

extern "C" int g3_gp_append(g3_ctx* ctx, const g3_kernel_prog* prog, const void* X, int64_t N0, int64_t N1, int64_t ldx, int d,
                            const void* delta, g3_dtype dt, void* K, int64_t ldk, void* invd, void* a, double out[8]) {
  if (!ctx || ctx->batch > 1) return -1;
  g3_dev_guard _dg(ctx);
  if (!prog) return -2;
  if (!X) return -3;
  int rc = g3h_args_append(N0, N1, 4);
  if (rc) return rc;
  if (d < 1 || d > G3_MAXCOLS) return -7;
  if (ldx < d) return -6;
  if (g3h_validate_prog(prog, d)) return -2;
  if (!delta) return -8;
  if (dt != G3_F64 && dt != G3_F32) return -9;
  if (!K) return -10;
  const size_t es = g3_esize(dt);
  const G3hAppendPlan p = g3h_append_plan(N0, N1, ldk);
  if (ldk < p.Np1 || ldk % (16 / (int64_t)es)) return -11;
  if (!invd) return -12;
  if (!a) return -13;
  if (!out) return -14;
  const double es_d = (double)es;
  for (int i = 0; i < 8; ++i) out[i] = 0.0;
  // ---- refusal check: the lift of tt_to_cov depends on the minimum of the whole diagonal
  rc = g3i_ensure_work(ctx, (size_t)N1 * es);
  if (rc) return rc;
  rc = g3_gram_diag(ctx, prog, X, N1, ldx, d, dt, ctx->work);
  if (rc) return rc;
  double dg[3];
  rc = g3i_vec_stats(ctx, ctx->work, N1, dt, dg);
  if (rc) return rc;
  if (!(dg[0] > 0.0) || !__builtin_isfinite(dg[1]) || !__builtin_isfinite(dg[2])) {
    out[6] = 1.0;
    return G3_OK;
  }
  char* rows = (char*)K + (size_t)p.rows_off * es;
  char* corner = (char*)K + (size_t)p.corner_off * es;
  char* rhs = (char*)K + (size_t)p.rhs_off * es;
  // ---- the new block row of the covariance and the resumed right-hand side
  int pr = g3i_prof_begin(ctx, G3_TAG_GRAM, (double)N1 * d * es_d + (double)(N1 - p.n0) * N1 * es_d);
  rc = g3_gram_rows(ctx, prog, X, N1, ldx, d, p.n0, p.r, dt, rows, ldk, G3_GRAM_SCRUB | G3_GRAM_PAD_EYE);
  if (!rc) rc = g3i_append_rhs(ctx, rhs, ldk, a, delta, p.n0, N1, p.Np1, G3_LB, dt);
  g3i_prof_end(ctx, pr);
  if (rc) return rc;
  if (p.n0 > 0) {
    // ---- the panel against the factor that stands (profiler region `trsm`)
    rc = g3i_reset_info(ctx);
    if (rc) return rc;
    pr = g3i_prof_begin(ctx, G3_TAG_TRSM, (double)p.n0 * p.n0 * p.r);
    rc = g3i_trsm_rlt(ctx, K, p.n0, ldk, rows, p.r, ldk, dt, invd);
    g3i_prof_end(ctx, pr);
    if (rc) return rc;
  }
  // ---- the one update of corner and right-hand side, then the corner (region `potrf`); its pivot flag counts from the
  //      corner's first row
  pr = g3i_prof_begin(ctx, G3_TAG_POTRF, 2.0 * (double)(p.r + G3_LB) * p.r * p.n0 + (double)p.r * p.r * p.r / 3.0);
  if (p.n0 > 0) rc = g3i_gemm_nt(ctx, corner, ldk, rows, ldk, rows, ldk, p.r + G3_LB, p.r, p.n0, -1.0, 1.0, dt, 0);
  if (!rc) rc = g3i_potrf_tall(ctx, corner, p.r, ldk, dt, (char*)invd + (size_t)p.w_off * es, G3_LB);
  g3i_prof_end(ctx, pr);
  if (rc) return rc;
  double st[5];
  rc = g3i_logp_finish(ctx, K, N1, p.Np1, ldk, rhs, a, p.n0, dt, st);     // the host waits here for the factor
  if (rc) return rc;
  out[0] = st[0];
  out[1] = st[1];
  out[2] = st[2];
  out[5] = st[4] != 0.0 ? st[4] + (double)p.n0 : 0.0;
  return G3_OK;
}

extern "C" int g3_gp_cross_append(g3_ctx* ctx, const g3_kernel_prog* prog, const void* Xs, int64_t M, int64_t ldxs, const void* X,
                                  int64_t N0, int64_t N1, int64_t ldx, int d, const void* L, int64_t ldl, const void* invd,
                                  const void* a, g3_dtype dt, void* V, int64_t ldv, void* mu, void* ss) {
  if (!ctx || ctx->batch > 1) return -1;
  g3_dev_guard _dg(ctx);
  if (!prog) return -2;
  if (!Xs) return -3;
  if (M <= 0) return -4;
  if (!X) return -6;
  int rc = g3h_args_append(N0, N1, 7);
  if (rc) return rc;
  if (d < 1 || d > G3_MAXCOLS) return -10;
  if (ldxs < d) return -5;
  if (ldx < d) return -9;
  if (g3h_validate_prog(prog, d)) return -2;
  if (!L) return -11;
  if (dt != G3_F64 && dt != G3_F32) return -15;
  const size_t es = g3_esize(dt);
  const int64_t al = 16 / (int64_t)es;
  const G3hAppendPlan p = g3h_append_plan(N0, N1, ldl);
  if (ldl < p.Np1 || ldl % al) return -12;
  if (!invd) return -13;
  if (mu && !a) return -14;
  if (!V) return -16;
  if (ldv < p.Np1 || ldv % al) return -17;
  const int64_t Mp = g3_roundup(M, 128);
  const double es_d = (double)es;
  char* Vnew = (char*)V + (size_t)p.n0 * es;                                   // columns [n0, Np1)
  const char* Lrows = (const char*)L + (size_t)p.rows_off * es;              // L[n0:Np1, 0:n0)
  // V[:, n0:Np1) = tt_to_num(cov(Xs, X[n0:N1)))  (elliptical.py:78-79), zero in the padding
  int pr = g3i_prof_begin(ctx, G3_TAG_CROSS_GRAM, (double)(N1 - p.n0 + M) * d * es_d + (double)(N1 - p.n0) * M * es_d);
  rc = g3_gram(ctx, prog, Xs, M, ldxs, (const char*)X + (size_t)p.n0 * ldx * es, N1 - p.n0, ldx, d, dt, Vnew, ldv, Mp, p.r, G3_GRAM_SCRUB);
  g3i_prof_end(ctx, pr);
  if (rc) return rc;
  rc = g3i_reset_info(ctx);
  if (rc) return rc;
  pr = g3i_prof_begin(ctx, G3_TAG_TRSM, 2.0 * (double)M * p.n0 * p.r + (double)M * p.r * p.r);
  if (p.n0 > 0) rc = g3i_gemm_nt(ctx, Vnew, ldv, V, ldv, Lrows, ldl, Mp, p.r, p.n0, -1.0, 1.0, dt, 0);
  if (!rc)
    rc = g3i_trsm_rlt(ctx, (const char*)L + (size_t)p.corner_off * es, p.r, ldl, Vnew, Mp, ldv, dt, (const char*)invd + (size_t)p.w_off * es);
  g3i_prof_end(ctx, pr);
  if (rc) return rc;
  if (mu || ss) {
    pr = g3i_prof_begin(ctx, G3_TAG_REDUCE, 2.0 * N1 * M);
    rc = g3i_rows_dot_ss_batched(ctx, V, M, N1, ldv, a, dt, mu, ss, 1, 0, 0, 0);
    g3i_prof_end(ctx, pr);
  }
  return rc;
}
