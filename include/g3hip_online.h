/*
 * g3hip_online.h -- conditioning on new observations without a refit: the entry points of libg3hip.so that extend what
 * g3_gp_factor and g3_gp_cross (g3hip.h) left on the device by rows appended to the inputs.  The conventions are those of
 * g3hip.h: int status, 0 = success, negative -i = argument i is invalid, G3_ERR_HIP with the text in g3_last_error, nothing
 * thrown across the ABI, row-major matrices with leading dimensions in elements, work queued on the context's stream.
 *
 * A lower Cholesky factor is built from its leading principal submatrices: appending rows to the covariance changes no
 * existing row of L, of its block inverses or of a = L^-1 delta.  With N0 rows factored and N1 > N0 wanted, let
 *      n0 = rounddown(N0, 128),  Np1 = roundup(N1, 128),  r = Np1 - n0.
 * The factorisation is resumed at block row n0 (the rows of a ragged old last block are recomputed, which replaces their
 * identity padding); the cost is about N0^2 r + r^2 (N0 + r / 3) flops against N1^3 / 3 for g3_gp_factor at N1.  The result
 * is the factor of all N1 rows to rounding, not an approximation.
 *
 * The reference's data-dependent rules look at the whole matrix, so where one of them would have acted these entry points
 * decline and the caller refits with g3_gp_factor:
 *   - tt_to_cov (g3py/libs/tensors.py:95-98) lifts the diagonal when its minimum is not positive: checked first, on all N1
 *     points, before anything is written (out_host[6] = 1);
 *   - CholeskyRobust's jitter schedule (tensors.py:203-222) restarts from the whole matrix: a factor that was jittered or
 *     replaced by the fallback must not be appended to (precondition), and a failed pivot of the new corner is reported in
 *     out_host[5], not repaired.
 * Neither entry point accepts a context in batch mode (status -1).
 */
#ifndef G3HIP_ONLINE_H
#define G3HIP_ONLINE_H

#include "g3hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Extend the factorisation g3_gp_factor (or an earlier g3_gp_append) left in K_dev / invd_dev / a_dev for the first N0 rows
 * of X_dev, with the same prog and with tries = fallback = info = 0, to all N1 rows of X_dev.
 *   X_dev      N1 x d inputs (row stride ldx); delta_dev  N1 entries, read from n0 on
 *   K_dev      Np1 + 128 rows of ldk >= Np1 elements (ldk a multiple of 16 bytes); invd_dev  Np1 / 128 blocks of 128 x 128
 *   a_dev      Np1 entries
 * Rows [n0, Np1) of K_dev, the right-hand-side block behind them, the block inverses from n0 / 128 on and a_dev[n0:Np1) are
 * written; rows below n0, blocks below n0 / 128 and a_dev[0:n0) are not.  Nothing else is read than what the precondition
 * covers: the strict upper triangle, the new rows and the columns from Np1 on may hold anything.  Two calls on the same
 * inputs give the same bits.
 *   out_host   [0..2] log-determinant sum log L_ii, a^T a and the count of non-finite a over all N1 rows, as g3_gp_factor;
 *              [3] tries = 0, [4] fallback = 0; [5] the pivot flag of the corner, 1-based in the whole matrix (non-zero:
 *              everything from row n0 on is unspecified, refit); [6] 1 = declined because the diagonal of the N1 points has
 *              a non-positive minimum or a non-finite entry: nothing was written, refit; [7] reserved (0).
 * Synchronises the stream twice: once for the diagonal's minimum, which decides whether anything is launched, once for
 * out_host. */
int g3_gp_append(g3_ctx* ctx, const g3_kernel_prog* prog, const void* X_dev, int64_t N0, int64_t N1, int64_t ldx, int d,
                 const void* delta_dev, g3_dtype dt, void* K_dev, int64_t ldk, void* invd_dev, void* a_dev, double out_host[8]);

/* The companion of g3_gp_cross: V_dev (roundup(M, 128) rows, ldv >= Np1) holds in its columns [0, n0) what g3_gp_cross (or an
 * earlier g3_gp_cross_append) left for the same Xs_dev and prog_cross at N0, and L_dev / invd_dev / a_dev the factor of all N1
 * rows.  Columns [n0, Np1) <- tt_to_num(prog_cross(Xs, X[n0:N1))) (zero in the padding), less V[:, 0:n0) L[n0:Np1, 0:n0)^T as
 * one product, solved against the corner factor; mu_dev = V a and ss_dev = |rows of V|^2 over all N1 columns (either may be
 * NULL; a_dev may be NULL when mu_dev is).  Columns below n0 are not written.  Stream-ordered, no host synchronisation. */
int g3_gp_cross_append(g3_ctx* ctx, const g3_kernel_prog* prog_cross, const void* Xs_dev, int64_t M, int64_t ldxs,
                       const void* X_dev, int64_t N0, int64_t N1, int64_t ldx, int d, const void* L_dev, int64_t ldl,
                       const void* invd_dev, const void* a_dev, g3_dtype dt, void* V_dev, int64_t ldv, void* mu_dev, void* ss_dev);

#ifdef __cplusplus
}
#endif

#endif
