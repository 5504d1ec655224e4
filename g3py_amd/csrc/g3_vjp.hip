// Reverse mode through the Cholesky factor (g3_potrf_vjp): CholeskyRobust.grad, g3py/libs/tensors.py:224-260 (Murray 2016).
//
// Given the factor L (lower) and Lbar = d f / d L, the adjoint of the covariance in the reference's lower convention is
//     Kbar = tril(S + S^T) - diag(S),   S = L^-T Phi(tt_to_num(L^T Lbar)) L^-1,   Phi = tril with halved diagonal.
// tril(S + S^T) - diag(S) halves the diagonal of S + S^T and nothing else, so Kbar = Phi(S + S^T) and S is never symmetrised
// by a pass of its own.  Every O(n^3) step is one of the library's own: Y = L^-T by the sweep g3_gp_loo uses (g3i_potri
// without its SYRKs, n^3 / 3 flops) and four MFMA products (g3i_gemm_nt) on row-major operands padded to a multiple of 128:
//     Lt = tril(L)^T, Lbt = tril(Lbar)^T      (tril_transpose_pad_kernel; the same pass leaves the identity-padded L the
//                                               inversion reads)
//     P  = Lt Lbt^T = L^T Lbar                (lower_only, n^3), then Phi + tt_to_num in place (phi_kernel)
//     Tt = Y P^T    = (P L^-1)^T              (dense, 2 n^3: upper triangular)
//     C  = Y Tt^T + Tt Y^T = S + S^T          (two lower_only products, 2 n^3)
//     Kbar = Phi(C)                           (phi_kernel, strided into the caller's n x n)
// 5 1/3 n^3 flops in all; the dead K range of the triangular operands is not skipped.  The two kernels here are the data
// movement around the products: one read and at most two writes of a matrix each.
#include "g3_internal.h"

#define VJ_T 64          // tile edge of the transpose
#define VJ_THREADS 256

// dstT (np x np, compact) = tril(src)^T and, when dstP is given, dstP (np x np, compact) = tril(src), for src n x n with
// leading dimension ld.  Rows and columns [n, np) carry pad_diag on the diagonal and zeros elsewhere; every element of both
// outputs is written, so nothing of what the workspace held before survives.  Elements of src above its diagonal are not
// loaded (they may be NaN).  One 64 x 64 tile per workgroup: rows are read and written 64 elements at a time (256 / 512
// contiguous bytes per wave), the transposition goes through an LDS tile whose rows are padded by one element -- a column
// read of it then touches 32 distinct banks per half wave for float (bank = (c + r) mod 32) and 32 distinct bank pairs for
// double (dword 130 c + 2 r mod 64), the conflict-free patterns of ds_read_b32 / ds_read_b64.
template <typename T>
__global__ void __launch_bounds__(VJ_THREADS)
tril_transpose_pad_kernel(const T* __restrict__ src, int64_t ld, int64_t n, int64_t np, T pad_diag, T* __restrict__ dstT,
                          T* __restrict__ dstP) {
  __shared__ T tile[VJ_T][VJ_T + 1];
  const int64_t i0 = (int64_t)blockIdx.y * VJ_T, j0 = (int64_t)blockIdx.x * VJ_T;
  const int c = threadIdx.x & (VJ_T - 1), r0 = threadIdx.x >> 6;
  for (int r = r0; r < VJ_T; r += VJ_THREADS / VJ_T) {
    const int64_t i = i0 + r, j = j0 + c;
    T v = T(0);
    if (i < n) {
      if (j <= i) v = src[i * ld + j];
    } else if (i == j) {
      v = pad_diag;
    }
    tile[r][c] = v;
    if (dstP) dstP[i * np + j] = v;
  }
  __syncthreads();
  for (int r = r0; r < VJ_T; r += VJ_THREADS / VJ_T) dstT[(j0 + r) * np + i0 + c] = tile[c][r];
}

// dst[i][j] = Phi(src)[i][j] for i, j < n: src below the diagonal, half of it on the diagonal, zero above -- also in the
// tiles a lower_only product never touched.  scrub: tt_to_num first (NaN -> 0, +-Inf -> 1e10, tensors.py:90-92).  Nothing
// above the diagonal of src is read.  dst may be src (in place).
template <typename T>
__global__ void __launch_bounds__(VJ_THREADS)
phi_kernel(T* dst, int64_t ldd, const T* src, int64_t lds, int64_t n, int scrub) {
  const int64_t j = (int64_t)blockIdx.x * VJ_THREADS + threadIdx.x;
  if (j >= n) return;
  for (int64_t i = blockIdx.y; i < n; i += gridDim.y) {
    T v = T(0);
    if (j <= i) {
      v = src[i * lds + j];
      if (scrub) {
        if (v != v) v = T(0);
        else if (__builtin_isinf(v)) v = (T)1e10f;
      }
      if (j == i) v *= T(0.5);
    }
    dst[i * ldd + j] = v;
  }
}

static int phi_launch(g3_ctx* ctx, void* dst, int64_t ldd, const void* src, int64_t lds, int64_t n, g3_dtype dt, int scrub) {
  const unsigned gx = (unsigned)((n + VJ_THREADS - 1) / VJ_THREADS);
  int64_t gy = 16384 / gx;                 // enough workgroups to fill the chip, rows dealt over them
  gy = gy < 1 ? 1 : (gy > n ? n : gy);
  g3_by_dtype(dt, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((phi_kernel<T>), dim3(gx, (unsigned)gy), dim3(VJ_THREADS), 0, ctx->stream, (T*)dst, ldd, (const T*)src, lds, n,
                       scrub);
  });
  G3_LAUNCH_CHECK();
  return G3_OK;
}

static int transpose_launch(g3_ctx* ctx, const void* src, int64_t ld, int64_t n, int64_t np, double pad_diag, void* dstT, void* dstP,
                            g3_dtype dt) {
  const dim3 grid((unsigned)(np / VJ_T), (unsigned)(np / VJ_T));
  g3_by_dtype(dt, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((tril_transpose_pad_kernel<T>), grid, dim3(VJ_THREADS), 0, ctx->stream, (const T*)src, ld, n, np, (T)pad_diag,
                       (T*)dstT, (T*)dstP);
  });
  G3_LAUNCH_CHECK();
  return G3_OK;
}

// the bytes of an n x n matrix with leading dimension ld overlap those of another
static bool overlaps(const void* a, int64_t lda, const void* b, int64_t ldb, int64_t n, size_t es) {
  const char *a0 = (const char*)a, *b0 = (const char*)b;
  const char *a1 = a0 + ((size_t)(n - 1) * lda + n) * es, *b1 = b0 + ((size_t)(n - 1) * ldb + n) * es;
  return a0 < b1 && b0 < a1;
}

extern "C" int g3_potrf_vjp(g3_ctx* ctx, const void* L_dev, int64_t ldl, const void* Lbar_dev, int64_t ldb, int64_t n, g3_dtype dt,
                            void* Kbar_dev, int64_t ldk) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (dt != G3_F64 && dt != G3_F32) return -7;       // (first: the size checks below need the element size)
  if (n < 0) return -6;
  if (n == 0) return G3_OK;
  if (!L_dev) return -2;
  if (ldl < n) return -3;
  if (!Lbar_dev) return -4;
  if (ldb < n) return -5;
  if (!Kbar_dev) return -8;
  if (ldk < n) return -9;
  const size_t es = g3_esize(dt);
  if (overlaps(Kbar_dev, ldk, L_dev, ldl, n, es) || overlaps(Kbar_dev, ldk, Lbar_dev, ldb, n, es)) return -8;
  const int64_t np = g3_roundup(n, G3_LB);
  // four np x np matrices, each reused once its first content is dead:
  //   M0: identity-padded L -> P        M1: Lt -> Tt        M2: Lbt -> C        M3: Y
  const size_t mat = (size_t)np * np * es;
  if (g3i_ensure_work(ctx, 4 * mat) != G3_OK) {
    (void)hipGetLastError();
    return G3_ERR_NOMEM;
  }
  char* M0 = (char*)ctx->work;
  char *M1 = M0 + mat, *M2 = M1 + mat, *M3 = M2 + mat;
  int rc = g3i_ensure_invd(ctx, np, dt);
  if (rc) return rc;
  rc = g3i_reset_info(ctx);              // the products and the sweep are no-ops behind a failed pivot's flag
  if (rc) return rc;
  rc = transpose_launch(ctx, L_dev, ldl, n, np, 1.0, M1, M0, dt);
  if (rc) return rc;
  rc = transpose_launch(ctx, Lbar_dev, ldb, n, np, 0.0, M2, nullptr, dt);
  if (rc) return rc;
  // Y = L^-T (upper triangular; g3i_potri memsets Y, so left of the diagonal it holds zeros the dense products may read)
  rc = g3i_trtri_blocks(ctx, M0, np, np, dt, ctx->invd);
  if (rc) return rc;
  int rec = g3i_prof_begin(ctx, G3_TAG_TRSM, (double)n * n * n / 3.0);
  rc = g3i_potri(ctx, M0, np, np, ctx->invd, dt, M3, np, nullptr, 0);
  g3i_prof_end(ctx, rec);
  if (rc) return rc;
  rc = g3i_gemm_nt(ctx, M0, np, M1, np, M2, np, np, np, np, 1.0, 0.0, dt, 1);       // P = L^T Lbar, lower
  if (rc) return rc;
  rc = phi_launch(ctx, M0, np, M0, np, np, dt, 1);
  if (rc) return rc;
  rc = g3i_gemm_nt(ctx, M1, np, M3, np, M0, np, np, np, np, 1.0, 0.0, dt, 0);       // Tt = Y P^T
  if (rc) return rc;
  rc = g3i_gemm_nt(ctx, M2, np, M3, np, M1, np, np, np, np, 1.0, 0.0, dt, 1);       // C = Y Tt^T = S, lower
  if (rc) return rc;
  rc = g3i_gemm_nt(ctx, M2, np, M1, np, M3, np, np, np, np, 1.0, 1.0, dt, 1);       // C += Tt Y^T = S^T, lower
  if (rc) return rc;
  return phi_launch(ctx, Kbar_dev, ldk, M2, np, n, dt, 0);
}
