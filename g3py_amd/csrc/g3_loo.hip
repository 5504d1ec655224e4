// Leave-one-out predictions from the Cholesky factor (g3_gp_loo, g3_gp_loo_batched).
//
// With K = L L^T the factored (noisy, possibly jittered) covariance, a = L^-1 delta and Y = L^-T:
//     alpha_i = [K^-1 delta]_i = sum_j Y_ij a_j        kdiag_i = [K^-1]_ii = sum_j Y_ij^2
// and the leave-one-out predictive of observation i is N(z_i - alpha_i / kdiag_i, 1 / kdiag_i) in the latent space.  The
// reference has no counterpart: its scores / Experiment harness (g3py/bayesian/models.py:449-469) refits per hold-out split.
//   single     the Y half of g3i_potri (g3_grad.hip: the right-looking sweep without its SYRKs, n^3 / 3 flops), then ONE
//              pass over the upper triangle of Y (rows_dot_ss_kernel in its triangular mode, g3_api.hip);
//   batched    members of at most 256 padded rows: one workgroup per member, one launch, no Y.  The whole inverse of a
//              member is the two 128-block inverses the factorisation left (W_0, W_1) and V_21 = -W_1 L_21 W_0, formed on the
//              MFMA pipe 64 columns at a time; alpha and kdiag are column sums of V = L^-1 = Y^T.
#include "g3_internal.h"
#include "g3_mfma.h"

#define LOO_THREADS 512
#define LOO_HALF 64        // columns of V_21 formed per pass
#define LOO_PAD_BYTES 64   // LDS row pitch = 64 columns + 64 B (as g3_crossb.hip: the 64 lanes' reads of four rows hit distinct banks)

// What the kernel relies on: L, W and a as g3_gp_factor_batched(_fields) leaves them -- the identity padding of the factor
// beyond N (so rows [N, Np) of V are unit vectors and add nothing to a valid column).  Elements of W_k above its diagonal
// are masked, not trusted.  Sums are combined in a fixed order: two calls give the same bits.
template <typename T>
__global__ void __launch_bounds__(LOO_THREADS)
loo_small_kernel(const T* __restrict__ L, int64_t ldl, int64_t lstride, const T* __restrict__ W, int64_t wstride,
                 const T* __restrict__ a, int64_t astride, T* __restrict__ alpha, T* __restrict__ kdiag, int64_t ostride, int N, int Np) {
  typedef MfmaT<T> MF;
  typedef typename MF::acc_t acc_t;
  typedef typename MF::chunk_t chunk_t;
  constexpr int EPC = MF::EPC;
  constexpr int KSTEP = 4 * EPC;                       // reduction indices one MFMA step of a wave covers
  constexpr int P = LOO_HALF + LOO_PAD_BYTES / (int)sizeof(T);
  const int b = blockIdx.x;
  L += (int64_t)b * lstride;
  W += (int64_t)b * wstride;
  a += (int64_t)b * astride;
  extern __shared__ __attribute__((aligned(16))) char smem_loo[];
  double* dpart = reinterpret_cast<double*>(smem_loo);           // [block 2][row quarter 4][column 128][alpha, kdiag]
  double* red = dpart + 2 * 4 * G3_LB * 2;                       // [wave 8][column 128][alpha, kdiag]   (Np = 256 only)
  T* Ts = reinterpret_cast<T*>(red + 8 * G3_LB * 2);             // [128][P]: 64 columns of L_21 W_0     (Np = 256 only)
  const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, q = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nblk = Np / G3_LB;
  auto a_at = [&](int i) -> double { return i < N ? (double)a[i] : 0.0; };

  // ---- the diagonal blocks: column c of W_k over rows c .. 127, a quarter of the rows per thread
  {
    const int c = tid & (G3_LB - 1), qq = tid >> 7;
    for (int k = 0; k < nblk; ++k) {
      const T* Wk = W + (int64_t)k * G3_LB * G3_LB;
      double m = 0.0, s = 0.0;
      for (int i = 32 * qq; i < 32 * qq + 32; ++i) {
        if (i < c) continue;
        const double v = (double)Wk[i * G3_LB + c];
        m = fma(v, a_at(k * G3_LB + i), m);
        s = fma(v, v, s);
      }
      dpart[((k * 4 + qq) * G3_LB + c) * 2] = m;
      dpart[((k * 4 + qq) * G3_LB + c) * 2 + 1] = s;
    }
  }

  // ---- V_21 = -W_1 (L_21 W_0), 64 columns per pass; wave w owns rows [16 w, 16 w + 16) of both products
  if (nblk == 2) {
    const T* W1 = W + (int64_t)G3_LB * G3_LB;
    const int m_a = 16 * w + r16;                       // the row this lane feeds as the A operand
    const T* lrow = L + (int64_t)(G3_LB + m_a) * ldl + q * EPC;       // row of L_21
    const T* wrow = W1 + (int64_t)m_a * G3_LB + q * EPC;              // row of W_1
    for (int h = 0; h < G3_LB / LOO_HALF; ++h) {
      const int n0 = LOO_HALF * h;
      acc_t acc[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) acc[ct] = acc_t{0, 0, 0, 0};
      // T[m][n] = sum_t L_21[m][t] W_0[t][n]; W_0 is lower triangular: t >= n only (t0 from n0, elements above the diagonal masked)
      for (int t0 = n0; t0 < G3_LB; t0 += KSTEP) {
        const chunk_t av = *reinterpret_cast<const chunk_t*>(lrow + t0);
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
          const int t = t0 + q * EPC + e;
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) {
            const int n = n0 + 16 * ct + r16;
            const T bv = t >= n ? W[t * G3_LB + n] : T(0);
            acc[ct] = MF::mfma(av[e], bv, acc[ct]);
          }
        }
      }
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) Ts[(16 * w + MF::row(lane, r)) * P + 16 * ct + r16] = acc[ct][r];
      __syncthreads();
      // V_21[m][n] = -sum_t W_1[m][t] T[t][n]; W_1 is lower triangular: t <= m < 16 (w + 1)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) acc[ct] = acc_t{0, 0, 0, 0};
      for (int t0 = 0; t0 < 16 * (w + 1); t0 += KSTEP) {
        const chunk_t av = *reinterpret_cast<const chunk_t*>(wrow + t0);
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
          const int t = t0 + q * EPC + e;
          const T ae = t <= m_a ? av[e] : T(0);
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) acc[ct] = MF::mfma(ae, Ts[t * P + 16 * ct + r16], acc[ct]);
        }
      }
      // column sums over this wave's 16 rows: 4 registers per lane, then the 4 lanes that share a column
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        double m = 0.0, s = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double v = -(double)acc[ct][r];
          m = fma(v, a_at(G3_LB + 16 * w + MF::row(lane, r)), m);
          s = fma(v, v, s);
        }
        m += __shfl_xor(m, 16, 64); s += __shfl_xor(s, 16, 64);
        m += __shfl_xor(m, 32, 64); s += __shfl_xor(s, 32, 64);
        if (q == 0) {
          red[(w * G3_LB + n0 + 16 * ct + r16) * 2] = m;
          red[(w * G3_LB + n0 + 16 * ct + r16) * 2 + 1] = s;
        }
      }
      __syncthreads();      // every wave has read T: the next pass may overwrite it
    }
  }
  __syncthreads();
  // ---- one thread per column adds the parts in a fixed order; the padding [N, Np) gets zeros, not the identity's 1
  if (tid < Np) {
    const int k = tid >> 7, c = tid & (G3_LB - 1);
    double m = 0.0, s = 0.0;
    if (tid < N) {
      const double* d0 = dpart + (k * 4 * G3_LB + c) * 2;
      m = (d0[0] + d0[2 * G3_LB]) + (d0[4 * G3_LB] + d0[6 * G3_LB]);
      s = (d0[1] + d0[2 * G3_LB + 1]) + (d0[4 * G3_LB + 1] + d0[6 * G3_LB + 1]);
      if (k == 0 && nblk == 2)
        for (int ww = 0; ww < 8; ++ww) {
          m += red[(ww * G3_LB + c) * 2];
          s += red[(ww * G3_LB + c) * 2 + 1];
        }
    }
    alpha[(int64_t)b * ostride + tid] = (T)m;
    kdiag[(int64_t)b * ostride + tid] = (T)s;
  }
}

template <typename T>
static int loo_small_launch(g3_ctx* ctx, const T* L, int64_t ldl, int64_t lstride, const T* W, int64_t wstride, const T* a,
                            int64_t astride, T* alpha, T* kdiag, int64_t ostride, int64_t N, int64_t Np, int batch) {
  const size_t parts = (size_t)2 * 4 * G3_LB * 2 * sizeof(double);
  const size_t full = parts + (size_t)8 * G3_LB * 2 * sizeof(double) + (size_t)G3_LB * (LOO_HALF * sizeof(T) + LOO_PAD_BYTES);
  auto kern = loo_small_kernel<T>;
  static bool attr_set[G3_MAX_DEVICES] = {};
  const int dev_slot = ctx->device & (G3_MAX_DEVICES - 1);
  if (!attr_set[dev_slot]) {
    G3_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)full));
    attr_set[dev_slot] = true;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)batch), dim3(LOO_THREADS), Np == G3_LB ? parts : full, ctx->stream, L, ldl, lstride, W,
                     wstride, a, astride, alpha, kdiag, ostride, (int)N, (int)Np);
  G3_LAUNCH_CHECK();
  return G3_OK;
}

// Y <- L^-T by the sweep of g3i_potri without the K^-1 product, then alpha and kdiag in one pass over Y's triangle
static int gp_loo_single(g3_ctx* ctx, const void* L, int64_t N, int64_t ldl, const void* invd, const void* a, g3_dtype dt, void* Y,
                         int64_t ldy, void* alpha, void* kdiag) {
  const int64_t Np = g3_roundup(N, G3_LB);
  int rc = g3i_kinv_sweep(ctx, 1, L, Np, ldl, 0, invd, dt, Y, ldy, nullptr, 0, G3_TAG_TRSM, (double)N * N * N / 3.0);
  if (rc) return rc;
  const int rec = g3i_prof_begin(ctx, G3_TAG_REDUCE, (double)N * (N + 1));
  rc = g3i_rows_dot_ss_tri(ctx, Y, N, Np, ldy, a, dt, alpha, kdiag);
  g3i_prof_end(ctx, rec);
  return rc;
}

extern "C" int g3_gp_loo(g3_ctx* ctx, const void* L_dev, int64_t N, int64_t ldl, const void* invd_dev, const void* a_dev,
                         g3_dtype dt, void* Y_dev, int64_t ldy, void* alpha_dev, void* kdiag_dev) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (dt != G3_F64 && dt != G3_F32) return -7;       // (first: the size checks below need the element size)
  int rc = g3h_args_factor(L_dev, N, true, ldl, nullptr, invd_dev, a_dev, g3_esize(dt), 2);
  if (!rc) rc = g3h_args_padded_out(Y_dev, ldy, N, g3_esize(dt), 8);
  if (rc) return rc;
  if (!alpha_dev) return -10;
  if (!kdiag_dev) return -11;
  return gp_loo_single(ctx, L_dev, N, ldl, invd_dev, a_dev, dt, Y_dev, ldy, alpha_dev, kdiag_dev);
}

extern "C" int g3_gp_loo_batched(g3_ctx* ctx, int batch, const void* L_dev, int64_t N, int64_t ldl, int64_t kstride,
                                 const void* invd_dev, const void* a_dev, g3_dtype dt, void* Y_dev, void* alpha_dev,
                                 void* kdiag_dev) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (dt != G3_F64 && dt != G3_F32) return -9;       // (first: the size checks below need the element size)
  if (batch < 1 || batch > G3_MAX_BATCH) return -2;
  const size_t es = g3_esize(dt);
  const int64_t Np = g3_roundup(N, G3_LB);
  if (const int bad = g3h_args_factor(L_dev, N, true, ldl, &kstride, invd_dev, a_dev, es, 3)) return bad;
  if (Np > 2 * G3_LB && !Y_dev) return -10;          // one workspace for the members that take the single path
  if (!alpha_dev) return -11;
  if (!kdiag_dev) return -12;
  const int64_t wstride = Np * G3_LB;
  if (Np <= 2 * G3_LB) {
    const int rec = g3i_prof_begin(ctx, G3_TAG_TRSM, (double)batch * (double)N * N * N / 3.0);
    const int rc = g3_by_dtype(dt, [&](auto t) {
      using T = decltype(t);
      return loo_small_launch<T>(ctx, (const T*)L_dev, ldl, kstride, (const T*)invd_dev, wstride, (const T*)a_dev, Np, (T*)alpha_dev,
                                 (T*)kdiag_dev, Np, N, Np, batch);
    });
    g3i_prof_end(ctx, rec);
    return rc;
  }
  // larger members: one at a time through the single path, sharing the one Y workspace (stream-ordered: a member's
  // sweep joins its bulk stream before the next member's opens)
  for (int b = 0; b < batch; ++b) {
    const int rc = gp_loo_single(ctx, (const char*)L_dev + (size_t)b * kstride * es, N, ldl, (const char*)invd_dev + (size_t)b * wstride * es,
                                 (const char*)a_dev + (size_t)b * Np * es, dt, Y_dev, Np, (char*)alpha_dev + (size_t)b * Np * es,
                                 (char*)kdiag_dev + (size_t)b * Np * es);
    if (rc) return rc;
  }
  return G3_OK;
}
