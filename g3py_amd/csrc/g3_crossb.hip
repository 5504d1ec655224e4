// Batched posterior cross solve for a chain of hyper-parameter vectors (g3_gp_cross_batched): for every member b of one
// g3_gp_factor_batched sweep and every query point i
//     V_b = Ks_b L_b^-T,   mu[b, i] = V_b[i, :] . a_b,   ss[b, i] = |V_b[i, :]|^2
// with Ks_b = tt_to_num(K_b(Xs, X)) from the batched rectangular Gram launch.  Replaces the reference's loop of single
// predictions over the rows of a trace (g3py/bayesian/models.py:489-519 -> elliptical.py:78-97 per row).
//
// One workgroup (4 waves) owns a 32-row stripe of one member (grid.x = stripe, grid.y = member) and walks the 128-column
// blocks k of the factor with the inverses W of its diagonal blocks (as g3_potrf leaves them):
//     T      = Ks[:, k] - sum_{j < k} V[:, j] L[k, j]^T        (32 x 128, reduction over the k * 128 solved columns)
//     V[:, k] = T W_k^T                                         (W_k lower triangular: column c reduces over t <= c)
//     mu += V[:, k] . a[k],  ss += |V[:, k]|^2                  (per-lane partial sums in fp64)
// Both products are v_mfma_*_16x16x4 with the accumulators as operands; a wave owns 32 rows x 32 of the 128 columns (2 x 2
// accumulator tiles).  The A operand (the stripe's V, then T) is shared by the four waves and lives in LDS; the B operand
// (rows of L, rows of W) is different for every wave, so it goes from global memory (L2: the member's factor is re-read by
// every stripe) straight into registers, one 16-byte chunk of consecutive reduction indices per lane -- the reduction
// index may be visited in any order as long as A and B agree (g3_gemm.hip).
// Np <= 256: the stripe's V never leaves LDS (32 x (Np + pad): 66 KB for fp64 at Np = 256, two workgroups per CU) -- unless
// the caller wants it (KEEPV): then every block of V is also stored over the block of Ks it came from.
// 256 < Np <= 1024: V[:, k] overwrites Ks[:, k] -- the stripe of the cross-Gram workspace this workgroup owns and has just
// consumed -- and the update product reads it back from there (L2); T alone is staged in LDS.
// What the kernel relies on (a wave reduces over t < 32 (w + 1), more than t <= c, and padding takes part in the products, so
// a NaN in any of these places would reach valid columns through 0 * NaN): (1) the strict upper triangle of every W_k is
// zero, as the fused diagonal-block kernel and g3i_trtri_blocks write it (g3_diag.h); (2) the Gram launch writes zeros into
// the columns [N, Np) and rows [M, Mp) of Ks; (3) the rows [N, Np) of L are zero left of the diagonal (the factor of an
// identity-padded covariance, G3_GRAM_PAD_EYE).  g3_gp_factor_batched leaves (1) and (3) so, g3i_gram_rect_batched (2).
// The sums over a row are combined in a fixed order (16 lanes by xor-shuffles, then the four waves through LDS): two calls
// give the same bits.
#include "g3_internal.h"
#include "g3_mfma.h"

#define CB_BM 32          // rows of a stripe
#define CB_PAD_BYTES 64   // row pitch = columns * size + 64 B: the 64 lanes' 16-byte chunks (16 rows x 4 chunks) hit distinct banks

template <typename T, bool SPILL, bool KEEPV>
__global__ void __launch_bounds__(256, 2)
cross_solve_kernel(T* Ks, int64_t sstride, const T* L, int64_t ldl, int64_t lstride, const T* W, int64_t wstride, const T* a,
                   int64_t astride, T* mu, T* ss, int64_t ostride, int N, int Np) {
  typedef MfmaT<T> MF;
  typedef typename MF::acc_t acc_t;
  typedef typename MF::chunk_t chunk_t;
  constexpr int EPC = MF::EPC;
  constexpr int KSTEP = 4 * EPC;                       // reduction indices one step of a wave covers
  constexpr int PAD = CB_PAD_BYTES / (int)sizeof(T);
  const int b = blockIdx.y, i0 = blockIdx.x * CB_BM;
  Ks += (int64_t)b * sstride + (int64_t)i0 * Np;       // this workgroup's stripe of the member's cross-Gram (row stride Np)
  L += (int64_t)b * lstride;
  W += (int64_t)b * wstride;
  if (a) a += (int64_t)b * astride;
  extern __shared__ __attribute__((aligned(16))) char smem_cb[];
  const int P = (SPILL ? G3_LB : Np) + PAD;            // LDS row pitch (elements)
  T* Vs = reinterpret_cast<T*>(smem_cb);               // !SPILL: the stripe's V (and T in place); SPILL: T only
  double* red = reinterpret_cast<double*>(smem_cb + (size_t)CB_BM * P * sizeof(T));   // [wave][row][mu, ss]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r16 = lane & 15, q = lane >> 4;
  double pm[2][4], ps[2][4];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) { pm[rt][r] = 0.0; ps[rt][r] = 0.0; }
  const int nblk = Np / G3_LB;
  for (int k = 0; k < nblk; ++k) {
    const int c0 = k * G3_LB;
    acc_t acc[2][2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) acc[rt][ct] = acc_t{0, 0, 0, 0};
    // ---- sum_{j < k} V[:, j] L[k, j]^T over the c0 columns solved so far
    {
      const T* lrow = L + (int64_t)(c0 + 32 * w + r16) * ldl + q * EPC;
      const T* arow = SPILL ? Ks + (int64_t)r16 * Np + q * EPC : Vs + r16 * P + q * EPC;
      const int64_t astep = SPILL ? (int64_t)16 * Np : (int64_t)16 * P;
#pragma unroll 2
      for (int t0 = 0; t0 < c0; t0 += KSTEP) {
        const chunk_t a0 = *reinterpret_cast<const chunk_t*>(arow + t0);
        const chunk_t a1 = *reinterpret_cast<const chunk_t*>(arow + astep + t0);
        const chunk_t b0 = *reinterpret_cast<const chunk_t*>(lrow + t0);
        const chunk_t b1 = *reinterpret_cast<const chunk_t*>(lrow + (int64_t)16 * ldl + t0);
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
          acc[0][0] = MF::mfma(a0[e], b0[e], acc[0][0]);
          acc[0][1] = MF::mfma(a0[e], b1[e], acc[0][1]);
          acc[1][0] = MF::mfma(a1[e], b0[e], acc[1][0]);
          acc[1][1] = MF::mfma(a1[e], b1[e], acc[1][1]);
        }
      }
    }
    // ---- T = Ks[:, k] - acc, staged for the product with W_k (!SPILL: in the block's own columns of the LDS stripe)
    T* Ts = SPILL ? Vs : Vs + c0;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * rt + MF::row(lane, r), col = 32 * w + 16 * ct + r16;
          Ts[row * P + col] = Ks[(int64_t)row * Np + c0 + col] - acc[rt][ct][r];
        }
    __syncthreads();
    // ---- V[:, k] = T W_k^T; W_k is lower triangular, so this wave's columns [32 w, 32 w + 32) reduce over t < 32 (w + 1)
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) acc[rt][ct] = acc_t{0, 0, 0, 0};
    {
      const T* wrow = W + (int64_t)k * G3_LB * G3_LB + (int64_t)(32 * w + r16) * G3_LB + q * EPC;
      const T* arow = Ts + r16 * P + q * EPC;
      const int tmax = 32 * (w + 1);
#pragma unroll 2
      for (int t0 = 0; t0 < tmax; t0 += KSTEP) {
        const chunk_t a0 = *reinterpret_cast<const chunk_t*>(arow + t0);
        const chunk_t a1 = *reinterpret_cast<const chunk_t*>(arow + 16 * P + t0);
        const chunk_t b0 = *reinterpret_cast<const chunk_t*>(wrow + t0);
        const chunk_t b1 = *reinterpret_cast<const chunk_t*>(wrow + 16 * G3_LB + t0);
#pragma unroll
        for (int e = 0; e < EPC; ++e) {
          acc[0][0] = MF::mfma(a0[e], b0[e], acc[0][0]);
          acc[0][1] = MF::mfma(a0[e], b1[e], acc[0][1]);
          acc[1][0] = MF::mfma(a1[e], b0[e], acc[1][0]);
          acc[1][1] = MF::mfma(a1[e], b1[e], acc[1][1]);
        }
      }
    }
    __syncthreads();          // every wave has read T: its place may be overwritten
    // ---- keep V[:, k] for the later blocks, and its share of the row sums (columns beyond N are padding)
    const bool keep = KEEPV || k + 1 < nblk;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      const int col = 32 * w + 16 * ct + r16;
      const bool in = c0 + col < N;
      const double av = (a && in) ? (double)a[c0 + col] : 0.0;
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const T v = acc[rt][ct][r];
          const int row = 16 * rt + MF::row(lane, r);
          if (keep) {
            if (SPILL || KEEPV) Ks[(int64_t)row * Np + c0 + col] = v;
            if (!SPILL) Vs[row * P + c0 + col] = v;
          }
          if (in) {
            pm[rt][r] += (double)v * av;
            ps[rt][r] += (double)v * (double)v;
          }
        }
    }
    __syncthreads();          // V[:, k] is visible to the workgroup's next block (LDS, or its own stripe in global memory)
  }
  // ---- row sums: the 16 lanes that share a row, then the four waves, in a fixed order
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double m = pm[rt][r], s = ps[rt][r];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        m += __shfl_xor(m, o, 64);
        s += __shfl_xor(s, o, 64);
      }
      if (r16 == 0) {
        const int row = 16 * rt + MF::row(lane, r);
        red[(w * CB_BM + row) * 2] = m;
        red[(w * CB_BM + row) * 2 + 1] = s;
      }
    }
  __syncthreads();
  if (tid < CB_BM) {
    double m = 0.0, s = 0.0;
    for (int ww = 0; ww < 4; ++ww) {
      m += red[(ww * CB_BM + tid) * 2];
      s += red[(ww * CB_BM + tid) * 2 + 1];
    }
    const int64_t o = (int64_t)b * ostride + i0 + tid;
    if (mu) mu[o] = (T)m;
    if (ss) ss[o] = (T)s;
  }
}

template <typename T, bool SPILL, bool KEEPV>
static int cross_solve_launch(g3_ctx* ctx, T* Ks, int64_t sstride, const T* L, int64_t ldl, int64_t lstride, const T* W,
                              int64_t wstride, const T* a, int64_t astride, T* mu, T* ss, int64_t ostride, int64_t Mp, int64_t N,
                              int64_t Np, int batch) {
  const size_t P = (size_t)(SPILL ? G3_LB : Np) + CB_PAD_BYTES / sizeof(T);
  const size_t lds = (size_t)CB_BM * P * sizeof(T) + (size_t)4 * CB_BM * 2 * sizeof(double);
  auto kern = cross_solve_kernel<T, SPILL, KEEPV>;
  static bool attr_set[G3_MAX_DEVICES] = {};
  const int dev_slot = ctx->device & (G3_MAX_DEVICES - 1);
  if (!attr_set[dev_slot]) {
    G3_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024));
    attr_set[dev_slot] = true;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)(Mp / CB_BM), (unsigned)batch), dim3(256), lds, ctx->stream, Ks, sstride, L, ldl, lstride, W,
                     wstride, a, astride, mu, ss, ostride, (int)N, (int)Np);
  G3_LAUNCH_CHECK();
  return G3_OK;
}

// Ks: batch x Mp x Np (compact, members sstride apart), consumed (SPILL: overwritten by V; keepv: V_b is left in it whole,
// for the posterior covariance of g3_gp_draws_batched -- the sums mu / ss are formed exactly as without it).  L / W / a as g3_gp_factor_batched
// leaves them.  mu, ss (either may be null): batch x ostride.  Np a multiple of 128, <= 1024; Mp a multiple of 128.
int g3i_cross_solve_batched(g3_ctx* ctx, void* Ks, int64_t sstride, const void* L, int64_t ldl, int64_t lstride, const void* W,
                            int64_t wstride, const void* a, int64_t astride, void* mu, void* ss, int64_t ostride, int64_t Mp,
                            int64_t N, int64_t Np, int batch, g3_dtype dt, int keepv) {
  if (Np % G3_LB || Np > 1024 || Mp % CB_BM || batch < 1 || N > Np) {
    snprintf(ctx->err, sizeof(ctx->err), "batched cross solve: shape not covered (Np=%lld Mp=%lld)", (long long)Np, (long long)Mp);
    return G3_ERR_HIP;
  }
  const bool spill = Np > 2 * G3_LB;
  return g3_by_dtype(dt, [&](auto t) {
    using T = decltype(t);
#define G3_CB_LAUNCH(SP, KV)                                                                                                   \
  cross_solve_launch<T, SP, KV>(ctx, (T*)Ks, sstride, (const T*)L, ldl, lstride, (const T*)W, wstride, (const T*)a, astride, (T*)mu, \
                                (T*)ss, ostride, Mp, N, Np, batch)
    if (spill) return keepv ? G3_CB_LAUNCH(true, true) : G3_CB_LAUNCH(true, false);
    return keepv ? G3_CB_LAUNCH(false, true) : G3_CB_LAUNCH(false, false);
#undef G3_CB_LAUNCH
  });
}
