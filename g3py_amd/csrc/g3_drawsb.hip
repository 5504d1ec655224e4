// Joint posterior draws for a chain of hyper-parameter vectors (g3_gp_draws_batched): the two kernels that the reference's
// `particles` (g3py/bayesian/models.py:521-543 -> gaussian.py:89-97 per row of a trace) needs beyond the batched
// factorisation, cross solve and MFMA product that exist already.
//
// 1. robust_factor_kernel -- CholeskyRobust.perform (g3py/libs/tensors.py:197-222) for `batch` independent matrices of at most
//    256 rows, the whole jitter schedule on the device.  A posterior covariance of dense noise-free query points is singular
//    to rounding, so most members of a chain may need a retry: sending those back to the host one by one (what
//    g3_gp_factor_batched does for the rare observation covariance that fails) would undo the batching.
//    One workgroup (8 waves) per member at a time; a workgroup
//      * writes lower(K_b) + add * I, identity padded, into the member's slot of L and factors it there with the wave
//        programs of the single call (g3_diag.h: diag128_wave / potrf256_wave, as small_factor_kernel);
//      * ONE lane reads the pivot flag and publishes it through an LDS word behind a barrier; every wave branches on that
//        copy.  The wave programs hold workgroup barriers, so the branch must be uniform over the workgroup: a flag read per
//        lane straight from memory is not guaranteed to be (VERDICT.md on coop_factor_kernel);
//      * on failure takes the diagonal mean / minimum and the non-finite count of the lower triangle from K_b (combined by
//        the functions of g3_reduce.h that g3_diag_stats uses) and walks G3hJitter -- the one definition
//        of the schedule's arithmetic, shared with the host callers -- until an attempt passes or `maxtries` are used up,
//        then writes the 1e-10 * I fallback;
//      * leaves tries / fallback / jitter per member in a device array: the batch comes back in one copy.
//    The block inverses the wave programs write are not wanted here: they go to a scratch slot per WORKGROUP (the grid is
//    capped, workgroups stride over the members), not per member.
// 2. draws_kernel -- out[b] = loc[b] (+ mu[b]) + Lp_b Z[b] with the member in the grid.  One draw per row (S = 1) is the
//    common case, a 128 x 128-tile GEMM per member would be all padding: one wave owns a row of Lp_b, reads it once,
//    coalesced, for up to DR_SC draws at a time, and adds the 64 partial sums in a fixed order.
#include "g3_internal.h"
#include "g3_mfma.h"
#include "g3_diag.h"

// Register budget: the wave programs were written to fit 128 VGPRs next to a bulk GEMM; inside the schedule's loop the
// compiler does not manage that without kilobytes of scratch per lane (the loop keeps more alive across them), and the
// schedule must not be traded for occupancy.  Two waves per SIMD -- ONE workgroup per CU -- is what the kernel asks for.
#ifndef RB_WAVES
#define RB_WAVES 2
#endif
#define RB_MAX_WGS 256   // one resident workgroup per CU; also bounds the scratch for the unwanted block inverses

// The schedule's state of the member a workgroup is working on.  It lives in LDS, written by thread 0 between barriers and
// read by everyone at the top of an attempt: nothing but kernel arguments is live across the factorisation, whose wave
// programs need the whole register budget.
struct RobustState {
  double dK, lift;        // G3hJitter
  double red[3][8];       // per wave: diagonal sum, diagonal minimum, non-finite count of the lower triangle
  int t;                  // -1: the plain attempt; >= 0: retry t of the schedule
  int finite, info;
};

// The whole program of one wave (block row W of the factorisation): the member loop and the schedule sit INSIDE the wave's
// program, which the kernel selects once -- with the eight programs selected inside the loop instead, the register allocator
// spills kilobytes per lane across the merged control flow.  Every barrier below is reached by all eight waves alike: the
// branches around them depend on LDS words and kernel arguments only.
template <typename T, bool P256, int W>
__device__ __forceinline__ void robust_program(const T* K, int64_t ldk, int64_t kstride, T* Lall, int64_t ldl, int64_t lstride, T* Wg,
                                               int* info, double* res, int batch, int n, int np, int maxtries, DiagLds<T>& S,
                                               RobustState& st, int wv) {
  for (int b = blockIdx.x; b < batch; b += gridDim.x) {
    // the thread's indices are re-materialised per member (an empty asm the optimiser cannot see through): otherwise what is
    // derived from them -- per-lane addresses of the copy loops and of the wave program -- is hoisted out of the member loop
    // and of the schedule's loop and held in registers across the factorisation, which needs the whole budget
    // (rebuilt from the wave's index, a scalar, and the lane count: threadIdx.x itself need not stay in a register either)
    int tid;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(tid));
    tid += 64 * wv;
    const int lane = tid & 63;
    const T* Kb = K + (int64_t)b * kstride;
    T* L = Lall + (int64_t)b * lstride;
    if (tid == 0) st.t = -1;          // (dK, lift and finite are written before they are first used: t >= 0)
    __syncthreads();
    bool ok = false;
    for (;;) {
      const int t = st.t;
      G3hJitter jit(0.0, 1.0);
      jit.dK = st.dK;
      jit.lift = st.lift;
      int failed = 1;
      if (t < 0 || (st.finite && jit.usable())) {
        const T add = t < 0 ? T(0) : (T)jit.value();
        // L <- lower(K_b) + add I, zero above the diagonal, identity in the padding (copy_lower_pad_kernel)
        for (int idx = tid; idx < np * np; idx += 512) {
          const int i = idx / np, j = idx - i * np;
          T v = T(0);
          if (i < n && j < n) {
            if (j <= i) v = Kb[(int64_t)i * ldk + j];
            if (j == i) v += add;
          } else if (i == j) {
            v = T(1);
          }
          L[(int64_t)i * ldl + j] = v;
        }
        __threadfence_block();
        __syncthreads();
        // the operands are re-materialised per attempt (an empty asm the optimiser cannot see through): otherwise the
        // per-lane addresses of the wave program are hoisted out of the schedule's loop and held in registers across it
        T* Lq = L;
        T* Wq = Wg;
        int64_t ldq = ldl;
        int* infoq = info;
        int laneq = lane;
        asm volatile("" : "+s"(Lq), "+s"(Wq), "+s"(ldq), "+s"(infoq), "+v"(laneq));
        if (P256) potrf256_wave<T, W>(Lq, ldq, Wq, infoq, 0, S, laneq);
        else diag128_wave<T, true, W>(Lq, ldq, Wq, (int64_t)G3_LB, infoq, 0, S, laneq);
        __threadfence_block();
        __syncthreads();                               // every wave's pivots are in: the flag is final
        if (tid == 0) {                                // ONE lane reads it (and clears it for the next attempt) ...
          st.info = __hip_atomic_load(info, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(info, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        failed = st.info;                              // ... and every wave branches on the workgroup's one copy
      }
      if (failed == 0) {
        ok = true;
        break;
      }
      __syncthreads();                                 // the state has been read by all: thread 0 may advance it
      if (t < 0) {
        // the schedule's inputs, from K_b: n <= 256 < 512, so a thread holds at most one diagonal entry
        double sm = 0.0, mn = 1.0 / 0.0, cnt = 0.0;
        if (tid < n) { sm = (double)Kb[(int64_t)tid * ldk + tid]; mn = sm; }
        for (int idx = tid; idx < n * n; idx += 512) {
          const int i = idx / n, j = idx - i * n;
          if (j <= i && !(fabs((double)Kb[(int64_t)i * ldk + j]) <= 1.7976931348623157e308)) cnt += 1.0;
        }
        sm = wave_sum(sm); mn = wave_min(mn); cnt = wave_sum(cnt);
        if (lane == 0) { st.red[0][wv] = sm; st.red[1][wv] = mn; st.red[2][wv] = cnt; }
        __syncthreads();
        if (tid == 0) {
          const double a = waves_min<8>(st.red[1]), e = waves_sum<8>(st.red[2]);
          const double mean = waves_sum<8>(st.red[0]) / (double)n;
          const G3hJitter first(mean, a);
          st.dK = first.dK;
          st.lift = first.lift;
          st.finite = G3hJitter::input_finite(e, mean) ? 1 : 0;
        }
      } else if (tid == 0) {
        jit.next();
        st.dK = jit.dK;
      }
      const bool more = t + 1 < maxtries;
      if (tid == 0) st.t = t + 1;
      __syncthreads();
      if (!more) break;
    }
    if (ok) {
      for (int i = n + tid; i < np; i += 512) L[(int64_t)i * ldl + i] = T(0);     // the padding's identity: zero, as the single call leaves it
    } else {
      for (int idx = tid; idx < np * np; idx += 512) {
        const int i = idx / np, j = idx - i * np;
        L[(int64_t)i * ldl + j] = (i == j && i < n) ? (T)1e-10f : T(0);
      }
    }
    if (tid == 0) {
      res[3 * b] = (double)(ok ? st.t + 1 : st.t);     // retries begun: t + 1 when attempt t passed, maxtries when none did
      res[3 * b + 1] = ok ? 0.0 : 1.0;
      res[3 * b + 2] = (ok && st.t >= 0) ? st.lift + st.dK : 0.0;
    }
    __syncthreads();
  }
}

template <typename T, bool P256>      // P256: 256 padded rows (the fused 256-wide factorisation), else 128
__global__ void __launch_bounds__(512, RB_WAVES)
robust_factor_kernel(const T* K, int64_t ldk, int64_t kstride, T* Lall, int64_t ldl, int64_t lstride, T* Wscr, int* info_all,
                     double* res, int batch, int n, int np, int maxtries) {
  __shared__ DiagLds<T> S;
  __shared__ RobustState st;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int w = wv < 4 ? wv : 11 - wv;                 // block rows dealt 0 1 2 3 | 7 6 5 4 over the SIMDs (potrf256_kernel)
  int* info = info_all + blockIdx.x;                   // zero on entry, zero again on exit
  T* Wg = Wscr + (int64_t)blockIdx.x * np * G3_LB;
#define G3_RB_CASE(WW) \
  robust_program<T, P256, WW>(K, ldk, kstride, Lall, ldl, lstride, Wg, info, res, batch, n, np, maxtries, S, st, wv)
  switch (w) {
    case 0: G3_RB_CASE(0); break;
    case 1: G3_RB_CASE(1); break;
    case 2: G3_RB_CASE(2); break;
    case 3: G3_RB_CASE(3); break;
    case 4: G3_RB_CASE(4); break;
    case 5: G3_RB_CASE(5); break;
    case 6: G3_RB_CASE(6); break;
    default: G3_RB_CASE(7); break;
  }
#undef G3_RB_CASE
}

size_t g3i_robust_scratch_bytes(int batch, int64_t n, g3_dtype dt) {
  const int64_t np = g3_roundup(n, G3_LB);
  return (size_t)(batch < RB_MAX_WGS ? batch : RB_MAX_WGS) * np * G3_LB * g3_esize(dt);
}

// n <= 256.  wscr: g3i_robust_scratch_bytes of device memory; res_dev: batch x [tries, fallback, jitter] doubles.
// Stream-ordered, no host synchronisation; the context's pivot flags are zero before and after.
int g3i_potrf_robust_batched(g3_ctx* ctx, const void* K, int64_t ldk, int64_t kstride, void* L, int64_t ldl, int64_t lstride, int batch,
                             int64_t n, g3_dtype dt, int maxtries, void* wscr, double* res_dev) {
  const int64_t np = g3_roundup(n, G3_LB);
  if (n < 1 || np > 2 * G3_LB || batch < 1 || ldk < n || ldl < np || lstride < np * ldl) {
    snprintf(ctx->err, sizeof(ctx->err), "batched robust factor: shape not covered (n=%lld ldk=%lld ldl=%lld)", (long long)n,
             (long long)ldk, (long long)ldl);
    return G3_ERR_HIP;
  }
  const unsigned grid = (unsigned)(batch < RB_MAX_WGS ? batch : RB_MAX_WGS);
  G3_HIP(hipMemsetAsync(ctx->d_info, 0, sizeof(int) * grid, ctx->stream));      // a flag per workgroup; each leaves its own zero again
  ctx->info_clean = false;
  g3_by_dtype(dt, [&](auto t) {
    using T = decltype(t);
#define G3_RB_LAUNCH(PP)                                                                                                          \
  hipLaunchKernelGGL((robust_factor_kernel<T, PP>), dim3(grid), dim3(512), 0, ctx->stream, (const T*)K, ldk, kstride, (T*)L, ldl, \
                     lstride, (T*)wscr, ctx->d_info, res_dev, batch, (int)n, (int)np, maxtries)
    if (np == 2 * G3_LB) G3_RB_LAUNCH(true);
    else G3_RB_LAUNCH(false);
#undef G3_RB_LAUNCH
  });
  G3_LAUNCH_CHECK();
  return G3_OK;
}

extern "C" int g3_potrf_robust_batched(g3_ctx* ctx, const void* K_dev, int64_t ldk, int64_t kstride, void* L_dev, int64_t ldl,
                                       int64_t lstride, int batch, int64_t n, g3_dtype dt, int maxtries, int* tries_host,
                                       int* fallback_host, double* jitter_host) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (!K_dev) return -2;
  if (n < 0) return -9;
  const int64_t np = g3_roundup(n, G3_LB);
  const size_t es = g3_esize(dt);
  if (ldk < n) return -3;
  if (kstride < n * ldk) return -4;
  if (!L_dev) return -5;
  if (ldl < np) return -6;
  if (lstride < np * ldl) return -7;
  if (batch < 1 || batch > G3_MAX_BATCH) return -8;
  if (dt != G3_F64 && dt != G3_F32) return -10;
  if (maxtries < 0) return -11;
  if (n == 0) {
    for (int b = 0; b < batch; ++b) {
      if (tries_host) tries_host[b] = 0;
      if (fallback_host) fallback_host[b] = 0;
      if (jitter_host) jitter_host[b] = 0.0;
    }
    return G3_OK;
  }
  if (np > 2 * G3_LB) {
    // larger members: the host-driven schedule of the single call, one member after the other
    for (int b = 0; b < batch; ++b) {
      char* Lb = (char*)L_dev + (size_t)b * lstride * es;
      G3_HIP(hipMemset2DAsync(Lb, (size_t)ldl * es, 0, (size_t)np * es, (size_t)np, ctx->stream));
      int rc = g3_potrf_robust(ctx, (const char*)K_dev + (size_t)b * kstride * es, ldk, Lb, ldl, n, dt, maxtries,
                               tries_host ? tries_host + b : nullptr, fallback_host ? fallback_host + b : nullptr,
                               jitter_host ? jitter_host + b : nullptr);
      if (rc) return rc;
    }
    return G3_OK;
  }
  const size_t wbytes = (g3i_robust_scratch_bytes(batch, n, dt) + 255) & ~(size_t)255;
  int rc = g3i_ensure_work(ctx, wbytes + (size_t)batch * 3 * sizeof(double));
  if (rc) return rc;
  double* res = (double*)((char*)ctx->work + wbytes);
  rc = g3i_potrf_robust_batched(ctx, K_dev, ldk, kstride, L_dev, ldl, lstride, batch, n, dt, maxtries, ctx->work, res);
  if (rc) return rc;
  double* h = (double*)malloc((size_t)batch * 3 * sizeof(double));
  if (!h) return G3_ERR_NOMEM;
  hipError_t e = hipMemcpyAsync(h, res, (size_t)batch * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    free(h);
    snprintf(ctx->err, sizeof(ctx->err), "g3_potrf_robust_batched: %s", hipGetErrorString(e));
    return G3_ERR_HIP;
  }
  for (int b = 0; b < batch; ++b) {
    if (tries_host) tries_host[b] = (int)h[3 * b];
    if (fallback_host) fallback_host[b] = (int)h[3 * b + 1];
    if (jitter_host) jitter_host[b] = h[3 * b + 2];
  }
  free(h);
  return G3_OK;
}

// ---------------------------------------------------------------------------------------
#define DR_SC 4           // draws a wave carries per pass over its row of Lp
template <typename T>
__global__ void __launch_bounds__(256)
draws_kernel(const T* __restrict__ Lp, int64_t ldl, int64_t lstride, const T* __restrict__ loc, const T* __restrict__ mu,
             int64_t mustride, const T* __restrict__ Z, T* __restrict__ out, int M, int S) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (int)(threadIdx.x >> 6);        // a wave per row of the member's factor; no barriers below
  if (i >= M) return;
  const T* lrow = Lp + (int64_t)b * lstride + (int64_t)i * ldl;
  const T* Zb = Z + (int64_t)b * M * S;
  T base = loc[(int64_t)b * M + i];
  if (mu) base += mu[(int64_t)b * mustride + i];
  for (int s0 = 0; s0 < S; s0 += DR_SC) {
    double acc[DR_SC];
#pragma unroll
    for (int c = 0; c < DR_SC; ++c) acc[c] = 0.0;
    for (int j = lane; j <= i; j += 64) {               // Lp is lower triangular
      const double l = (double)lrow[j];
      const T* z = Zb + (int64_t)j * S + s0;
#pragma unroll
      for (int c = 0; c < DR_SC; ++c)
        if (s0 + c < S) acc[c] = fma(l, (double)z[c], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < DR_SC; ++c) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o, 64);
      if (lane == 0 && s0 + c < S) out[((int64_t)b * M + i) * S + s0 + c] = base + (T)acc[c];
    }
  }
}

// Lp: batch factors lstride apart (lower, M x M valid); loc: batch x M; mu: batch x mustride or null; Z, out: batch x M x S
int g3i_draws_batched(g3_ctx* ctx, const void* Lp, int64_t ldl, int64_t lstride, const void* loc, const void* mu, int64_t mustride,
                      const void* Z, void* out, int64_t M, int64_t S, int batch, g3_dtype dt) {
  const dim3 grid((unsigned)((M + 3) / 4), (unsigned)batch);
  g3_by_dtype(dt, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((draws_kernel<T>), grid, dim3(256), 0, ctx->stream, (const T*)Lp, ldl, lstride, (const T*)loc, (const T*)mu,
                       mustride, (const T*)Z, (T*)out, (int)M, (int)S);
  });
  G3_LAUNCH_CHECK();
  return G3_OK;
}
