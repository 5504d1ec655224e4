// Leave-fold-out cross-validation from the Cholesky factor (g3_gp_cv).  No counterpart in the reference: its scores / Experiment
// harness (g3py/bayesian/models.py:449-469, selection.py:237-292) observes the complement, refactors and predicts once per fold.
//
// With K = L L^T the factored (noisy, possibly jittered) covariance, A = K^-1 and alpha = A delta, a fold with index set I,
// conditioned on every observation outside I, is
//     z_I | rest ~ N(z_I - r_I, A_II^-1),    r_I = A_II^-1 alpha_I,
//     log p(z_I | rest) = -1/2 alpha_I^T A_II^-1 alpha_I + 1/2 log det A_II - |I| / 2 log 2 pi.
// With A_II = C C^T and b = C^-1 alpha_I: r_I = C^-T b, the marginal variances diag(A_II^-1) are the column square-norms of
// C^-1, log det A_II = 2 sum log C_ii and the quadratic form is |b|^2 -- a fold is a small "process" with covariance A_II and
// residual alpha_I, and what g3_gp_loo_batched calls alpha and kdiag of it are r_I and the variances.  Steps:
//   1  g3_potri's sweep (Y <- L^-T, lower triangle of Kinv <- A) and alpha = Y a: g3_gp_dlogp's prologue, 2 N^3 / 3 flops;
//   2  cv_gather_kernel: every fold of a launch group becomes a member in g3_gp_factor_batched's layout, (Sp + 128) x Sp with
//      Sp = roundup(largest fold of the group, 128), in the context's workspace: the lower triangle of A[I, I] (read from the
//      lower triangle of Kinv alone), zeros above it, the identity from the fold's size on, and the right-hand-side block
//      [alpha_I; 0].  It reads s^2 / 2 elements per fold and writes (Sp + 128) Sp;
//   3  g3i_factor_members, the launches g3_gp_factor_batched queues behind its Gram launch: one workgroup per member up to
//      Sp = 256, one lock-step sweep above (a group of one fold: the single-matrix sweep), never the cooperative kernel;
//      sum_f s_f^3 / 3 flops.  Every member is factored at its padded size: the identity adds nothing to either scalar;
//   4  g3_gp_loo_batched on the members (Sp > 256: one at a time, with Y as the workspace): sum_f s_f^3 / 3 flops;
//   5  cv_scatter_kernel: resid[i_p] = r_p, pvar[i_p] = v_p (NaN for a fold whose pivot failed) over outputs cleared before.
// A group holds at most 256 MB of members.  No atomics anywhere, every sum in a fixed order: two calls give the same bits.
#include "g3_internal.h"

#define CV_GROUP_BYTES ((size_t)256 << 20)
#define CV_ROWS 64        // grid.y of the gather: rows p, p + 64, ... of a member per workgroup

// bytes of one member's slot at padded size sp: the tall matrix, its block inverses, b, r and v
static inline size_t cv_member_bytes(int64_t sp, size_t es) { return (size_t)((sp + G3_LB) * sp + sp * G3_LB + 3 * sp) * es; }

// Member blockIdx.z of a group: rows [0, Sp + 128) of its slot (leading dimension Sp), 16 bytes of a row per thread.  ptr and idx
// are the device copies of the call's fold lists, ptr advanced to the group's first fold.  Element (p, q) of the fold's block,
// q <= p < s, is Kinv[max(i_p, i_q)][min(i_p, i_q)]: consecutive q read consecutive addresses where the fold is a run of
// consecutive observations, and the right element wherever it is not.  Every element of the slot's matrix is written.
template <typename T>
__global__ void __launch_bounds__(256)
cv_gather_kernel(const T* __restrict__ Kinv, int64_t ldc, const T* __restrict__ alpha, const int32_t* __restrict__ idx,
                 const int64_t* __restrict__ ptr, T* __restrict__ M, int64_t kstride, int Sp) {
  constexpr int V = 16 / (int)sizeof(T);
  typedef T vec_t __attribute__((ext_vector_type(V)));
  const int64_t o = ptr[blockIdx.z];
  const int s = (int)(ptr[blockIdx.z + 1] - o);
  const int32_t* I = idx + o;
  T* Mf = M + (int64_t)blockIdx.z * kstride;
  const int q0 = (int)(blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (q0 >= Sp) return;
  int iq[V];
#pragma unroll
  for (int e = 0; e < V; ++e) iq[e] = q0 + e < s ? I[q0 + e] : -1;
  for (int p = blockIdx.y; p < Sp + G3_LB; p += gridDim.y) {
    vec_t v;
    if (p < s) {
      const int ip = I[p];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        T x = T(0);
        if (q0 + e <= p) {
          const int hi = ip > iq[e] ? ip : iq[e], lo = ip > iq[e] ? iq[e] : ip;
          x = Kinv[(int64_t)hi * ldc + lo];
        }
        v[e] = x;
      }
    } else if (p < Sp) {
#pragma unroll
      for (int e = 0; e < V; ++e) v[e] = q0 + e == p ? T(1) : T(0);
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) v[e] = (p == Sp && iq[e] >= 0) ? alpha[iq[e]] : T(0);
    }
    *reinterpret_cast<vec_t*>(Mf + (int64_t)p * Sp + q0) = v;
  }
}

// resid[i_p] = r_p and pvar[i_p] = v_p of member blockIdx.y (vectors Sp apart), NaN where the member's pivot flag is set
template <typename T>
__global__ void __launch_bounds__(256)
cv_scatter_kernel(const T* __restrict__ r, const T* __restrict__ v, int Sp, const int32_t* __restrict__ idx,
                  const int64_t* __restrict__ ptr, const int* __restrict__ flags, T* __restrict__ resid, T* __restrict__ pvar) {
  const int64_t o = ptr[blockIdx.y];
  const int s = (int)(ptr[blockIdx.y + 1] - o);
  const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (p >= s) return;
  const bool bad = flags[blockIdx.y] != 0;
  const T nan = (T)__builtin_nan("");
  const int64_t i = idx[o + p], m = (int64_t)blockIdx.y * Sp + p;
  resid[i] = bad ? nan : r[m];
  pvar[i] = bad ? nan : v[m];
}

static inline size_t cv_align(size_t b) { return (b + 255) & ~(size_t)255; }

static int gp_cv_impl(g3_ctx* ctx, const void* L, int64_t N, int64_t ldl, const void* invd, const void* a, g3_dtype dt, void* Y,
                      int64_t ldy, void* Kinv, int64_t ldc, void* alpha, const int32_t* idx_host, const int64_t* ptr_host, int nfold,
                      void* resid, void* pvar, double* fold_host, int* info_host, const std::vector<int>& first,
                      const std::vector<int64_t>& sps, double* hst) {
  const size_t es = g3_esize(dt);
  const int64_t Np = g3_roundup(N, G3_LB), total = ptr_host[nfold];
  const int ngroup = (int)sps.size();
  // the workspace: the fold lists, the folds' scalars and pivot flags, then the slots of the largest group
  size_t gbytes = 0;
  for (int g = 0; g < ngroup; ++g) {
    const size_t nb = (size_t)(first[g + 1] - first[g]);
    const size_t need = cv_align(nb * (size_t)((sps[g] + G3_LB) * sps[g]) * es) + cv_align(nb * (size_t)(sps[g] * G3_LB) * es) +
                        3 * cv_align(nb * (size_t)sps[g] * es);
    gbytes = need > gbytes ? need : gbytes;
  }
  const size_t o_ptr = cv_align((size_t)(total > 0 ? total : 1) * sizeof(int32_t)), o_st = o_ptr + cv_align((size_t)(nfold + 1) * sizeof(int64_t)),
               o_fl = o_st + cv_align((size_t)nfold * 4 * sizeof(double)), o_grp = o_fl + cv_align((size_t)nfold * sizeof(int));
  if (g3i_ensure_work(ctx, o_grp + gbytes) != G3_OK) {
    (void)hipGetLastError();
    return G3_ERR_NOMEM;
  }
  char* base = (char*)ctx->work;
  int32_t* d_idx = (int32_t*)base;
  int64_t* d_ptr = (int64_t*)(base + o_ptr);
  double* d_st = (double*)(base + o_st);
  int* d_fl = (int*)(base + o_fl);
  // (the host lists stay valid until the synchronisation below: this call does not return before it)
  if (total > 0) G3_HIP(hipMemcpyAsync(d_idx, idx_host, (size_t)total * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  G3_HIP(hipMemcpyAsync(d_ptr, ptr_host, (size_t)(nfold + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  int rc = g3i_kinv_alpha(ctx, 1, L, N, ldl, 0, invd, a, dt, Y, ldy, Kinv, ldc, alpha, G3_TAG_POTRF);
  if (rc) return rc;
  G3_HIP(hipMemsetAsync(resid, 0, (size_t)Np * es, ctx->stream));
  G3_HIP(hipMemsetAsync(pvar, 0, (size_t)Np * es, ctx->stream));
  for (int g = 0; g < ngroup; ++g) {
    const int f0 = first[g], nb = first[g + 1] - f0;
    const int64_t Sp = sps[g], kstride = (Sp + G3_LB) * Sp;
    char* M = base + o_grp;
    char* W = M + cv_align((size_t)nb * kstride * es);
    char* b = W + cv_align((size_t)nb * Sp * G3_LB * es);
    char* r = b + cv_align((size_t)nb * Sp * es);
    char* v = r + cv_align((size_t)nb * Sp * es);
    const unsigned threads = Sp * (int64_t)es / 16 <= 64 ? 64 : 256;
    int rec = g3i_prof_begin(ctx, G3_TAG_GRAM, (double)nb * (double)(Sp + G3_LB) * Sp * es);
    g3_by_dtype(dt, [&](auto ty) {
      using T = decltype(ty);
      const unsigned gx = (unsigned)((Sp * (int64_t)sizeof(T) / 16 + threads - 1) / threads);
      hipLaunchKernelGGL((cv_gather_kernel<T>), dim3(gx, CV_ROWS, (unsigned)nb), dim3(threads), 0, ctx->stream, (const T*)Kinv, ldc,
                         (const T*)alpha, d_idx, d_ptr + f0, (T*)M, kstride, (int)Sp);
    });
    g3i_prof_end(ctx, rec);
    G3_LAUNCH_CHECK();
    // the right-hand sides of the one-workgroup kernel: the first row of every member's block, kstride apart
    rc = g3i_factor_members(ctx, nb, Sp, Sp, M + (size_t)Sp * Sp * es, kstride, dt, M, Sp, kstride, W, b, d_st + 4 * f0, nullptr,
                            ctx->h_info + f0, d_fl + f0);
    if (rc) return rc;
    rc = g3_gp_loo_batched(ctx, nb, M, Sp, Sp, kstride, W, b, dt, Y, r, v);
    if (rc) return rc < 0 && rc > G3_ERR_HIP ? G3_ERR_HIP : rc;      // (no argument of this call's own is at fault)
    rec = g3i_prof_begin(ctx, G3_TAG_REDUCE, 2.0 * (double)(ptr_host[f0 + nb] - ptr_host[f0]));
    g3_by_dtype(dt, [&](auto ty) {
      using T = decltype(ty);
      hipLaunchKernelGGL((cv_scatter_kernel<T>), dim3((unsigned)((Sp + 255) / 256), (unsigned)nb), dim3(256), 0, ctx->stream, (const T*)r,
                         (const T*)v, (int)Sp, d_idx, d_ptr + f0, d_fl + f0, (T*)resid, (T*)pvar);
    });
    g3i_prof_end(ctx, rec);
    G3_LAUNCH_CHECK();
  }
  G3_HIP(hipMemcpyAsync(hst, d_st, (size_t)nfold * 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  G3_HIP(hipStreamSynchronize(ctx->stream));        // the one synchronisation: scalars and flags are host outputs
  const double nan = __builtin_nan("");
  for (int f = 0; f < nfold; ++f) {
    const int info = ctx->h_info[f];
    info_host[f] = info;
    fold_host[2 * f] = info ? nan : 2.0 * hst[4 * f];
    fold_host[2 * f + 1] = info ? nan : hst[4 * f + 1];
  }
  return G3_OK;
}

extern "C" int g3_gp_cv(g3_ctx* ctx, const void* L_dev, int64_t N, int64_t ldl, const void* invd_dev, const void* a_dev, g3_dtype dt,
                        void* Y_dev, int64_t ldy, void* Kinv_dev, int64_t ldc, void* alpha_dev, const int32_t* idx_host,
                        const int64_t* ptr_host, int nfold, void* resid_dev, void* pvar_dev, double* fold_host, int* info_host) {
  if (!ctx) return -1;
  g3_dev_guard _dg(ctx);
  if (dt != G3_F64 && dt != G3_F32) return -7;       // (first: the size checks below need the element size)
  const size_t es = g3_esize(dt);
  int rc = g3h_args_factor(L_dev, N, true, ldl, nullptr, invd_dev, a_dev, es, 2);
  if (!rc) rc = g3h_args_padded_out(Y_dev, ldy, N, es, 8);
  if (!rc) rc = g3h_args_padded_out(Kinv_dev, ldc, N, es, 10);
  if (rc) return rc;
  if (!alpha_dev) return -12;
  rc = g3h_args_folds(idx_host, ptr_host, nfold, N, 13);
  if (rc) return rc;
  if (!resid_dev) return -16;
  if (!pvar_dev) return -17;
  if (!fold_host) return -18;
  if (!info_host) return -19;
  double* hst = (double*)malloc((size_t)nfold * 4 * sizeof(double));
  if (!hst) return G3_ERR_NOMEM;
  try {
    std::vector<int> first;
    std::vector<int64_t> sps;
    g3h_fold_groups(ptr_host, nfold, CV_GROUP_BYTES, [&](int64_t sp) { return cv_member_bytes(sp, es); }, &first, &sps);
    rc = gp_cv_impl(ctx, L_dev, N, ldl, invd_dev, a_dev, dt, Y_dev, ldy, Kinv_dev, ldc, alpha_dev, idx_host, ptr_host, nfold, resid_dev,
                    pvar_dev, fold_host, info_host, first, sps, hst);
  } catch (...) {          // (the group lists: a few thousand integers)
    rc = G3_ERR_NOMEM;
  }
  free(hst);
  return rc;
}
