// Derivative of a kernel expression (g3_kernel_prog: shift + sum of products of leaves) with respect to the columns of its
// FIRST argument, for ONE pair of points, as device functions: what the pair kernel and the diagonal kernel of
// g3_cross_dx.hip share.  The reference gets these from one tt.grad(..., space) through its Theano graph; the leaf formulas
// differentiated here are g3_kernel_eval.h's (kernels.py:293-487, metrics.py:30-35,54-56,89-131).  Everything is in fp64.
//
// With dx = xi_c - xj_c, rate r_c, frequency f_c and column c among the leaf's dims (any other column: 0):
//   SE, MAT32, MAT52, RQ   D = sum 1/2 r^2 dx^2:  dk/dD * r_c^2 dx_c, dk/dD as leaf_grad (g3_grad.hip) has it: SE -k,
//                          MAT32 -3/2 var e^-s, MAT52 -5/6 (1 + s) var e^-s, RQ -var (1 + D/a)^(-a-1) -- finite at D = 0
//   OU     -k r_c sign(dx_c), sign(0) = 0
//   COS    -2 pi f_c var sin(2 pi f_c dx_c) prod_{k != c} cos(2 pi f_k dx_k)
//   SIN    k 2 pi f_c r_c sin(2 pi f_c dx_c)                      (positive exponent, as the value is written)
//   SINC   th = 2 pi^2 f dx:  var (cos th_c - sinc th_c) / dx_c prod_{k != c} sinc th_k, 0 at dx_c = 0
//   SM     var e^(-2 pi^2 sum r^2 dx^2) [-4 pi^2 r_c^2 dx_c prod_k cos t_k - 2 pi f_c sin t_c prod_{k != c} cos t_k], t = 2 pi f dx
//   DOT    m = bias + sum r^2 xi xj:  var p m^(p-1) r_c^2 xj_c, m^0 = 1
//   NN     u = 2 m12 / (a b), a = 1 + 2 m11, b = 1 + 2 m22:  var / sqrt(1 - u^2) [2 r_c^2 xj_c / (a b) - u 4 r_c^2 xi_c / a]
//   BW     var I_c prod_{k != c} min(xi_k, xj_k), I_c = 1 for xi_c < xj_c, 1/2 at a tie (which makes the doubled partial exact
//          on the diagonal), 0 otherwise
//   NOISE, WN, VAR   0
// Every leaf is symmetric in its arguments, so d k(x, x) / d x_c = 2 d1_c k(x, x')|x' = x: the diagonal kernel is the pair
// function at xj = xi, doubled.
#pragma once
#include <hip/hip_runtime.h>

#include "g3hip.h"

#define G3DX_PI 3.14159265358979323846

__device__ __forceinline__ bool dx_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN too

__device__ __forceinline__ double dx_dot_metric(const g3_leaf& lf, const double* xi, const double* xj) {
  double m = lf.alpha;
  for (int k = 0; k < lf.ndims; ++k) m += (xi[lf.dims[k]] * xj[lf.dims[k]]) * (lf.rate[k] * lf.rate[k]);
  return m;
}

// Value of leaf `lf` (variance included) for the pair (xi, xj) and, with D1, emit(c, d leaf / d xi_c) for every column the
// leaf uses.  diag: the square-case diagonal (xj is xi; NOISE and WN are their variance there and 0 / the tie count off it).
// A leaf whose value is not finite emits zeros: tt_to_num replaces such a covariance by a constant.
template <bool D1, typename Emit>
__device__ __forceinline__ double leaf_d1(const g3_leaf& lf, const double* xi, const double* xj, bool diag, const Emit& emit) {
  const int nd = lf.ndims;
  const double var = lf.var;
  switch (lf.kind) {
    case G3_K_NOISE:
      return diag ? var : 0.0;
    case G3_K_WN: {
      if (diag) return var;
      double cnt = 0.0;
      for (int k = 0; k < nd; ++k) cnt += (xi[lf.dims[k]] - xj[lf.dims[k]] == 0.0) ? 1.0 : 0.0;
      return var * cnt;
    }
    case G3_K_SE:
    case G3_K_MAT32:
    case G3_K_MAT52:
    case G3_K_RQ: {
      double D = 0.0;
      for (int k = 0; k < nd; ++k) {
        const double dx = xi[lf.dims[k]] - xj[lf.dims[k]];
        D += (dx * dx) * (0.5 * lf.rate[k] * lf.rate[k]);
      }
      double kv, dkdD;
      if (lf.kind == G3_K_SE) {
        kv = exp(-D); dkdD = -kv;
      } else if (lf.kind == G3_K_MAT32) {
        const double s = sqrt(3.0 * D), e = exp(-s);
        kv = (1.0 + s) * e; dkdD = -1.5 * e;
      } else if (lf.kind == G3_K_MAT52) {
        const double s = sqrt(5.0 * D), e = exp(-s);
        kv = (1.0 + s + 5.0 * D / 3.0) * e; dkdD = -(5.0 / 6.0) * (1.0 + s) * e;
      } else {
        const double al = lf.alpha, b = 1.0 + D / al;
        kv = pow(b, -al); dkdD = -kv / b;
      }
      const double v = var * kv;
      if (D1) {
        const double c0 = dx_finite(v) ? var * dkdD : 0.0;
        for (int k = 0; k < nd; ++k) {
          const double dx = xi[lf.dims[k]] - xj[lf.dims[k]];
          emit(lf.dims[k], c0 * (lf.rate[k] * lf.rate[k]) * dx);
        }
      }
      return v;
    }
    case G3_K_OU: {
      double D = 0.0;
      for (int k = 0; k < nd; ++k) D += fabs(xi[lf.dims[k]] - xj[lf.dims[k]]) * lf.rate[k];
      const double v = var * exp(-D);
      if (D1) {
        const double c0 = dx_finite(v) ? -v : 0.0;
        for (int k = 0; k < nd; ++k) {
          const double dx = xi[lf.dims[k]] - xj[lf.dims[k]];
          emit(lf.dims[k], dx > 0.0 ? c0 * lf.rate[k] : dx < 0.0 ? -c0 * lf.rate[k] : dx == 0.0 ? 0.0 : dx);
        }
      }
      return v;
    }
    case G3_K_SIN: {
      double s = 0.0;
      for (int k = 0; k < nd; ++k) {
        const double q = sin(G3DX_PI * (xi[lf.dims[k]] - xj[lf.dims[k]]) * lf.freq[k]);
        s += (q * q) * lf.rate[k];
      }
      const double v = var * exp(2.0 * s);
      if (D1) {
        const double c0 = dx_finite(v) ? v * (2.0 * G3DX_PI) : 0.0;
        for (int k = 0; k < nd; ++k) {
          const double dx = xi[lf.dims[k]] - xj[lf.dims[k]];
          emit(lf.dims[k], c0 * lf.freq[k] * lf.rate[k] * sin(2.0 * G3DX_PI * dx * lf.freq[k]));
        }
      }
      return v;
    }
    case G3_K_COS:
    case G3_K_SINC:
    case G3_K_SM: {
      // value = var * env * prod_k f_k ;  d / d xi_m = var * (env' f_m + env f'_m) * prod_{k != m} f_k
      const bool sinc = lf.kind == G3_K_SINC, sm = lf.kind == G3_K_SM;
      const double cs = sinc ? 2.0 * G3DX_PI * G3DX_PI : 2.0 * G3DX_PI;
      double p = 1.0, s = 0.0;
      for (int k = 0; k < nd; ++k) {
        const double dx = xi[lf.dims[k]] - xj[lf.dims[k]];
        const double th = cs * dx * lf.freq[k];
        p *= sinc ? (dx != 0.0 ? sin(th) / th : 1.0) : cos(th);
        s += (dx * dx) * (lf.rate[k] * lf.rate[k]);
      }
      const double env = sm ? exp(-2.0 * G3DX_PI * G3DX_PI * s) : 1.0;
      const double v = var * (env * p);
      if (D1) {
        const double c0 = dx_finite(v) ? var * env : 0.0;
        for (int m = 0; m < nd; ++m) {
          const double dx = xi[lf.dims[m]] - xj[lf.dims[m]];
          const double th = cs * dx * lf.freq[m];
          double fm, dfm;
          if (sinc) {
            fm = dx != 0.0 ? sin(th) / th : 1.0;
            dfm = dx != 0.0 ? (cos(th) - fm) / dx : 0.0;
          } else {
            fm = cos(th);
            dfm = -cs * lf.freq[m] * sin(th);
          }
          // the other factors: by division where that is exact to rounding, else multiplied out (a factor may be 0)
          double others;
          if (fm != 0.0) {
            others = p / fm;
          } else {
            others = 1.0;
            for (int k = 0; k < nd; ++k) {
              if (k == m) continue;
              const double dk = xi[lf.dims[k]] - xj[lf.dims[k]];
              const double tk = cs * dk * lf.freq[k];
              others *= sinc ? (dk != 0.0 ? sin(tk) / tk : 1.0) : cos(tk);
            }
          }
          double g = dfm * others;
          if (sm) g += (-4.0 * G3DX_PI * G3DX_PI) * (lf.rate[m] * lf.rate[m]) * dx * p;
          emit(lf.dims[m], c0 * g);
        }
      }
      return v;
    }
    case G3_K_DOT: {
      const double m = dx_dot_metric(lf, xi, xj);
      const int p = (int)lf.freq[0];
      double mp1 = 1.0;
      for (int q = 1; q < p; ++q) mp1 *= m;
      const double v = var * (mp1 * m);
      if (D1) {
        const double c0 = dx_finite(v) ? var * (double)p * mp1 : 0.0;
        for (int k = 0; k < nd; ++k) emit(lf.dims[k], c0 * (lf.rate[k] * lf.rate[k]) * xj[lf.dims[k]]);
      }
      return v;
    }
    case G3_K_NN: {
      const double m12 = dx_dot_metric(lf, xi, xj);
      const double a = 1.0 + 2.0 * dx_dot_metric(lf, xi, xi), b = 1.0 + 2.0 * dx_dot_metric(lf, xj, xj);
      const double u = 2.0 * m12 / (a * b);
      const double v = var * asin(u);
      if (D1) {
        const double c0 = dx_finite(v) ? var / sqrt(1.0 - u * u) : 0.0;
        for (int k = 0; k < nd; ++k) {
          const double r2 = lf.rate[k] * lf.rate[k];
          emit(lf.dims[k], c0 * (2.0 * r2 * xj[lf.dims[k]] / (a * b) - u * (4.0 * r2 * xi[lf.dims[k]]) / a));
        }
      }
      return v;
    }
    case G3_K_BW: {
      double p = 1.0;
      for (int k = 0; k < nd; ++k) p *= fmin(xi[lf.dims[k]], xj[lf.dims[k]]);
      const double v = var * p;
      if (D1) {
        const double c0 = dx_finite(v) ? var : 0.0;
        for (int m = 0; m < nd; ++m) {
          const double a = xi[lf.dims[m]], b = xj[lf.dims[m]];
          const double ind = a < b ? 1.0 : a == b ? 0.5 : 0.0;
          const double fm = fmin(a, b);
          double others;
          if (fm != 0.0) {
            others = p / fm;
          } else {
            others = 1.0;
            for (int k = 0; k < nd; ++k)
              if (k != m) others *= fmin(xi[lf.dims[k]], xj[lf.dims[k]]);
          }
          emit(lf.dims[m], c0 * ind * others);
        }
      }
      return v;
    }
    case G3_K_VAR:
      return var;
    default:
      return 0.0;
  }
}

struct DxNoEmit {
  __device__ __forceinline__ void operator()(int, double) const {}
};

// qconst[l] = d prog / d (leaf l) when every product has one factor: the sum of the coefficients of the products that are
// leaf l.  Returns whether some product has more factors (the pair function then needs the leaves' values).
__device__ __forceinline__ bool prog_qconst(const g3_kernel_prog& sp, double* qconst) {
  bool multi = false;
  for (int p = 0; p < sp.nprod; ++p) multi |= sp.prod[p].nfac > 1;
  for (int l = 0; l < G3_MAXLEAF; ++l) {
    double q = 0.0;
    for (int p = 0; p < sp.nprod; ++p)
      if (sp.prod[p].nfac == 1 && sp.prod[p].fac[0] == l) q += sp.prod[p].coef;
    qconst[l] = q;
  }
  return multi;
}

// add(c, d1_c prog(xi, xj)) piecewise: one call per leaf and column the leaf uses, the product rule applied -- the partial of
// leaf l times the sum, over the products and the places that hold it, of the coefficient and the OTHER factors' values
// (multiplied out, never p / f: a factor may be 0).  A piece that is not finite is passed as 0.  sp, qconst: in LDS;
// multi: prog_qconst's; lv: nleaf doubles of this thread, lvs apart (multi only).  Programs of single-factor products -- the
// common case -- evaluate every leaf once per pair; with products the values come first and the partials in a second call.
template <typename Add>
__device__ __forceinline__ void prog_d1(const g3_kernel_prog& sp, const double* qconst, bool multi, const double* xi,
                                        const double* xj, bool diag, double* lv, int lvs, const Add& add) {
  const int nleaf = sp.nleaf, nprod = sp.nprod;
  if (!multi) {
    for (int l = 0; l < nleaf; ++l) {
      const double q = qconst[l];
      if (q == 0.0) continue;
      leaf_d1<true>(sp.leaf[l], xi, xj, diag, [&add, q](int c, double g) {
        const double t = q * g;
        add(c, dx_finite(t) ? t : 0.0);
      });
    }
    return;
  }
  for (int l = 0; l < nleaf; ++l) lv[l * lvs] = leaf_d1<false>(sp.leaf[l], xi, xj, diag, DxNoEmit());
  for (int l = 0; l < nleaf; ++l) {
    const int kd = sp.leaf[l].kind;
    if (kd == G3_K_NOISE || kd == G3_K_WN || kd == G3_K_VAR) continue;   // constants: no partial
    double q = 0.0;
    for (int p = 0; p < nprod; ++p) {
      const g3_prod& pr = sp.prod[p];
      for (int f = 0; f < pr.nfac; ++f) {
        if (pr.fac[f] != l) continue;
        double v = pr.coef;
        for (int g = 0; g < pr.nfac; ++g)
          if (g != f) v *= lv[pr.fac[g] * lvs];
        q += v;
      }
    }
    if (q == 0.0) continue;
    leaf_d1<true>(sp.leaf[l], xi, xj, diag, [&add, q](int c, double g) {
      const double t = q * g;
      add(c, dx_finite(t) ? t : 0.0);
    });
  }
}
