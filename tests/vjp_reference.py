"""NumPy reference of the reverse mode through the Cholesky factor for the tests (helper module, not collected).

    problem        the setting of loo_reference.problem: SE, d = 2, rate (0.9, 1.2), var 1.3, noise 0.1, seeded by n -- the
                   inputs, the noisy covariance K, its factor L, a dense random Lbar and a random symmetric dK
    reference      oracle.cholesky_grad (CholeskyRobust.grad, g3py/libs/tensors.py:224-260) on tril(Lbar)
    forward_mode   the exact derivative of the factor, dL = L Phi(L^-1 dK L^-T) (Murray 2016, eq. 8), for the adjoint identity
                   <tril Lbar, dL> = <Kbar, tril dK>
    fp32_gap       |cholesky_grad in float32 - in float64| / |ref| on the same (float32-representable) inputs: what float32
                   arithmetic alone costs at this size and conditioning
"""
import functools

import numpy as np
import scipy.linalg

from loo_reference import problem as loo_problem
from oracle import g3_oracle as orc

RATE = np.array([0.9, 1.2])
SE_SPEC = ('SE', 1.3, RATE, None)
NOISE = 0.1


def phi(A):
    """tril with halved diagonal (tril_and_halve_diagonal, tensors.py:245-247)"""
    P = np.tril(A)
    P[np.diag_indices_from(P)] *= 0.5
    return P


@functools.lru_cache(maxsize=None)
def problem(n):
    """dict(X, y, K, L, Lbar, dK) in float64, computed once per n and read-only.  Lbar is dense: what is above its diagonal
    cannot influence the result, and the tests overwrite it with NaN."""
    X, y = loo_problem(n)
    K = np.asarray(orc.GP(SE_SPEC, NOISE).prior_kernel(X, True), dtype=np.float64)
    L = np.linalg.cholesky(K)
    rng = np.random.default_rng(5000 + 11 * n)
    Lbar = rng.standard_normal((n, n))
    S = rng.standard_normal((n, n))
    out = dict(X=np.asarray(X, dtype=np.float64), y=np.asarray(y, dtype=np.float64), K=K, L=L, Lbar=Lbar, dK=S + S.T)
    for a in out.values():
        a.setflags(write=False)
    return out


def reference(L, Lbar):
    """Kbar of oracle.cholesky_grad in the dtype of L; only the lower triangle of Lbar enters"""
    return orc.cholesky_grad(np.asarray(L), np.tril(np.asarray(Lbar, dtype=np.asarray(L).dtype)))


def forward_mode(L, dK):
    """dL = L Phi(L^-1 dK L^-T) for a symmetric perturbation dK of K = L L^T"""
    A = scipy.linalg.solve_triangular(L, dK, lower=True)
    A = scipy.linalg.solve_triangular(L, A.T, lower=True).T
    return L.dot(phi(A))


def with_nan_above(Lbar):
    """a copy of Lbar whose strict upper triangle holds NaN"""
    out = np.array(Lbar, copy=True)
    out[np.triu_indices_from(out, 1)] = np.nan
    return out


@functools.lru_cache(maxsize=None)
def fp32_gap(n):
    """(gap, ref64, L32, Lbar32): the inputs rounded to float32, the float64 reference on exactly those inputs, and
    |cholesky_grad in float32 - ref64|_F / |ref64|_F"""
    p = problem(n)
    L32, B32 = p['L'].astype(np.float32), np.tril(p['Lbar']).astype(np.float32)
    ref64 = reference(L32.astype(np.float64), B32.astype(np.float64))
    got32 = reference(L32, B32)
    assert got32.dtype == np.float32
    gap = float(np.linalg.norm(got32.astype(np.float64) - ref64) / np.linalg.norm(ref64))
    for a in (ref64, L32, B32):
        a.setflags(write=False)
    return gap, ref64, L32, B32
