"""NumPy / SciPy restatement of the two append entry points (include/g3hip_online.h), block for block as g3_append.hip runs
them, and the seeded problems the host and the GPU tests share.

With N0 rows factored and N1 wanted: n0 = rounddown(N0, 128), Np1 = roundup(N1, 128), r = Np1 - n0.  The padded covariance
carries the identity from N on (G3_GRAM_PAD_EYE), so the padded factor is [[L, 0], [0, I]] and a is 0 in the padding."""
import functools

import numpy as np
import scipy.linalg

P = 128
D = 3
RATE = np.array([0.8, 1.0, 1.3])
SE = ('SE', 1.3, RATE, None)
NOISE = 0.1
SPEC = ('sum', SE, ('NOISE', NOISE))


def roundup(n, m=P):
    return (int(n) + m - 1) // m * m


def plan(N0, N1):
    """(n0, Np1, r)"""
    n0, Np1 = N0 // P * P, roundup(N1)
    return n0, Np1, Np1 - n0


def capacity(have, need):
    """the workspace rule: unchanged while `need` fits, else at least 1.5 x `have`, a multiple of 128"""
    if need <= have:
        return have
    return max(roundup(have + (have + 1) // 2), roundup(need))


def padded(K, Np):
    """the N x N covariance in an Np x Np identity"""
    out = np.eye(Np)
    out[:len(K), :len(K)] = K
    return out


def factor(K, delta):
    """what g3_gp_factor leaves for the N x N covariance K: (padded lower factor, padded a = L^-1 delta, sum log L_ii, a^T a)"""
    N, Np = len(K), roundup(len(K))
    L = scipy.linalg.cholesky(padded(K, Np), lower=True)
    a = np.zeros(Np)
    a[:N] = scipy.linalg.solve_triangular(L[:N, :N], delta[:N], lower=True)
    return L, a, float(np.log(np.diag(L)[:N]).sum()), float(a @ a)


def append_factor(K1, L0, a0, delta, N0):
    """g3_gp_append: K1 the N1 x N1 covariance, (L0, a0) = factor(K1[:N0, :N0], delta[:N0])[:2]; the same four results at N1.
    Nothing of L0 / a0 from n0 on is used."""
    N1 = len(K1)
    n0, Np1, r = plan(N0, N1)
    rows = padded(K1, Np1)[n0:]                              # g3_gram_rows
    rhs = np.zeros(Np1)
    rhs[:n0], rhs[n0:N1] = a0[:n0], delta[n0:N1]             # the resumed right-hand side
    L00 = L0[:n0, :n0]
    panel = scipy.linalg.solve_triangular(L00, rows[:, :n0].T, lower=True, check_finite=False).T if n0 else np.zeros((r, 0))
    stacked = np.vstack([rows[:, n0:], rhs[None, n0:]]) - np.vstack([panel, rhs[None, :n0]]) @ panel.T      # ONE product
    corner = scipy.linalg.cholesky(stacked[:r], lower=True)
    a1 = np.concatenate([a0[:n0], scipy.linalg.solve_triangular(corner, stacked[r], lower=True)])
    L1 = np.zeros((Np1, Np1))
    L1[:n0, :n0], L1[n0:, :n0], L1[n0:, n0:] = L00, panel, corner
    return L1, a1, float(np.log(np.diag(L1)[:N1]).sum()), float(a1[:N1] @ a1[:N1])


def cross(Kx, L, a, N):
    """g3_gp_cross: (V = Kx L^-T zero-padded to the factor's columns, mu, ss) for the M x N cross covariance Kx"""
    V = np.zeros((len(Kx), len(L)))
    V[:, :N] = scipy.linalg.solve_triangular(L[:N, :N], Kx.T, lower=True).T
    return V, V @ a, (V * V).sum(axis=1)


def append_cross(V0, Kx1, L1, a1, N0):
    """g3_gp_cross_append: V0 = cross(...)[0] at N0 (columns from n0 on are not used), Kx1 the M x N1 cross covariance"""
    N1 = Kx1.shape[1]
    n0, Np1, r = plan(N0, N1)
    new = np.zeros((len(Kx1), r))
    new[:, :N1 - n0] = Kx1[:, n0:]
    new -= V0[:, :n0] @ L1[n0:, :n0].T
    new = scipy.linalg.solve_triangular(L1[n0:, n0:], new.T, lower=True).T
    V = np.hstack([V0[:, :n0], new])
    return V, V @ a1, (V * V).sum(axis=1)


@functools.lru_cache(maxsize=None)
def problem(N, M=0, seed=0):
    """(X, y, Xs): N + M points at constant density in D dimensions -- the SE + noise covariance stays near kappa ~ 1e2 at
    every N -- and a smooth response with noise"""
    rng = np.random.default_rng(1000 * seed + N)
    side = max(N, 8) ** (1.0 / D)
    X = rng.uniform(0, side, (N, D))
    y = np.sin(X.sum(axis=1) / np.sqrt(D)) + 0.1 * rng.standard_normal(N)
    Xs = rng.uniform(0, side, (M, D))           # drawn last: X and y do not depend on M
    for a in (X, y, Xs):
        a.setflags(write=False)
    return X, y, Xs


@functools.lru_cache(maxsize=None)
def covariance(N, seed=0):
    """tt_to_num of the SE + noise covariance of problem(N) from the oracle, computed once"""
    from oracle import g3_oracle as orc
    K = orc.tt_to_num(orc.kernel_cov(SPEC, problem(N, 0, seed)[0]))
    K.setflags(write=False)
    return K


@functools.lru_cache(maxsize=None)
def reference(N, seed=0):
    """factor(covariance(N), y), computed once"""
    out = factor(covariance(N, seed), problem(N, 0, seed)[1])
    for a in out[:2]:
        a.setflags(write=False)
    return out
