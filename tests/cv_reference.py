"""NumPy reference of leave-fold-out cross-validation for the tests (helper module, not collected).

Two independent routes to the same numbers, both through the oracle's GP (oracle/g3_oracle.py):

    closed_form   A = K^-1 from np.linalg.inv of the noisy covariance, alpha = A delta; per fold I: r_I = A_II^-1 alpha_I,
                  Sigma_I = A_II^-1, loc_I = z_I - r_I, and the joint normal log density from the fold's two scalars
    refits        per fold: the oracle's GP observed on the complement, its `location` and `kernel(noise=True)` at the fold's
                  inputs, the joint normal log density from np.linalg.cholesky of that kernel -- F refits

and the measured float32 error of the closed form (`fp32_gap`), from which the fp32 tests take their tolerance.
"""
import numpy as np

from oracle import g3_oracle as orc


def as_folds(folds, N):
    """int k / label array / list of index arrays -> list of index arrays, written independently of the package's parser"""
    if isinstance(folds, (int, np.integer)):
        return np.array_split(np.arange(N), folds)
    if isinstance(folds, np.ndarray) and folds.ndim == 1 and len(folds) == N:
        return [np.nonzero(folds == u)[0] for u in sorted(set(folds[folds >= 0].tolist()))]
    return [np.asarray(f, dtype=np.int64) for f in folds]


def _typed(gp, dtype):
    g = orc.GP(gp.kf, None, gp.mean_spec, gp.map.spec, dtype=dtype)
    g.kn = gp.kn
    return g


def closed_form(gp, X, y, folds, dtype=np.float64):
    """dict of resid, pvar, loc, var (length N, NaN in no fold), fold ((F, 2): log det A_II, alpha_I^T A_II^-1 alpha_I),
    logpredictive (sum of the held-out points' marginal log densities), logpredictive_joint (sum over folds of
    log p(y_I | rest)) and held (the held-out indices) of the oracle process `gp` on (X, y), everything in `dtype`"""
    X = np.asarray(X, dtype=dtype)
    y = np.asarray(y, dtype=dtype)
    N = len(y)
    folds = as_folds(folds, N)
    g = _typed(gp, dtype)
    K = np.asarray(g.prior_kernel(X, True), dtype=dtype)
    z = np.asarray(g.mapping_outputs(y), dtype=dtype)
    delta = z - np.asarray(g.prior_location(X), dtype=dtype)
    A = np.linalg.inv(K)
    alpha = A.dot(delta)
    resid, pvar = np.full(N, np.nan, dtype=dtype), np.full(N, np.nan, dtype=dtype)
    fold = np.zeros((len(folds), 2), dtype=dtype)
    t = np.dtype(dtype).type
    joint = t(0)
    for f, I in enumerate(folds):
        if len(I) == 0:
            continue
        AII = A[np.ix_(I, I)]
        S = np.linalg.inv(AII)
        r = S.dot(alpha[I])
        resid[I], pvar[I] = r, np.diag(S)
        fold[f] = np.linalg.slogdet(AII)[1], alpha[I].dot(r)
        # (every term and the running sum in `dtype`, as logp_cho forms its density: a float64 constant would promote them)
        term = t(-0.5) * fold[f, 1] + t(0.5) * fold[f, 0] + t(-0.5) * t(len(I)) * np.log(t(2.0 * np.pi)) + t(g.map.logdet_dinv(y[I]))
        joint = t(joint + t(term))
    held = np.concatenate(folds) if len(folds) else np.zeros(0, dtype=np.int64)
    loc = z - resid
    lp = orc.logp_cho(y[held], loc[held], np.diag(np.sqrt(pvar[held])).astype(dtype), g.map)
    return dict(resid=resid, pvar=pvar, loc=loc, var=pvar, fold=fold, logpredictive=lp, logpredictive_joint=joint, held=held)


def refits(gp, X, y, folds):
    """F refits in float64: dict of loc, var, mean, variance, median (length N, NaN in no fold), logpredictive and
    logpredictive_joint.  Every fold needs a non-empty complement."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    N = len(y)
    out = {k: np.full(N, np.nan) for k in ('loc', 'var', 'mean', 'variance', 'median')}
    lp = joint = 0.0
    for I in as_folds(folds, N):
        if len(I) == 0:
            continue
        keep = np.ones(N, dtype=bool)
        keep[I] = False
        Xo, yo, Xi = X[keep], y[keep], X[I]
        loc = gp.location(Xi, Xo, yo)
        S = gp.kernel(Xi, Xo, noise=True)
        out['loc'][I], out['var'][I] = loc, np.diag(S)
        out['mean'][I] = gp.mean(Xi, Xo, yo, noise=True)
        out['variance'][I] = gp.variance(Xi, Xo, yo, noise=True)
        out['median'][I] = gp.median(Xi, Xo, yo)
        lp += float(gp.logpredictive(y[I], Xi, Xo, yo))
        joint += float(orc.logp_cho(y[I], loc, np.linalg.cholesky(S), gp.map))
    out['logpredictive'], out['logpredictive_joint'] = lp, joint
    return out


def fp32_gap(gp, X, y, folds):
    """|closed form in float32 - closed form in float64| on the same (float32-representable) inputs, per quantity:
    (dict(loc, var, logpredictive, logpredictive_joint), the float64 closed form) -- what float32 arithmetic alone costs at this
    size and conditioning.  loc and var: the largest entry of the difference over the held-out points; the scores: the
    difference of the two sums."""
    X32 = np.asarray(X, dtype=np.float32)
    y32 = np.asarray(y, dtype=np.float32)
    c32 = closed_form(gp, X32, y32, folds, np.float32)
    c64 = closed_form(gp, X32.astype(np.float64), y32.astype(np.float64), folds, np.float64)
    h = c64['held']
    gap = dict(loc=float(np.abs(c32['loc'][h] - c64['loc'][h]).max()), var=float(np.abs(c32['var'][h] - c64['var'][h]).max()),
               logpredictive=abs(float(c32['logpredictive']) - float(c64['logpredictive'])),
               logpredictive_joint=abs(float(c32['logpredictive_joint']) - float(c64['logpredictive_joint'])))
    return gap, c64
