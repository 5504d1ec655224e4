"""NumPy reference of leave-one-out cross-validation for the tests (helper module, not collected).

Two independent routes to the same numbers, both through the oracle's GP (oracle/g3_oracle.py):

    closed_form   alpha = K^-1 delta and c = diag K^-1 from np.linalg.inv of the noisy covariance,
                  loc_i = z_i - alpha_i / c_i, var_i = 1 / c_i                          (Rasmussen & Williams 5.4.2)
    brute_force   for every i: the oracle's GP observed on the other N - 1 points, predicted at x_i with noise, and its
                  logpredictive of y_i -- N refits, O(N^4)

and the measured float32 error of the closed form (`fp32_gap`), from which the fp32 tests take their tolerance.
"""
import numpy as np

from oracle import g3_oracle as orc


def problem(N, d=2, seed=0, dtype=np.float64):
    """inputs on a box that grows with N (a fixed density keeps kappa(K) in the hundreds at noise 0.1) and a smooth signal"""
    rng = np.random.default_rng(1000 + 7 * N + seed)
    X = rng.uniform(0.0, N ** (1.0 / d), (N, d)).astype(dtype)
    y = (np.sin(X.sum(axis=1) / np.sqrt(d)) + 0.3 * rng.standard_normal(N)).astype(dtype)
    return X, y


def closed_form(gp, X, y, dtype=np.float64):
    """(alpha, c, loc, var, logpredictive) of the oracle process `gp` (orc.GP) on (X, y), everything in `dtype`"""
    X = np.asarray(X, dtype=dtype)
    y = np.asarray(y, dtype=dtype)
    g = orc.GP(gp.kf, None, gp.mean_spec, gp.map.spec, dtype=dtype)
    g.kn = gp.kn
    K = np.asarray(g.prior_kernel(X, True), dtype=dtype)
    z = np.asarray(g.mapping_outputs(y), dtype=dtype)
    delta = z - np.asarray(g.prior_location(X), dtype=dtype)
    Kinv = np.linalg.inv(K)
    alpha = Kinv.dot(delta)
    c = np.diag(Kinv).copy()
    loc = z - alpha / c
    var = 1.0 / c
    lp = orc.logp_cho(y, loc, np.diag(np.sqrt(var)).astype(dtype), g.map)
    return alpha, c, loc, var, lp


def brute_force(gp, X, y):
    """N refits in float64: dict(loc, var, mean, variance, median (length N), logpredictive (their sum))"""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    N = len(y)
    out = {k: np.empty(N) for k in ('loc', 'var', 'mean', 'variance', 'median')}
    lp = 0.0
    for i in range(N):
        keep = np.arange(N) != i
        Xo, yo, xi = X[keep], y[keep], X[i:i + 1]
        out['loc'][i] = gp.location(xi, Xo, yo)[0]
        out['var'][i] = gp.kernel_diag(xi, Xo, noise=True)[0]
        out['mean'][i] = gp.mean(xi, Xo, yo, noise=True)[0]
        out['variance'][i] = gp.variance(xi, Xo, yo, noise=True)[0]
        out['median'][i] = gp.median(xi, Xo, yo)[0]
        lp += float(gp.logpredictive(y[i:i + 1], xi, Xo, yo))
    out['logpredictive'] = lp
    return out


def fp32_gap(gp, X, y):
    """|closed form in float32 - closed form in float64| on the same (float32-representable) inputs, per quantity:
    (dict(loc, var, logpredictive), (loc, var, logpredictive in float64)) -- what float32 arithmetic alone costs at this size
    and conditioning.  loc and var: the largest entry of the difference; logpredictive: the difference of the two sums."""
    X32 = np.asarray(X, dtype=np.float32)
    y32 = np.asarray(y, dtype=np.float32)
    _, _, l32, v32, p32 = closed_form(gp, X32, y32, np.float32)
    _, _, l64, v64, p64 = closed_form(gp, X32.astype(np.float64), y32.astype(np.float64), np.float64)
    return dict(loc=float(np.abs(l32 - l64).max()), var=float(np.abs(v32 - v64).max()),
                logpredictive=abs(float(p32) - float(p64))), (l64, v64, float(p64))
