"""NumPy reference of the gradient of the leave-one-out log predictive for the tests (helper module, not collected).

With A = K^-1 of the noisy covariance, delta = T^-1(y) - m(X), alpha = A delta and c = diag A the score of
loo_reference.closed_form is F = sum_i [1/2 log c_i - 1/2 alpha_i^2 / c_i] - N/2 log 2 pi + log |det dT^-1(y)| and

    dF = sum_ij W_ij dK_ij - u . d delta + d logdet,     W = -A diag(q) A + 1/2 (u alpha^T + alpha u^T),
    q_i = 1/2 (1 / c_i + alpha_i^2 / c_i^2),             u = A b,  b_i = alpha_i / c_i

in natural parameter space, everything through the oracle's GP (oracle/g3_oracle.py) and np.linalg.inv.  `lbar` is the same
gradient as a function of the Cholesky factor, `finite_difference` the central difference of the closed form's score, and
`fp32_gap` the measured float32 error of this closed form, from which the fp32 tests take their tolerance.
"""
import numpy as np

from loo_reference import closed_form
from oracle import g3_oracle as orc


def _gp(gp, dtype):
    g = orc.GP(gp.kf, None, gp.mean_spec, gp.map.spec, dtype=dtype)
    g.kn = gp.kn
    return g


def weights(gp, X, y, dtype=np.float64):
    """(W, u, alpha, c) of the oracle process `gp` on (X, y) in `dtype`; W symmetric"""
    X, y = np.asarray(X, dtype=dtype), np.asarray(y, dtype=dtype)
    g = _gp(gp, dtype)
    K = np.asarray(g.prior_kernel(X, True), dtype=dtype)
    delta = np.asarray(g.mapping_outputs(y), dtype=dtype) - np.asarray(g.prior_location(X), dtype=dtype)
    A = np.linalg.inv(K)
    A = (A + A.T) / np.dtype(dtype).type(2)
    alpha = A.dot(delta)
    c = np.diag(A).copy()
    q = (1 / c + alpha ** 2 / c ** 2) / np.dtype(dtype).type(2)
    u = A.dot(alpha / c)
    W = -(A * q).dot(A) + (np.outer(u, alpha) + np.outer(alpha, u)) / np.dtype(dtype).type(2)
    return W.astype(dtype), u.astype(dtype), alpha.astype(dtype), c.astype(dtype)


def reference(gp, X, y, dtype=np.float64):
    """dict(slots={(leaf, pname, k): sum_ij W_ij dK_ij}, mean=[(pname, k, u . column)], mapping=[(pname, -u . dinv +
    dlogdet)], W, u, alpha, c) in natural space, in `dtype`"""
    X, y = np.asarray(X, dtype=dtype), np.asarray(y, dtype=dtype)
    g = _gp(gp, dtype)
    W, u, alpha, c = weights(gp, X, y, dtype)
    x = g._x(X)
    _, kg = orc.kernel_cov_grads(g.kn, x, dtype)
    slots = {(l, p, k): np.sum(W * np.asarray(dK, dtype=dtype), dtype=dtype) for l, p, k, dK in kg}
    mean = [(p, k, u.dot(np.asarray(col, dtype=dtype))) for p, k, col in orc.mean_grads(g.mean_spec, x, dtype)]
    mapping = [(p, -u.dot(np.asarray(dcol, dtype=dtype)) + ds) for (p, dcol), (_, ds) in zip(g.map.dinv(y), g.map.dlogdet_dinv(y))]
    return dict(slots=slots, mean=mean, mapping=mapping, W=W, u=u, alpha=alpha, c=c)


def natural_vector(ref):
    """the reference's entries as one vector: kernel slots in the oracle's order, then mean, then mapping"""
    return np.array([float(v) for v in ref['slots'].values()] + [float(v) for _, _, v in ref['mean']]
                    + [float(v) for _, v in ref['mapping']])


def lbar(gp, X, y):
    """L -> Lbar = 2 tril(W L): the score's gradient with respect to the factor, for factor_vjp and orc.cholesky_grad"""
    W = weights(gp, X, y)[0]
    return lambda L: 2.0 * np.tril(W.dot(np.tril(L)))


def finite_difference(make_gp, theta, X, y, h=1e-6):
    """central differences of loo_reference.closed_form's log predictive over the entries of the natural-space vector
    `theta`; make_gp(theta) -> orc.GP; step h * max(1, |theta_k|)"""
    theta = np.asarray(theta, dtype=np.float64)
    out = np.empty(len(theta))
    for k in range(len(theta)):
        e = np.zeros(len(theta))
        e[k] = h * max(1.0, abs(theta[k]))
        out[k] = (float(closed_form(make_gp(theta + e), X, y)[4]) - float(closed_form(make_gp(theta - e), X, y)[4])) / (2 * e[k])
    return out


def fp32_gap(gp, X, y):
    """(gap, ref64): |this closed form in float32 - in float64| / |in float64| as vector norms over natural_vector, on the
    same float32-representable inputs, and the float64 reference dict -- what float32 arithmetic alone costs here"""
    X32, y32 = np.asarray(X, dtype=np.float32), np.asarray(y, dtype=np.float32)
    r32 = reference(gp, X32, y32, np.float32)
    r64 = reference(gp, X32.astype(np.float64), y32.astype(np.float64), np.float64)
    v32, v64 = natural_vector(r32), natural_vector(r64)
    return float(np.linalg.norm(v32 - v64) / np.linalg.norm(v64)), r64
