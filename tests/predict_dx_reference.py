"""NumPy reference of the gradients of the posterior location and variance with respect to the query inputs, for the
tests (helper module, not collected).

    d1            (k, d1 k): a spec tree's cross covariance k(xs_i, x_j) and its partials with respect to the columns of xs_i,
                  all 15 leaf kinds and the sum / prod / scale / shift nodes over dot_reference.kernel_cov_ext's spec tuples
    dkss          d k(x, x) / d x on the square-case diagonal: 2 d1 at x' = x
    closed_form   (dloc, ddiag, dsd) of an oracle process from np.linalg.inv, refined in long double (_inverse)
    central       (dloc, ddiag) by central differences through the oracle's GP.location and GP.kernel_diag -- a route that does
                  not rest on the closed form
    fp32_gap      the measured float32 error of the closed form, from which the fp32 tests take their tolerance

Conventions at the kinks: OU sign(0) = 0, SINC 0 at dx = 0, BW 1/2 at a tie (which makes 2 d1 exact on the diagonal).
"""
import numpy as np

from dot_reference import kernel_cov_ext
from oracle import g3_oracle as orc

PI = np.pi
_CONST = ('NOISE', 'WN', 'VAR')

# every leaf kind alone and three mixed trees (products of two and of three factors, scale, shift, dims subsets), d = 3
D = 3
R = np.array([0.6, 0.9, 1.2])
F = np.array([0.11, 0.07, 0.05])
P = np.array([0.7, 0.5, 0.3])
SUB = np.array([0, 2])
LEAVES = {
    'SE': ('SE', 1.3, R, None), 'OU': ('OU', 0.9, R, None), 'MAT32': ('MAT32', 1.1, R, None), 'MAT52': ('MAT52', 0.8, R, None),
    'RQ': ('RQ', 1.2, R, 1.7, None), 'COS': ('COS', 0.9, F, None), 'SIN': ('SIN', 0.7, F, P, None),
    'SINC': ('SINC', 1.1, F, None), 'SM': ('SM', 1.2, F, 0.3 * P, None), 'NOISE': ('NOISE', 0.4), 'WN': ('WN', 0.4, None),
    'DOT': ('DOT', 0.7, R, 0.4, 3, None), 'NN': ('NN', 1.4, R, 0.5, None), 'BW': ('BW', 0.8, None), 'VAR': ('VAR', 0.6),
}
TREES = {
    'POL*SE+COS': ('sum', ('prod', ('DOT', 1.0, R, 0.5, 2, None), ('SE', 1.1, R, None)), ('COS', 0.9, F, None)),
    '2*MAT52*SIN+0.1+noise': ('sum', ('shift', 0.1, ('scale', 2.0, ('prod', ('MAT52', 0.8, R, None), ('SIN', 0.7, F, P, None)))),
                              ('NOISE', 0.1)),
    'SE[dims]*NN*BW[dims]': ('prod', ('prod', ('SE', 1.3, R[SUB], SUB), ('NN', 1.4, R, 0.5, None)), ('BW', 0.8, SUB)),
}


def _loo_prod(f, m):
    """product over the last axis of f with entry m left out"""
    return np.prod(np.delete(f, m, axis=-1), axis=-1)


def _leaf_d1(spec, a, b, dtype):
    """(M, N, d): d leaf(a_i, b_j) / d a_ic"""
    op = spec[0]
    t = np.dtype(dtype).type
    M, N, d = a.shape[0], b.shape[0], a.shape[1]
    out = np.zeros((M, N, d), dtype=dtype)
    if op in _CONST:
        return out
    dims = spec[-1]
    cols = np.arange(d) if dims is None else np.atleast_1d(dims)
    nd = len(cols)
    A, B = a[:, cols], b[:, cols]
    dx = A[:, None, :] - B[None, :, :]
    var = t(spec[1])

    def vec(v):
        return np.broadcast_to(np.asarray(v, dtype=dtype), (nd,))
    with np.errstate(all='ignore'):
        if op in ('SE', 'MAT32', 'MAT52', 'RQ'):
            rate = vec(spec[2])
            D = np.dot(dx ** 2, t(0.5) * rate ** 2)
            if op == 'SE':
                dk = -var * np.exp(-D)
            elif op == 'MAT32':
                dk = t(-1.5) * var * np.exp(-np.sqrt(t(3) * D))
            elif op == 'MAT52':
                s = np.sqrt(t(5) * D)
                dk = -t(5) / t(6) * (t(1) + s) * var * np.exp(-s)
            else:
                al = t(spec[3])
                dk = -var * np.power(t(1) + D / al, -al - t(1))
            g = dk[..., None] * rate ** 2 * dx
        elif op == 'OU':
            rate = vec(spec[2])
            k = var * np.exp(-np.dot(np.abs(dx), rate))
            g = -k[..., None] * rate * np.sign(dx)
        elif op == 'COS':
            f = vec(spec[2])
            th = t(2 * PI) * dx * f
            c = np.cos(th)
            g = np.stack([-t(2 * PI) * f[m] * var * np.sin(th[..., m]) * _loo_prod(c, m) for m in range(nd)], axis=-1)
        elif op == 'SIN':
            f, r = vec(spec[2]), vec(spec[3])
            k = var * np.exp(t(2) * np.dot(np.sin(t(PI) * dx * f) ** 2, r))
            g = k[..., None] * t(2 * PI) * f * r * np.sin(t(2 * PI) * f * dx)
        elif op == 'SINC':
            f = vec(spec[2])
            th = t(2 * PI * PI) * f * dx
            sinc = np.where(dx != 0, np.sin(th) / th, t(1))
            df = np.where(dx != 0, (np.cos(th) - sinc) / dx, t(0))
            g = np.stack([var * df[..., m] * _loo_prod(sinc, m) for m in range(nd)], axis=-1)
        elif op == 'SM':
            f, r = vec(spec[2]), vec(spec[3])
            env = var * np.exp(t(-2 * PI * PI) * np.dot(dx ** 2, r ** 2))
            th = t(2 * PI) * f * dx
            c = np.cos(th)
            g = np.stack([env * (t(-4 * PI * PI) * r[m] ** 2 * dx[..., m] * np.prod(c, axis=-1)
                                 - t(2 * PI) * f[m] * np.sin(th[..., m]) * _loo_prod(c, m)) for m in range(nd)], axis=-1)
        elif op == 'DOT':
            rate, bias, p = vec(spec[2]), t(spec[3]), int(spec[4])
            m = bias + np.dot(A[:, None, :] * B[None, :, :], rate ** 2)
            mp1 = np.ones_like(m)
            for _ in range(p - 1):
                mp1 = mp1 * m
            g = (var * t(p) * mp1)[..., None] * rate ** 2 * B[None, :, :]
        elif op == 'NN':
            rate, bias = vec(spec[2]), t(spec[3])
            m12 = bias + np.dot(A[:, None, :] * B[None, :, :], rate ** 2)
            a1 = (t(1) + t(2) * (bias + np.dot(A * A, rate ** 2)))[:, None]
            b1 = (t(1) + t(2) * (bias + np.dot(B * B, rate ** 2)))[None, :]
            u = t(2) * m12 / (a1 * b1)
            g = (var / np.sqrt(t(1) - u * u))[..., None] * (
                t(2) * rate ** 2 * B[None, :, :] / (a1 * b1)[..., None] - u[..., None] * t(4) * rate ** 2 * A[:, None, :] / a1[..., None])
        elif op == 'BW':
            mn = np.minimum(A[:, None, :], B[None, :, :])
            ind = np.where(A[:, None, :] < B[None, :, :], t(1), np.where(A[:, None, :] == B[None, :, :], t(0.5), t(0)))
            g = np.stack([var * ind[..., m] * _loo_prod(mn, m) for m in range(nd)], axis=-1)
        else:
            raise ValueError('unknown kernel spec ' + str(op))
    np.add.at(out, (slice(None), slice(None), cols), g.astype(dtype))
    return out


def d1(spec, xs, x, dtype=np.float64, diag=False):
    """(k, g): k (M, N) = the spec tree on the pairs (xs_i, x_j), g (M, N, d) = d k_ij / d xs_ic.  diag=True: the pairs
    (xs_i, xs_j) with the SQUARE-case values (NOISE / WN on the diagonal), of which only i == j is meaningful (dkss)"""
    a = np.asarray(xs, dtype=dtype)
    a = a[:, None] if a.ndim == 1 else a
    b = a if diag else np.asarray(x, dtype=dtype)
    b = b[:, None] if b.ndim == 1 else b
    t = np.dtype(dtype).type
    op = spec[0]
    if op in ('sum', 'prod'):
        k1, g1 = d1(spec[1], a, b, dtype, diag)
        k2, g2 = d1(spec[2], a, b, dtype, diag)
        if op == 'sum':
            return k1 + k2, g1 + g2
        return k1 * k2, g1 * k2[..., None] + g2 * k1[..., None]
    if op == 'scale':
        k, g = d1(spec[2], a, b, dtype, diag)
        return t(spec[1]) * k, t(spec[1]) * g
    if op == 'shift':
        k, g = d1(spec[2], a, b, dtype, diag)
        return t(spec[1]) + k, g
    return kernel_cov_ext(spec, a, None if diag else b, dtype), _leaf_d1(spec, a, b, dtype)


def dkss(spec, xs, dtype=np.float64):
    """(M, d): d k(x, x) / d x_c at x = xs_i -- every leaf is symmetric, so twice the partial in the first argument"""
    _, g = d1(spec, xs, None, dtype, diag=True)
    i = np.arange(g.shape[0])
    return np.dtype(dtype).type(2) * g[i, i, :]


def mean_dx(mean_spec, xs, dtype=np.float64):
    xs = np.asarray(xs, dtype=dtype)
    out = np.zeros(xs.shape, dtype=dtype)
    if mean_spec[0] == 'Linear':
        cols = slice(None) if len(mean_spec) < 4 or mean_spec[3] is None else mean_spec[3]
        out[:, cols] = np.asarray(mean_spec[2], dtype=dtype)
    return out


_INVERSES = {}


def _inverse(K):
    """(K^-1, the type it is held in).  float64: np.linalg.inv refined by two Newton steps A <- A + A (I - K A) in long double,
    and the contractions that follow stay in long double -- d diag is the difference of two sums that can be 1e4 times
    larger than it (a polynomial kernel on inputs of both signs), where kappa(K) eps of plain float64 would show at 1e-7.
    float32: plain float32, whose error is what fp32_gap is there to measure.  The last few inverses are remembered."""
    if K.dtype != np.float64:
        return np.linalg.inv(K), K.dtype.type
    key = K.tobytes()
    if key not in _INVERSES:
        if len(_INVERSES) >= 4:
            _INVERSES.clear()
        wide = np.longdouble
        Kw, A = K.astype(wide), np.linalg.inv(K).astype(wide)
        eye = np.eye(len(K), dtype=wide)
        for _ in range(2):
            A = A + A.dot(eye - Kw.dot(A))
        _INVERSES[key] = A
    return _INVERSES[key], np.longdouble


def closed_form(gp, X, y, Xs, noise=False, jitter=0.0, dtype=np.float64, prior=False):
    """(dloc, ddiag, dsd), each (M, d): the gradients with respect to Xs of the oracle process's location, kernel_diag
    (clipped at 0: zero gradient where it clips) and kernel_sd (0 where sd == 0), from the inverse of the noisy covariance
    (+ jitter * I: a factor that went through the jitter schedule is differentiated as it was kept), _inverse above"""
    t = np.dtype(dtype).type
    X, Xs, y = np.asarray(X, dtype=dtype), np.asarray(Xs, dtype=dtype), np.asarray(y, dtype=dtype)
    X = X[:, None] if X.ndim == 1 else X
    Xs = Xs[:, None] if Xs.ndim == 1 else Xs
    kspec = gp.kn if noise else gp.kf
    dloc = mean_dx(gp.mean_spec, Xs, dtype)
    ddiag = dkss(kspec, Xs, dtype)
    kss = np.diag(kernel_cov_ext(kspec, Xs, None, dtype))
    if noise:
        kss = np.diag(orc.tt_to_cov(np.diag(kss)))
    diag = kss
    if not prior:
        K = orc.tt_to_cov(kernel_cov_ext(gp.kn, X, None, dtype)) + t(jitter) * np.eye(len(X), dtype=dtype)
        A, wide = _inverse(K)
        mp = orc.Mapping(gp.map.spec, dtype)
        delta = orc.tt_to_num(mp.inv(y)) - orc.mean_eval(gp.mean_spec, X, dtype)
        alpha = A.dot(delta.astype(wide))
        k, g = d1(kspec, Xs, X, dtype)
        k = orc.tt_to_num(k).astype(wide)
        g = g.astype(wide)
        w = k.dot(A)
        dloc = (dloc + np.einsum('j,ijc->ic', alpha, g)).astype(dtype)
        ddiag = (ddiag - wide(2) * np.einsum('ij,ijc->ic', w, g)).astype(dtype)
        diag = (kss - np.sum(w * k, axis=1)).astype(dtype)
    ddiag = np.where((diag < 0)[:, None], t(0), ddiag)
    sd = np.sqrt(np.where(diag < 0, t(0), diag))
    with np.errstate(all='ignore'):
        dsd = np.where((sd > 0)[:, None], ddiag / (t(2) * sd)[:, None], t(0))
    return dloc.astype(dtype), ddiag.astype(dtype), dsd.astype(dtype)


def central(gp, X, y, Xs, h=1e-5):
    """(dloc, ddiag) by central differences of the oracle's GP.location and GP.kernel_diag (float64, noise=False)"""
    Xs = np.asarray(Xs, dtype=np.float64)
    Xs = Xs[:, None] if Xs.ndim == 1 else Xs
    dloc, ddiag = np.empty(Xs.shape), np.empty(Xs.shape)
    for c in range(Xs.shape[1]):
        up, dn = Xs.copy(), Xs.copy()
        up[:, c] += h
        dn[:, c] -= h
        dloc[:, c] = (gp.location(up, X, y) - gp.location(dn, X, y)) / (2 * h)
        ddiag[:, c] = (gp.kernel_diag(up, X) - gp.kernel_diag(dn, X)) / (2 * h)
    return dloc, ddiag


def central_cov(spec, xs, x, h=1e-5):
    """(M, N, d): central differences of kernel_cov_ext(spec, xs, x) in the columns of xs"""
    xs = np.asarray(xs, dtype=np.float64)
    out = np.empty((xs.shape[0], np.asarray(x).shape[0], xs.shape[1]))
    for c in range(xs.shape[1]):
        up, dn = xs.copy(), xs.copy()
        up[:, c] += h
        dn[:, c] -= h
        out[:, :, c] = (kernel_cov_ext(spec, up, x) - kernel_cov_ext(spec, dn, x)) / (2 * h)
    return out


def fp32_gap(gp, X, y, Xs, noise=False):
    """|closed form in float32 - closed form in float64| on the same (float32-representable) inputs, per quantity:
    (dict(location, kernel_diag, kernel_sd), the float64 triple) -- what float32 arithmetic alone costs at this size and
    conditioning; the largest entry of each difference"""
    X32, y32, S32 = (np.asarray(v, dtype=np.float32) for v in (X, y, Xs))
    r32 = closed_form(gp, X32, y32, S32, noise=noise, dtype=np.float32)
    r64 = closed_form(gp, X32.astype(np.float64), y32.astype(np.float64), S32.astype(np.float64), noise=noise)
    return {k: float(np.abs(a.astype(np.float64) - b).max()) for k, a, b in zip(('location', 'kernel_diag', 'kernel_sd'), r32, r64)}, r64
