"""NumPy reference of the dot-product kernel family for the tests (helper module, not collected).

The oracle (oracle/g3_oracle.py) knows the stationary leaves only.  `kernel_cov_ext` evaluates the new leaf tuples

    ('DOT', var, rate, bias, p, dims)   var * (bias + sum_k rate_k^2 x1_k x2_k)**p    kernels.py:82-93, 324-341; metrics.py:111-131
    ('NN',  var, rate, bias, dims)      var * arcsin(2 m12 / ((1 + 2 m11)(1 + 2 m22)))  kernels.py:348-349 (pointwise)
    ('BW',  var, dims)                  var * prod_k min(x1_k, x2_k)                  kernels.py:293-295; metrics.py:54-56
    ('VAR', var)                        var                                           kernels.py:298-308 (NIL: var = 0)

and hands every other node to `oracle.g3_oracle.kernel_cov`.  The oracle's tree recursion and its GP / TP classes look
`kernel_cov` (and `kernel_cov_grads`) up as module globals, so a test installs the extended functions with

    monkeypatch.setattr(oracle.g3_oracle, 'kernel_cov', kernel_cov_ext)
    monkeypatch.setattr(oracle.g3_oracle, 'kernel_cov_grads', kernel_cov_grads_ext)

and then uses the oracle's own GP(...).logp / location / kernel_diag / dlogp_natural on mixed trees.
"""
import numpy as np

from oracle import g3_oracle as orc

_ORIG_COV = orc.kernel_cov
_ORIG_GRADS = orc.kernel_cov_grads
NEW_LEAVES = ('DOT', 'NN', 'BW', 'VAR')
_NODES = ('sum', 'prod', 'scale', 'shift')


def _cols(x, dims):
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[:, None]
    return x if dims is None else x[:, np.atleast_1d(dims)]


def _dot(a, b, rate, bias):
    """ARD_DotBias.gram: bias + dot(x1 * x2, rate**2) over the pairs -- metrics.py:130-131"""
    return bias + np.dot(a[:, None, :] * b[None, :, :], rate ** 2)


def _self(a, rate, bias):
    """m(x, x) per point"""
    return bias + np.dot(a * a, rate ** 2)


def _ipow(m, p):
    v = m
    for _ in range(int(p) - 1):
        v = v * m
    return v


def kernel_cov_ext(spec, x1, x2=None, dtype=np.float64):
    op = spec[0]
    if op not in NEW_LEAVES:
        # composite nodes recurse through orc.kernel_cov (a module global: the patched function when installed);
        # without the patch installed, recurse here
        if op in _NODES and orc.kernel_cov is not kernel_cov_ext:
            t = np.dtype(dtype).type
            if op == 'sum':
                return kernel_cov_ext(spec[1], x1, x2, dtype) + kernel_cov_ext(spec[2], x1, x2, dtype)
            if op == 'prod':
                return kernel_cov_ext(spec[1], x1, x2, dtype) * kernel_cov_ext(spec[2], x1, x2, dtype)
            if op == 'scale':
                return t(spec[1]) * kernel_cov_ext(spec[2], x1, x2, dtype)
            return t(spec[1]) + kernel_cov_ext(spec[2], x1, x2, dtype)
        return _ORIG_COV(spec, x1, x2, dtype)
    t = np.dtype(dtype).type
    a = np.asarray(x1, dtype=dtype)
    a = a[:, None] if a.ndim == 1 else a
    b = a if x2 is None else np.asarray(x2, dtype=dtype)
    b = b[:, None] if b.ndim == 1 else b
    var = t(spec[1])
    if op == 'VAR':
        return var * np.ones((a.shape[0], b.shape[0]), dtype=dtype)
    dims = spec[-1]
    a, b = _cols(a, dims), _cols(b, dims)
    if op == 'BW':
        return var * np.prod(np.minimum(a[:, None, :], b[None, :, :]), axis=2)
    rate = np.broadcast_to(np.asarray(spec[2], dtype=dtype), (a.shape[1],))
    bias = t(spec[3])
    m12 = _dot(a, b, rate, bias)
    if op == 'DOT':
        return var * _ipow(m12, spec[4])
    m11, m22 = _self(a, rate, bias), _self(b, rate, bias)
    return var * np.arcsin(t(2) * m12 / ((t(1) + t(2) * m11)[:, None] * (t(1) + t(2) * m22)[None, :]))


def nn_argument(spec, x):
    """the arcsin argument of an NN leaf on the square case (|s| <= 1/4 analytically: 2ab <= a^2 + b^2 and
    (1 + 2u)^2 >= 8u)"""
    a = _cols(np.asarray(x, dtype=np.float64), spec[-1])
    rate = np.broadcast_to(np.asarray(spec[2], dtype=np.float64), (a.shape[1],))
    m11 = _self(a, rate, spec[3])
    return 2 * _dot(a, a, rate, spec[3]) / ((1 + 2 * m11)[:, None] * (1 + 2 * m11)[None, :])


def kernel_cov_grads_ext(spec, x, dtype=np.float64, _leaf=None):
    """(K, [(leaf, pname, k, dK)]) as oracle.g3_oracle.kernel_cov_grads returns it, with the new leaves: `alpha` is the
    bias of a DOT / NN leaf.  With m = bias + sum_k rate_k^2 x_ik x_jk:
      DOT  dK/dvar = m^p, dK/dbias = var p m^(p-1), dK/drate_k = var p m^(p-1) 2 rate_k x_ik x_jk
      NN   s = 2 m12 / (a b), a = 1 + 2 m11, b = 1 + 2 m22:
           dK/dtheta = var / sqrt(1 - s^2) [2 dm12 / (a b) - s (2 dm11 / a + 2 dm22 / b)]
      BW, VAR: var only."""
    x = np.asarray(x, dtype=dtype)
    if x.ndim == 1:
        x = x[:, None]
    if _leaf is None:
        _leaf = [0]
    op = spec[0]
    if op in ('sum', 'prod'):
        K1, g1 = kernel_cov_grads_ext(spec[1], x, dtype, _leaf)
        K2, g2 = kernel_cov_grads_ext(spec[2], x, dtype, _leaf)
        if op == 'sum':
            return K1 + K2, g1 + g2
        return K1 * K2, [(l, p, k, dK * K2) for l, p, k, dK in g1] + [(l, p, k, dK * K1) for l, p, k, dK in g2]
    if op == 'scale':
        K, g = kernel_cov_grads_ext(spec[2], x, dtype, _leaf)
        return spec[1] * K, [(l, p, k, spec[1] * dK) for l, p, k, dK in g]
    if op == 'shift':
        K, g = kernel_cov_grads_ext(spec[2], x, dtype, _leaf)
        return spec[1] + K, g
    if op not in NEW_LEAVES:
        return _ORIG_GRADS(spec, x, dtype, _leaf)
    leaf = _leaf[0]
    _leaf[0] += 1
    var = spec[1]
    n = x.shape[0]
    if op == 'VAR':
        return var * np.ones((n, n)), [(leaf, 'var', None, np.ones((n, n)))]
    a = _cols(x, spec[-1])
    nd = a.shape[1]
    if op == 'BW':
        k0 = np.prod(np.minimum(a[:, None, :], a[None, :, :]), axis=2)
        return var * k0, [(leaf, 'var', None, k0)]
    rate = np.broadcast_to(np.asarray(spec[2], dtype=dtype), (nd,))
    bias = spec[3]
    m12 = _dot(a, a, rate, bias)
    xx = a[:, None, :] * a[None, :, :]                     # x_ik x_jk
    if op == 'DOT':
        p = int(spec[4])
        mp1 = _ipow(m12, p - 1) if p > 1 else np.ones_like(m12)
        grads = [(leaf, 'var', None, mp1 * m12), (leaf, 'alpha', None, var * p * mp1)]
        for k in range(nd):
            grads.append((leaf, 'rate', k, var * p * mp1 * 2 * rate[k] * xx[:, :, k]))
        return var * mp1 * m12, grads
    m11 = _self(a, rate, bias)
    A, B = (1 + 2 * m11)[:, None], (1 + 2 * m11)[None, :]
    s = 2 * m12 / (A * B)
    c = var / np.sqrt(1 - s * s)
    grads = [(leaf, 'var', None, np.arcsin(s)),
             (leaf, 'alpha', None, c * (2 / (A * B) - s * (2 / A + 2 / B)))]
    for k in range(nd):
        dm12 = 2 * rate[k] * xx[:, :, k]
        dm11 = (2 * rate[k] * a[:, k] ** 2)[:, None]
        dm22 = (2 * rate[k] * a[:, k] ** 2)[None, :]
        grads.append((leaf, 'rate', k, c * (2 * dm12 / (A * B) - s * (2 * dm11 / A + 2 * dm22 / B))))
    return var * np.arcsin(s), grads


def dot_zoo(d):
    """every class alone and mixed sum / product / scale / shift trees, as spec tuples for inputs with d columns"""
    r = np.linspace(0.6, 1.3, d)
    sub = np.array([0, d - 1]) if d > 1 else None
    rs = r[[0, d - 1]] if d > 1 else r
    se = ('SE', 1.1, np.linspace(0.5, 0.9, d), None)
    return {
        'KernelDot': ('DOT', 1.3, r, 0.0, 1, None),
        'LIN': ('DOT', 1.0, r, 0.5, 1, None),
        'POL2': ('DOT', 1.0, r, 0.5, 2, None),
        'POL3': ('DOT', 0.7, r, 0.4, 3, None),
        'POL4': ('DOT', 1.0, 0.5 * r, 0.3, 4, None),
        'NN': ('NN', 1.4, r, 0.5, None),
        'BW': ('BW', 0.8, None),
        'VAR': ('VAR', 0.6),
        'NIL': ('VAR', 0.0),
        'LIN+SE': ('sum', ('DOT', 1.0, r, 0.5, 1, None), se),
        'POL*SE': ('prod', ('DOT', 1.0, r, 0.5, 2, None), se),
        '2*NN+0.1': ('shift', 0.1, ('scale', 2.0, ('NN', 1.0, r, 0.5, None))),
        'BW[dims]+VAR': ('sum', ('BW', 0.8, sub), ('VAR', 0.3)),
        'NIL+OU': ('sum', ('VAR', 0.0), ('OU', 0.9, np.linspace(0.4, 0.8, d), None)),
        'LIN[dims]+SE+noise': ('sum', ('sum', ('DOT', 1.0, rs, 0.5, 1, sub), se), ('NOISE', 0.1)),
    }


def has_bw(spec):
    if spec[0] in _NODES:
        return any(has_bw(s) for s in spec[1:] if isinstance(s, tuple))
    return spec[0] == 'BW'


def zoo_inputs(spec, n, d, seed):
    """inputs of both signs for the dot group and NN, strictly positive where a BW leaf is present"""
    rng = np.random.default_rng(seed)
    if has_bw(spec):
        return rng.uniform(0.2, 3.0, (n, d))
    return 1.5 * rng.standard_normal((n, d))
