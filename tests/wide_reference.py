"""Inputs, kernel expressions, tolerances and fp64 references shared by tests/test_gpu_wide_inputs.py (GPU) and the wide
structures of tests/test_host.py (CPU): inputs of up to G3_MAXCOLS = 40 columns, leaves on up to G3_MAXD = 32 of them.

Every leaf gets per-column values that all differ -- a dropped, repeated or swapped column changes every element -- scaled
with the number of columns so that the covariance stays of order one: the exponent of an L2 leaf is sum_k rate_k^2 dx_k^2
(rate ~ 1 / sqrt(nd)), the exponent of OU's L1 metric is sum_k rate_k |dx_k| (rate ~ 1 / nd; at 1 / sqrt(nd) the off-diagonal
of OU at 16 columns is 4e-3 and `assert_condition` below refuses it).  The reference is oracle/g3_oracle.py in fp64, evaluated
live on the same inputs (for fp32 kernels: on the fp32-rounded inputs)."""
import functools

import numpy as np
import scipy.linalg

STATIONARY = ('SE', 'OU', 'MAT32', 'MAT52', 'RQ')
GRAM_WIDTHS = (5, 7, 9, 15, 17, 31, 32, 33, 40)
MAXD = 32


def rate(nd):
    return np.linspace(0.6, 1.4, nd) / np.sqrt(nd)


def freq(nd):
    return np.linspace(0.05, 0.3, nd) / np.sqrt(nd)


def leaf(kind, cols, var=1.3):
    """one leaf of `kind` on the columns `cols` with this module's per-column values"""
    cols = np.asarray(cols, dtype=int)
    nd = len(cols)
    if kind == 'OU':
        return (kind, var, np.linspace(0.6, 1.4, nd) / nd, cols)
    if kind == 'RQ':
        return (kind, var, rate(nd), 1.7, cols)
    if kind in ('SE', 'MAT32', 'MAT52'):
        return (kind, var, rate(nd), cols)
    if kind == 'COS':
        return (kind, var, freq(nd), cols)
    if kind == 'SM':
        return (kind, var, freq(nd), 0.3 * rate(nd), cols)
    if kind == 'WN':
        return (kind, var, cols)
    raise ValueError(kind)


def top(d):
    """the (at most 32) highest columns of a d-column input: column 39 at d = 40"""
    return np.arange(max(0, d - MAXD), d)


def se_plus_cos(d, ncos, kind='SE', cvar=0.4):
    """1.3 * stationary(top 32 columns) + cvar * COS(first ncos columns)"""
    return ('sum', leaf(kind, top(d)), leaf('COS', np.arange(ncos), cvar))


def width_specs(d):
    """the expressions of the width sweep: name -> spec (no leaf uses more than 32 columns)"""
    strided = np.arange(0, d, 2)
    others = np.arange(1, d, 2)
    return {
        'SE': leaf('SE', top(d)),
        'MAT52*RQ+WN': ('sum', ('prod', leaf('MAT52', strided), leaf('RQ', others, 1.0)), leaf('WN', [d - 1], 0.2)),
        'SE[descending]': leaf('SE', np.arange(min(d, MAXD))[::-1]),
    }


def boundary_cases():
    """the LDS / trig-pair boundary cases: name -> (d, spec, trig pairs)"""
    return {
        'd16_cos16': (16, se_plus_cos(16, 16), 16),
        'd32_cos16': (32, se_plus_cos(32, 16), 16),
        'd32_cos17': (32, se_plus_cos(32, 17), 17),
        'd32_cos24': (32, se_plus_cos(32, 24), 24),
        'd32_cos25': (32, se_plus_cos(32, 25), 25),
        'd40_cos12': (40, se_plus_cos(40, 12), 12),
        'd40_sm8': (40, ('sum', leaf('SE', top(40)), leaf('SM', np.arange(8), 0.4)), 8),
    }


def gradient_specs():
    """the wide structures of the gradient tests: name -> (d, spec, slots)"""
    from oracle import g3_oracle as orc
    se32_ou6 = ('sum', leaf('SE', np.arange(32)), leaf('OU', np.arange(32, 38), 0.8))
    out = {
        'd38_40slots': (38, se32_ou6, 40),
        'd38_41slots': (38, orc.with_noise(se32_ou6, 0.1), 41),
        'd31_32slots': (31, leaf('SE', np.arange(31)), 32),
        'd32_33slots': (32, leaf('SE', np.arange(32)), 33),
        'd40_se_times_cos': (40, orc.with_noise(('prod', leaf('SE', top(40)), leaf('COS', np.arange(12), 1.0)), 0.1), 47),
    }
    for kind in STATIONARY:
        out['d16_%s' % kind] = (16, leaf(kind, np.arange(16)), 17 + (kind == 'RQ'))
        out['d16_%s_noise' % kind] = (16, orc.with_noise(leaf(kind, np.arange(16)), 0.1), 18 + (kind == 'RQ'))
    return out


# dynamic LDS of the two run-time Gram paths, from the formulas of g3_gram.hip (gram_t) and g3_gram_jit.hip (g3i_gram_jit)
JIT_MAX_PAIRS, JIT_MAX_LDS, INTERP_MAX_PAIRS = 24, 96 * 1024, 16


def lds_generated(d, pairs, itemsize):
    return 192 * ((d | 1) + ((2 * pairs) | 1 if pairs else 0)) * itemsize


def lds_interpreted(d, pairs, itemsize):
    nt = pairs if pairs <= INTERP_MAX_PAIRS else 0
    return 192 * ((d | 1) + (2 * nt + 1 if nt else 0)) * itemsize


def generated_declines(d, pairs, itemsize):
    """the unambiguous half of g3i_gram_jit's rule: more than 24 pairs or more than 96 KiB -> no generated kernel"""
    return pairs > JIT_MAX_PAIRS or lds_generated(d, pairs, itemsize) > JIT_MAX_LDS


@functools.lru_cache(maxsize=None)
def inputs(n, d, seed=0):
    """X ~ U(0, 3)^(n x d), seeded; read-only (shared between tests)"""
    X = np.random.default_rng(100000 * seed + 1000 * d + n).uniform(0, 3, (n, d))
    X.setflags(write=False)
    return X


def as_seen(X, dtype):
    """the inputs as a kernel of `dtype` sees them, in fp64 (the oracle is evaluated on these)"""
    return np.asarray(X, dtype=dtype).astype(np.float64)


def assert_condition(ref, square=True):
    """from the reference alone: the 1st percentile of |off-diagonal entries| is >= 0.05, so the absolute part of the
    tolerance cannot swallow a covariance that has underflowed"""
    ref = np.asarray(ref)
    off = np.abs(ref[~np.eye(len(ref), dtype=bool)]) if square else np.abs(ref).ravel()
    p1 = np.percentile(off, 1)
    assert p1 >= 0.05, 'reference off-diagonal 1st percentile %.3g < 0.05: the inputs do not test this expression' % p1


def gram_tol(dtype, ref):
    """the project's Gram tolerances (tests/test_gpu_gram.py)"""
    m = max(1.0, float(np.abs(ref).max()))
    if np.dtype(dtype) == np.float64:
        return dict(rtol=2e-12, atol=1e-13 * m)
    return dict(rtol=3e-4, atol=3e-5 * m)


def upload(dev, X, dtype, extra=0):
    """X on the device; extra > 0: leading dimension d + extra, the extra columns NaN (a kernel that reads them shows it)"""
    X = np.asarray(X, dtype=dtype)
    if not extra:
        return dev.upload(X)
    n, d = X.shape
    A = dev.upload(X, pad_cols=d + extra)
    wide = np.full((n, d + extra), np.nan, dtype=dtype)
    wide[:, :d] = X
    dev.copy_in(A, wide)
    assert A.ld == d + extra
    return A


def gram(dev, spec, d, A, B=None, dtype=np.float64, flags=0, pad=None):
    """g3_gram of uploaded inputs A (and B): the square covariance of A, or the cross block K(A, B); the whole padded output"""
    from g3py_amd.device import compile_spec
    n1, n2 = A.rows, (A.rows if B is None else B.rows)
    p1 = pad or n1
    p2 = (pad or n2) if B is None else n2
    out = dev.alloc(p1, p2, dtype, zero=True)
    dev.gram(compile_spec(spec, d), A, B, d, out, p1, p2, flags)
    res = dev.download(out)
    out.free()
    return res


def grad_problem(n, seed):
    """a random symmetric G and a random alpha, as tests/test_gpu_gram.py::test_gram_grad_matches_oracle"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n))
    return (A + A.T) / 2, rng.standard_normal(n)


def grad_reference(spec, X, G, alpha):
    """per slot of the oracle's dK/dparam: (leaf, name, k, 1/2 sum (alpha alpha^T - G) dK, 1/2 sum |(...) dK|)"""
    from oracle import g3_oracle as orc
    K, grads = orc.kernel_cov_grads(spec, X)
    Gfull = np.outer(alpha, alpha) - G
    return K, [(lf, pname, k, 0.5 * np.sum(Gfull * dK), 0.5 * np.sum(np.abs(Gfull * dK)) + 1e-30) for (lf, pname, k, dK) in grads]


def assert_slots(out, gmap, ref, tol, what=''):
    assert gmap.nslots == len(ref) == len(out), (what, gmap.nslots, len(ref), len(out))
    for (lf, pname, k, want, scale) in ref:
        slot = getattr(gmap, pname)[lf] + (0 if k is None else k)
        assert abs(out[slot] - want) < tol * scale, (what, lf, pname, k, out[slot], want, scale)


def posterior(spec, noise, X, y, Xs=None):
    """the oracle's Gaussian posterior as tests/test_gpu_fuzz.py::_oracle computes it, plus alpha = K^-1 y, the noise-free
    posterior covariance of the query points and the factor"""
    from oracle import g3_oracle as orc
    K = orc.tt_to_num(orc.kernel_cov(orc.with_noise(spec, noise), X))
    L = scipy.linalg.cholesky(K, lower=True)
    a = scipy.linalg.solve_triangular(L, y, lower=True)
    out = dict(K=K, L=L, logp=-0.5 * len(y) * np.log(2 * np.pi) - 0.5 * a.dot(a) - np.log(np.diag(L)).sum(),
               logdet=np.log(np.diag(L)).sum(), quad=a.dot(a), alpha=scipy.linalg.solve_triangular(L, a, lower=True, trans='T'))
    if Xs is not None:
        Ks = orc.tt_to_num(orc.kernel_cov(spec, Xs, X))
        V = scipy.linalg.solve_triangular(L, Ks.T, lower=True)
        Kss = orc.kernel_cov(spec, Xs)
        prior = np.diag(Kss)
        out.update(mean=V.T.dot(a), ss=(V ** 2).sum(0), prior=prior, variance=np.maximum(prior - (V ** 2).sum(0), 0.0),
                   cov=Kss - V.T.dot(V))
    return out
