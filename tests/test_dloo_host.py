"""CPU tests of the gradient of the leave-one-out log predictive: the closed form of tests/dloo_reference.py against central
differences of loo_reference.closed_form, the same gradient as a function of the factor through oracle.cholesky_grad, the
weight G = -2 W as g3_gp_dloo forms it (M, u, alpha on padded operands) restated in NumPy, the two new symbols and their
bindings, and the guards of GaussianProcess.dloo / dloo_chain.  No device call is made here."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import dloo_reference as dr
from loo_reference import problem
from oracle import g3_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('g3_gp_dloo', 'g3_gp_dloo_batched_fields')


@pytest.fixture(scope='module')
def lib():
    from g3py_amd import _lib
    return _lib.load()


def _se_bias(t):
    return orc.GP(('SE', t[0], t[1:3], None), t[3], ('Bias', t[4]))


def _composite(t):
    spec = ('sum', ('prod', ('MAT52', t[0], t[1:3], None), ('COS', t[3], t[4:6], None)), ('RQ', t[6], t[8:10], t[7], None))
    return orc.GP(spec, t[10], ('Bias', t[11]), ('ArcsinhLinear', t[12], t[13]))


CASES = {
    'se_noise_bias': (97, _se_bias, np.array([1.3, 0.9, 1.2, 0.1, 0.4]), False),
    'mat52cos_rq_noise_arcsinh_bias': (60, _composite, np.array([1.1, 0.9, 1.2, 1.0, 0.11, 0.07, 0.6, 1.7, 0.7, 0.5, 0.1, 0.3,
                                                                 0.1, 0.8]), True),
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_closed_form_against_central_differences(case):
    """h = 1e-6 max(1, |theta|); bound 1e-6 of the gradient's norm (measured: 5e-9 for SE + noise + Bias at N = 97)"""
    N, make, theta, warped = CASES[case]
    X, y = problem(N, seed=4)
    if warped:
        y = np.sinh(y)
    got = dr.natural_vector(dr.reference(make(theta), X, y))
    assert got.shape == theta.shape
    fd = dr.finite_difference(make, theta, X, y)
    err = np.linalg.norm(got - fd) / np.linalg.norm(fd)
    print('dloo closed form %s N=%d: rel error against central differences %.2e (bound 1e-6)\n  closed form %s\n  differences %s'
          % (case, N, err, got, fd))
    assert np.all(np.isfinite(got)) and err <= 1e-6


def test_lbar_identity_through_cholesky_grad():
    """as a function of the factor the score has Lbar = 2 tril(W L), and CholeskyRobust.grad turns it into the covariance
    adjoint of the lower convention, tril(2 W) - diag(W)"""
    N = 97
    X, y = problem(N)
    gp = _se_bias(CASES['se_noise_bias'][2])
    W = dr.weights(gp, X, y)[0]
    L = np.linalg.cholesky(np.asarray(gp.prior_kernel(X, True), dtype=np.float64))
    got = orc.cholesky_grad(L, dr.lbar(gp, X, y)(L))
    want = np.tril(2 * W) - np.diag(np.diag(W))
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print('Lbar identity N=%d: rel error %.2e (bound 1e-12)' % (N, err))
    assert err <= 1e-12


@pytest.mark.parametrize('N', [1, 97, 130])
def test_weight_as_the_device_forms_it(N):
    """G = M M^T - u alpha^T - alpha u^T with M = mirror(tril K^-1) diag(s) identity-padded to a multiple of 128, u = M t:
    -2 W on the N x N block, the identity on the padding, u = K^-1 (alpha / c) with zeros behind it"""
    X, y = problem(N)
    gp = _se_bias(CASES['se_noise_bias'][2])
    W, u, alpha, c = dr.weights(gp, X, y)
    Np = (N + 127) // 128 * 128
    A = np.linalg.inv(np.asarray(gp.prior_kernel(X, True), dtype=np.float64))
    low = np.tril(0.5 * (A + A.T))
    low[np.triu_indices(N, 1)] = np.nan                          # nothing above the diagonal is read
    s, t, ap = np.ones(Np), np.zeros(Np), np.zeros(Np)
    h = np.sqrt(c + alpha ** 2)
    s[:N], t[:N], ap[:N] = h / c, alpha / h, alpha
    M = np.eye(Np)
    i, j = np.tril_indices(N)
    M[i, j] = low[i, j]
    M[j, i] = low[i, j]
    M = M * s[None, :]
    ud = M.dot(t)
    G = M.dot(M.T) - np.outer(ud, ap) - np.outer(ap, ud)
    err = np.linalg.norm(G[:N, :N] + 2 * W) / np.linalg.norm(2 * W)
    print('G = -2 W as formed from M, u, alpha, N=%d: rel error %.2e (bound 1e-12)' % (N, err))
    assert err <= 1e-12
    assert np.array_equal(G[N:, N:], np.eye(Np - N)) and not G[N:, :N].any() and not ud[N:].any()
    np.testing.assert_allclose(ud[:N], u, rtol=0, atol=1e-12 * np.abs(u).max())


def _prototype(name):
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'g3hip.h')).read(), flags=re.S)
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, header)
    assert m, '%s is not declared in include/g3hip.h' % name
    return [' '.join(a.split()) for a in m.group(1).split(',')]


def test_symbols_in_library_header_and_signature_table(lib):
    from g3py_amd import _lib

    def ctype(decl):
        if 'g3_kernel_prog*' in decl:
            return C.POINTER(_lib.KernelProg)
        if 'g3_grad_map*' in decl:
            return C.POINTER(_lib.GradMap)
        if decl.startswith('double*'):
            return C.POINTER(C.c_double)
        if '*' in decl:
            return C.c_void_p
        if decl.startswith('int64_t'):
            return C.c_int64
        assert decl.startswith('int ') or decl.startswith('g3_dtype '), decl
        return C.c_int
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.EXPORTS
        f = getattr(lib, name)
        assert list(f.argtypes) == [ctype(d) for d in _prototype(name)], name
        assert f.restype is C.c_int
    assert len(lib.g3_gp_dloo.argtypes) == 20 and len(lib.g3_gp_dloo_batched_fields.argtypes) == 23
    assert lib.g3_version() >= 104


def test_null_context(lib):
    assert lib.g3_gp_dloo(None, None, None, None, 0, 0, 0, None, 0, None, None, 0, None, 0, None, 0, None, None, None, None) == -1
    assert lib.g3_gp_dloo_batched_fields(None, None, 0, None, None, 0, None, None, 0, 0, 0, None, 0, 0, None, None, 0, None, None,
                                         None, None, None, None) == -1


def test_signatures_and_guards():
    import g3py_amd as g3
    sig = inspect.signature(g3.GaussianProcess.dloo)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [('params', None), ('inputs', None), ('outputs', None)]
    sig = inspect.signature(g3.GaussianProcess.dloo_chain)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [('chain', inspect.Parameter.empty), ('batch', None)]
    assert g3.WarpedGaussianProcess.dloo is g3.GaussianProcess.dloo
    for cls in (g3.StudentTProcess, g3.WarpedStudentTProcess):        # as with loo
        assert not hasattr(cls, 'dloo') and not hasattr(cls, 'dloo_chain')
    assert list(inspect.signature(g3.Device.gp_dloo).parameters) == [
        'self', 'prog', 'gmap', 'X', 'N', 'd', 'L', 'W', 'a', 'Y', 'Kinv', 'alpha', 'kdiag', 'u']
    X, y = problem(16)
    gp = g3.GaussianProcess(space=X, location=g3.Zero(), kernel=g3.SE(X))
    with pytest.raises(g3.G3Error, match='loo needs observations'):
        gp.dloo()
    with pytest.raises(g3.G3Error, match='loo needs observations'):
        gp.dloo_chain(np.zeros((1, gp.active.ndim)))
    gp.observed(X, y)
    gp.distribute(None, 0, 1)
    with pytest.raises(g3.G3Error, match='loo runs on one GPU'):
        gp.dloo()
    with pytest.raises(g3.G3Error, match='loo runs on one GPU'):
        gp.dloo_chain(np.zeros((1, gp.active.ndim)))
