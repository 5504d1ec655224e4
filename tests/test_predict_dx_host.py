"""Host tests of the gradients with respect to the query inputs: the NumPy restatement of the leaf partials
(tests/predict_dx_reference.py) against central differences of dot_reference.kernel_cov_ext, its conventions at the kinks,
Mean.dx, and the refusals of the two entry points that need no GPU.

Bound of the difference tests: 1e-7 of max |closed form| at h = 1e-5 -- truncation h^2 k''' / 6 and rounding eps k / h are both
of order 1e-10 here; 1.8e-10 is the worst gap these inputs gave when the formulas were written."""
import os

import numpy as np
import pytest

from dot_reference import kernel_cov_ext
from predict_dx_reference import D, LEAVES, TREES, central_cov, d1, dkss

ZOO = dict(LEAVES, **TREES)


def _inputs(seed, n):
    """strictly positive (BW), no two points share a coordinate (no OU / BW / SINC ties)"""
    return np.random.default_rng(seed).uniform(0.2, 3.0, (n, D))


@pytest.mark.parametrize('name', sorted(ZOO))
def test_d1_matches_central_differences(name):
    spec = ZOO[name]
    xs, x = _inputs(1, 7), _inputs(2, 9)
    k, g = d1(spec, xs, x)
    np.testing.assert_array_equal(k, kernel_cov_ext(spec, xs, x))
    fd = central_cov(spec, xs, x, 1e-5)
    scale = np.abs(g).max()
    print('%s: max gap %.2e of max |d1 k| = %.3e (bound 1e-7)' % (name, np.abs(g - fd).max() / (scale or 1.0), scale))
    if name in ('NOISE', 'WN', 'VAR'):
        assert scale == 0.0 and not fd.any()
    else:
        assert scale > 0.0
    assert np.abs(g - fd).max() <= 1e-7 * scale


@pytest.mark.parametrize('name', sorted(ZOO))
def test_twice_d1_is_the_derivative_of_the_diagonal(name):
    spec = ZOO[name]
    xs = _inputs(3, 8)
    g = dkss(spec, xs)
    fd = np.empty_like(g)
    for c in range(D):
        up, dn = xs.copy(), xs.copy()
        up[:, c] += 1e-5
        dn[:, c] -= 1e-5
        fd[:, c] = (np.diag(kernel_cov_ext(spec, up)) - np.diag(kernel_cov_ext(spec, dn))) / 2e-5
    scale = np.abs(g).max()
    print('%s: diagonal, max gap %.2e of %.3e' % (name, np.abs(g - fd).max() / (scale or 1.0), scale))
    assert np.abs(g - fd).max() <= 1e-7 * scale


def test_conventions_at_the_kinks():
    x = np.array([[1.0, 2.0, 0.5]])
    xs = np.array([[1.0, 2.5, 0.25]])          # column 0 ties
    _, g = d1(LEAVES['OU'], xs, x)
    assert g[0, 0, 0] == 0.0 and g[0, 0, 1] < 0.0 and g[0, 0, 2] > 0.0           # -k r sign(dx), sign(0) = 0
    _, g = d1(LEAVES['SINC'], xs, x)
    assert g[0, 0, 0] == 0.0 and g[0, 0, 1] != 0.0
    _, g = d1(LEAVES['BW'], xs, x)
    np.testing.assert_allclose(g[0, 0], 0.8 * np.array([0.5 * 2.0 * 0.25, 0.0, 1.0 * 2.0]), rtol=1e-15)   # tie 1/2, xs > x: 0, xs < x: 1
    # a factor that is 0 does not poison the others: cos(2 pi f dx) = 0 in column 0
    spec = ('COS', 1.0, np.array([0.25, 0.1, 0.1]), None)
    _, g = d1(spec, np.array([[1.0, 0.3, 0.2]]), np.array([[0.0, 0.0, 0.0]]))
    assert np.all(np.isfinite(g)) and abs(g[0, 0, 0]) > 0.1 and abs(g[0, 0, 1]) < 1e-15


def test_mean_dx():
    import g3py_amd as g3
    x = np.random.default_rng(0).standard_normal((5, D))
    gp = g3.GaussianProcess(space=x[:2], location=g3.Zero(), kernel=g3.SE(x))
    np.testing.assert_array_equal(gp.f_location.dx(x, {}), np.zeros((5, D)))
    gp = g3.GaussianProcess(space=x[:2], location=g3.Bias(), kernel=g3.SE(x))
    np.testing.assert_array_equal(gp.f_location.dx(x, {gp.f_location.bias.name: 0.7}), np.zeros((5, D)))
    gp = g3.GaussianProcess(space=x[:2], location=g3.Linear(x), kernel=g3.SE(x))
    loc = gp.f_location
    coeff = np.array([0.3, -0.2, 1.5])
    values = {loc.constant.name: 0.4, loc.coeff.name: coeff}
    got = loc.dx(x, values)
    np.testing.assert_array_equal(got, np.broadcast_to(coeff, (5, D)))
    fd = np.stack([(loc(x + 1e-5 * np.eye(D)[c], values) - loc(x - 1e-5 * np.eye(D)[c], values)) / 2e-5 for c in range(D)], axis=1)
    np.testing.assert_allclose(got, fd, rtol=1e-9, atol=1e-9)
    with pytest.raises(NotImplementedError):
        g3.Mean().dx(x, {})


@pytest.fixture(scope='module')
def lib():
    from g3py_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.load()


def test_null_context_is_refused(lib):
    assert lib.g3_gp_cross_dx(None, None, None, 0, 0, None, 0, 0, 0, 0, None, None, 0, None, 0, None, 0, None, None, 0) == -1
    assert lib.g3_gram_diag_dx(None, None, None, 0, 0, 0, 0, None, 0) == -1
