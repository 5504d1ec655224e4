"""CPU tests of leave-one-out cross-validation: the two new symbols and their bindings, the signatures of loo / loo_chain /
scores(loo=...), and the O(N) host assembly (g3py_amd.processes.gaussian.loo_assemble) fed with alpha and kdiag from
np.linalg.inv against N refits of the oracle's GP (tests/loo_reference.py).  No device call is made here."""
import inspect
import os
import re

import numpy as np
import pytest

from loo_reference import brute_force, closed_form, problem
from oracle import g3_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 97


@pytest.fixture(scope='module')
def lib():
    from g3py_amd import _lib
    return _lib.load()


def test_symbols_in_library_header_and_signature_table(lib):
    from g3py_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'g3hip.h')).read(), flags=re.S)
    for name in ('g3_gp_loo', 'g3_gp_loo_batched'):
        assert hasattr(lib, name)
        assert name in _lib.EXPORTS
        assert re.search(r'\b%s\s*\(' % name, header)
    assert lib.g3_version() >= 102


def test_null_context_and_argument_checks(lib):
    assert lib.g3_gp_loo(None, None, 0, 0, None, None, 0, None, 0, None, None) == -1
    assert lib.g3_gp_loo_batched(None, 1, None, 0, 0, 0, None, None, 0, None, None, None) == -1


def test_signatures():
    import g3py_amd as g3
    sig = inspect.signature(g3.GaussianProcess.loo)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ('params', None), ('inputs', None), ('outputs', None), ('mean', True), ('std', True), ('var', False),
        ('median', False), ('logpred', True)]
    assert g3.WarpedGaussianProcess.loo is g3.GaussianProcess.loo
    sig = inspect.signature(g3.GaussianProcess.loo_chain)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [('chain', inspect.Parameter.empty), ('batch', None)]
    par = inspect.signature(g3.GaussianProcess.scores).parameters
    assert list(par)[-4:] == ['median', 'args', 'loo', 'kwargs']       # one keyword behind the existing ones ...
    assert par['loo'].default is False and par['loo'].kind is inspect.Parameter.KEYWORD_ONLY     # ... that no positional argument can set
    assert not hasattr(g3.StudentTProcess, 'loo') and not hasattr(g3.StudentTProcess, 'loo_chain')
    assert hasattr(g3.Device, 'gp_loo') and hasattr(g3.Device, 'gp_loo_batched')


def _se(noise=0.1, **kw):
    return orc.GP(('SE', 1.3, np.array([0.9, 1.2]), None), noise, **kw)


@pytest.fixture(scope='module')
def plain():
    X, y = problem(N)
    gp = _se()
    return X, y, gp, closed_form(gp, X, y), brute_force(gp, X, y)


def test_assembly_plain_gp_reproduces_the_refits(plain):
    import g3py_amd as g3
    from g3py_amd.processes.gaussian import loo_assemble
    X, y, gp, (alpha, c, loc, var, lp), bf = plain
    # the identity itself, reference against reference
    np.testing.assert_allclose(loc, bf['loc'], rtol=0, atol=1e-10)
    np.testing.assert_allclose(var, bf['var'], rtol=1e-10)
    assert abs(lp - bf['logpredictive']) <= 1e-10 * abs(bf['logpredictive'])
    r = loo_assemble(alpha, c, y, g3.Identity(), {}, y=y, mean=True, std=True, var=True, median=True)
    assert list(r) == ['mean', 'variance', 'std', 'median', 'logpredictive']
    np.testing.assert_allclose(r.mean, bf['mean'], rtol=0, atol=1e-10)
    np.testing.assert_allclose(r.median, bf['median'], rtol=0, atol=1e-10)
    np.testing.assert_allclose(r.variance, bf['variance'], rtol=1e-10)
    np.testing.assert_allclose(r.std, np.sqrt(bf['variance']), rtol=1e-10)
    assert abs(r.logpredictive - bf['logpredictive']) <= 1e-10 * abs(bf['logpredictive'])
    # only what was asked for
    assert list(loo_assemble(alpha, c, y, g3.Identity(), {}, y=y, mean=False, std=False)) == ['logpredictive']
    assert list(loo_assemble(alpha, c, y, g3.Identity(), {}, y=y, std=False, logpred=False)) == ['mean']


def test_assembly_rows_form_equals_row_by_row(plain):
    """the chain form: (B, N) vectors in, one logpredictive per row out"""
    import g3py_amd as g3
    from g3py_amd.processes.gaussian import loo_assemble
    X, y, gp, (alpha, c, loc, var, lp), bf = plain
    A = np.stack([alpha, 0.5 * alpha, alpha])
    C = np.stack([c, 2.0 * c, c])
    C[2, 3] = np.nan                                           # a row that cannot be scored
    rows = loo_assemble(A, C, np.broadcast_to(y, A.shape), g3.Identity(), {}, y=y)['logpredictive']
    assert rows.shape == (3,)
    for j in range(2):
        one = loo_assemble(A[j], C[j], y, g3.Identity(), {}, y=y)['logpredictive']
        assert abs(rows[j] - one) <= 1e-12 * abs(one)
    assert abs(rows[0] - bf['logpredictive']) <= 1e-10 * abs(bf['logpredictive'])
    assert rows[2] == np.float32(-1e30)


def test_assembly_warped_gp_and_the_sentinel_branch():
    import g3py_amd as g3
    from g3py_amd.processes.gaussian import loo_assemble
    X, y = problem(N, seed=1)
    y = np.abs(y) + 0.5                                        # inside BoxCox's domain
    spec = ('BoxCoxLinear', 1.0, 1.0, 1.2)
    gp = _se(mean=('Bias', 0.2), mapping=spec)
    alpha, c, loc, var, lp = closed_form(gp, X, y)
    bf = brute_force(gp, X, y)
    x = np.linspace(0, 1, 8)[:, None]
    wgp = g3.WarpedGaussianProcess(space=x, location=g3.Bias(), kernel=g3.SE(x), mapping=g3.BoxCoxLinear())
    values = {'WGP_BoxCoxLinear_shift': 1.0, 'WGP_BoxCoxLinear_scale': 1.0, 'WGP_BoxCoxLinear_power': 1.2}
    z = wgp.f_mapping.inv(y, values)
    np.testing.assert_allclose(z, gp.mapping_outputs(y), rtol=0, atol=1e-14)
    assert wgp._LOO_HERMITE == 10 and g3.GaussianProcess._LOO_HERMITE is None
    r = loo_assemble(alpha, c, z, wgp.f_mapping, values, y=y, hermite=wgp._LOO_HERMITE, var=True, median=True)
    scale = max(1.0, np.abs(bf['mean']).max())
    np.testing.assert_allclose(r.mean, bf['mean'], rtol=0, atol=1e-10 * scale)
    np.testing.assert_allclose(r.median, bf['median'], rtol=0, atol=1e-10 * scale)
    np.testing.assert_allclose(r.variance, bf['variance'], rtol=0, atol=1e-10 * scale ** 2)
    np.testing.assert_allclose(r.std, np.sqrt(bf['variance']), rtol=0, atol=1e-10 * scale)
    assert abs(r.logpredictive - bf['logpredictive']) <= 1e-10 * abs(bf['logpredictive'])
    # a NaN observation: logp_cho_diag's -1e30 branch, the curves from the scrubbed vector
    y_bad = y.copy()
    y_bad[5] = np.nan
    z_bad = np.where(np.isnan(wgp.f_mapping.inv(y_bad, values)), 0.0, wgp.f_mapping.inv(y_bad, values))
    rb = loo_assemble(alpha, c, z_bad, wgp.f_mapping, values, y=y_bad, hermite=10)
    assert rb.logpredictive == np.float32(-1e30)
    assert np.all(np.isfinite(rb.mean)) and np.all(np.isfinite(rb.std))


def test_loo_without_a_gpu_raises_g3error():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    import g3py_amd as g3
    X, y = problem(16)
    gp = g3.GaussianProcess(space=X, location=g3.Zero(), kernel=g3.SE(X))
    gp.observed(X, y)
    with pytest.raises(g3.G3Error):
        gp.loo()
    with pytest.raises(g3.G3Error):
        gp.loo_chain(np.zeros((2, gp.active.ndim)))
    with pytest.raises(g3.G3Error):
        gp.scores(loo=True)


def test_loo_is_refused_on_a_distributed_process_and_without_observations():
    import g3py_amd as g3
    X, y = problem(16)
    gp = g3.GaussianProcess(space=X, location=g3.Zero(), kernel=g3.SE(X))
    with pytest.raises(g3.G3Error, match='loo needs observations'):
        gp.loo()
    gp.observed(X, y)
    gp.distribute(None, 0, 1)
    tp = g3.StudentTProcess(space=X, location=g3.Zero(), kernel=g3.SE(X))
    tp.observed(X, y)
    tp.predict = lambda *a, **k: g3.libs.DictObj(mean=np.zeros(len(X)))      # scores' own prediction needs a device
    tp.hidden = np.zeros(len(X))
    with pytest.raises(g3.G3Error, match='not available for StudentTProcess'):
        tp.scores(loo=True)
    with pytest.raises(g3.G3Error, match='loo runs on one GPU'):
        gp.loo()
    with pytest.raises(g3.G3Error, match='loo runs on one GPU'):
        gp.loo_chain(np.zeros((2, gp.active.ndim)))
