"""CPU tests of leave-fold-out cross-validation: the new symbol and its bindings, the fold parser and its refusals, the closed
form of tests/cv_reference.py against per-fold refits of the oracle's GP, and the O(N) host assembly
(g3py_amd.processes.gaussian.cv_assemble) fed with the reference's resid / pvar.  No device call is made here."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from cv_reference import closed_form, refits
from loo_reference import problem
from oracle import g3_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 60
CONTIGUOUS = 4
INTERLEAVED = np.arange(N) % 5


@pytest.fixture(scope='module')
def lib():
    from g3py_amd import _lib
    return _lib.load()


def test_symbol_in_library_header_and_signature_table(lib):
    from g3py_amd import _lib
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'g3hip.h')).read(), flags=re.S)
    assert hasattr(lib, 'g3_gp_cv') and 'g3_gp_cv' in _lib.EXPORTS and re.search(r'\bg3_gp_cv\s*\(', header)
    assert lib.g3_version() >= 105
    assert lib.g3_gp_cv(None, None, 0, 0, None, None, 0, None, 0, None, 0, None, None, None, 0, None, None, None, None) == -1


def test_signatures():
    import g3py_amd as g3
    sig = inspect.signature(g3.GaussianProcess.cv)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ('params', None), ('folds', 5), ('inputs', None), ('outputs', None), ('mean', True), ('std', True), ('var', False),
        ('median', False), ('logpred', True)]
    assert g3.WarpedGaussianProcess.cv is g3.GaussianProcess.cv
    assert not hasattr(g3.StudentTProcess, 'cv') and hasattr(g3.Device, 'gp_cv')


# ---------------------------------------------------------------------------------------------- folds
def test_fold_parsing():
    from g3py_amd.processes.gaussian import parse_folds
    got = parse_folds(4, 10)
    assert [f.tolist() for f in got] == [[0, 1, 2], [3, 4, 5], [6, 7], [8, 9]] and all(f.dtype == np.int64 for f in got)
    assert [f.tolist() for f in parse_folds(np.int64(3), 3)] == [[0], [1], [2]]
    assert [len(f) for f in parse_folds(5, 3)] == [1, 1, 1, 0, 0]                       # an empty fold is a fold
    labels = np.array([2, -1, 0, 2, 0, -7, 9])
    assert [f.tolist() for f in parse_folds(labels, 7)] == [[2, 4], [0, 3], [6]]        # in the order of the labels
    assert [f.tolist() for f in parse_folds(labels.tolist(), 7)] == [[2, 4], [0, 3], [6]]
    seq = [np.array([5, 1]), [], [0, 6, 2]]
    assert [f.tolist() for f in parse_folds(seq, 7)] == [[5, 1], [], [0, 6, 2]]         # as given: order kept, not sorted
    assert [f.tolist() for f in parse_folds([[0, 1], [2, 3]], 7)] == [[0, 1], [2, 3]]   # equal sizes: still index arrays
    assert [f.tolist() for f in parse_folds([np.arange(7)], 7)] == [list(range(7))]
    assert len(parse_folds([[i] for i in range(7)], 7)) == 7
    assert len(parse_folds(4096, 5000)) == 4096


def test_fold_refusals_name_the_first_offence():
    from g3py_amd.processes.gaussian import parse_folds
    with pytest.raises(ValueError, match='overlap'):
        parse_folds([[0, 1], [2, 1], [99]], 7)              # the overlap comes before the index out of range
    with pytest.raises(ValueError, match='out of range'):
        parse_folds([[0, 7], [0]], 7)                       # and here the other way round
    with pytest.raises(ValueError, match='out of range'):
        parse_folds([[0, -1]], 7)
    with pytest.raises(ValueError, match='more than 4096 folds'):
        parse_folds(4097, 10000)
    with pytest.raises(ValueError, match='more than 4096 folds'):
        parse_folds(np.arange(5000), 5000)
    with pytest.raises(ValueError, match='more than 4096 folds'):
        parse_folds([[i] for i in range(4097)], 5000)
    with pytest.raises(ValueError, match='at least one fold'):
        parse_folds(0, 7)
    with pytest.raises(ValueError, match='at least one fold'):
        parse_folds([], 7)
    with pytest.raises(ValueError, match='fold labels for'):
        parse_folds(np.zeros(6, dtype=int), 7)
    with pytest.raises(ValueError, match='integers'):
        parse_folds(np.zeros(7), 7)
    for bad in ('kfold', None, 2.5, True, {0: [1]}):
        with pytest.raises(ValueError):
            parse_folds(bad, 7)


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_fold_validation_under_asan_ubsan(tmp_path):
    """the entry point's own fold checks and launch groups (g3_host.h: plain C++, no GPU call before they pass) as a
    stand-alone program under g++ -fsanitize=address,undefined: tests/host_asan/cv_folds.cpp"""
    exe = str(tmp_path / 'cv_folds')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'g3py_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'host_asan', 'cv_folds.cpp'), '-o', exe])
    env = dict(os.environ)
    env.pop('LD_PRELOAD', None)            # ASan must come first in the link order of the test binary
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'cv_folds ok' in r.stdout


# ---------------------------------------------------------------------------------------------- reference against reference
def _se(noise=0.1, **kw):
    return orc.GP(('SE', 1.3, np.array([0.9, 1.2]), None), noise, **kw)


@pytest.fixture(scope='module')
def plain():
    X, y = problem(N)
    return X, y, _se()


@pytest.mark.parametrize('folds', [CONTIGUOUS, INTERLEAVED], ids=['contiguous', 'interleaved'])
def test_closed_form_equals_the_refits(plain, folds):
    X, y, gp = plain
    cf, rf = closed_form(gp, X, y, folds), refits(gp, X, y, folds)
    print('cv closed form against refits: loc %.2e var %.2e logpredictive %.2e joint %.2e' % (
        np.abs(cf['loc'] - rf['loc']).max(), np.abs(cf['var'] / rf['var'] - 1).max(),
        abs(cf['logpredictive'] / rf['logpredictive'] - 1), abs(cf['logpredictive_joint'] / rf['logpredictive_joint'] - 1)))
    np.testing.assert_allclose(cf['loc'], rf['loc'], rtol=0, atol=1e-10)
    np.testing.assert_allclose(cf['var'], rf['var'], rtol=1e-10)
    assert abs(cf['logpredictive'] - rf['logpredictive']) <= 1e-10 * abs(rf['logpredictive'])
    assert abs(cf['logpredictive_joint'] - rf['logpredictive_joint']) <= 1e-10 * abs(rf['logpredictive_joint'])


def test_limits_of_the_closed_form(plain):
    """N folds of one point is leave-one-out; one fold of everything is the prior, its joint score loglike"""
    from loo_reference import closed_form as loo_closed_form
    X, y, gp = plain
    _, _, loc, var, lp = loo_closed_form(gp, X, y)
    cf = closed_form(gp, X, y, N)
    np.testing.assert_allclose(cf['loc'], loc, rtol=0, atol=1e-12)
    np.testing.assert_allclose(cf['var'], var, rtol=1e-12)
    assert abs(cf['logpredictive'] - lp) <= 1e-12 * abs(lp) and abs(cf['logpredictive_joint'] - lp) <= 1e-12 * abs(lp)
    ll = gp.loglike(X, y)
    assert abs(closed_form(gp, X, y, 1)['logpredictive_joint'] - ll) <= 1e-10 * abs(ll)


# ---------------------------------------------------------------------------------------------- the assembly
KEYS = ['mean', 'variance', 'std', 'median', 'logpredictive', 'logpredictive_joint', 'folds', 'info']


def test_assembly_plain_gp_reproduces_the_refits(plain):
    import g3py_amd as g3
    from g3py_amd.processes.gaussian import cv_assemble, parse_folds
    X, y, gp = plain
    labels = INTERLEAVED.copy()
    labels[::7] = -1                                       # some observations in no fold
    fl = parse_folds(labels, N)
    cf, rf = closed_form(gp, X, y, labels), refits(gp, X, y, labels)
    out = np.isin(np.arange(N), np.concatenate(fl), invert=True)
    r = cv_assemble(np.nan_to_num(cf['resid']), np.nan_to_num(cf['pvar']), cf['fold'], np.zeros(len(fl), dtype=np.int32), fl, y,
                    g3.Identity(), {}, y, var=True, median=True)
    assert list(r) == KEYS
    for k in ('mean', 'variance', 'std', 'median'):
        assert r[k].shape == (N,) and np.all(np.isnan(r[k][out])) and np.all(np.isfinite(r[k][~out]))
    np.testing.assert_allclose(r.mean[~out], rf['mean'][~out], rtol=0, atol=1e-10)
    np.testing.assert_allclose(r.median[~out], rf['median'][~out], rtol=0, atol=1e-10)
    np.testing.assert_allclose(r.variance[~out], rf['variance'][~out], rtol=1e-10)
    np.testing.assert_allclose(r.std[~out], np.sqrt(rf['variance'][~out]), rtol=1e-10)
    assert abs(r.logpredictive - rf['logpredictive']) <= 1e-10 * abs(rf['logpredictive'])
    assert abs(r.logpredictive_joint - rf['logpredictive_joint']) <= 1e-10 * abs(rf['logpredictive_joint'])
    assert [f.tolist() for f in r.folds] == [f.tolist() for f in fl] and np.all(r.info == 0)
    # only what was asked for; a fold with a pivot flag: both scores take the sentinel, the curves stay
    args = (np.nan_to_num(cf['resid']), np.nan_to_num(cf['pvar']), cf['fold'])
    assert list(cv_assemble(*args, np.zeros(len(fl)), fl, y, g3.Identity(), {}, y, std=False, logpred=False)) == ['mean', 'folds', 'info']
    info = np.zeros(len(fl), dtype=np.int32)
    info[2] = 17
    rb = cv_assemble(*args, info, fl, y, g3.Identity(), {}, y)
    assert rb.logpredictive == np.float32(-1e30) and rb.logpredictive_joint == np.float32(-1e30) and rb.info[2] == 17


def test_assembly_warped_gp():
    import g3py_amd as g3
    from g3py_amd.processes.gaussian import cv_assemble, parse_folds
    X, y = problem(N, seed=1)
    y = np.abs(y) + 0.5                                        # inside BoxCox's domain
    gp = _se(mean=('Bias', 0.2), mapping=('BoxCoxLinear', 1.0, 1.0, 1.2))
    fl = parse_folds(CONTIGUOUS, N)
    cf, rf = closed_form(gp, X, y, CONTIGUOUS), refits(gp, X, y, CONTIGUOUS)
    x = np.linspace(0, 1, 8)[:, None]
    wgp = g3.WarpedGaussianProcess(space=x, location=g3.Bias(), kernel=g3.SE(x), mapping=g3.BoxCoxLinear())
    values = {'WGP_BoxCoxLinear_shift': 1.0, 'WGP_BoxCoxLinear_scale': 1.0, 'WGP_BoxCoxLinear_power': 1.2}
    z = wgp.f_mapping.inv(y, values)
    r = cv_assemble(cf['resid'], cf['pvar'], cf['fold'], np.zeros(len(fl), dtype=np.int32), fl, z, wgp.f_mapping, values, y,
                    hermite=wgp._LOO_HERMITE, var=True, median=True)
    assert list(r) == KEYS
    scale = max(1.0, np.abs(rf['mean']).max())
    np.testing.assert_allclose(r.mean, rf['mean'], rtol=0, atol=1e-10 * scale)
    np.testing.assert_allclose(r.median, rf['median'], rtol=0, atol=1e-10 * scale)
    np.testing.assert_allclose(r.variance, rf['variance'], rtol=0, atol=1e-10 * scale ** 2)
    np.testing.assert_allclose(r.std, np.sqrt(rf['variance']), rtol=0, atol=1e-10 * scale)
    assert abs(r.logpredictive - rf['logpredictive']) <= 1e-10 * abs(rf['logpredictive'])
    assert abs(r.logpredictive_joint - rf['logpredictive_joint']) <= 1e-10 * abs(rf['logpredictive_joint'])


# ---------------------------------------------------------------------------------------------- guards
def test_cv_without_a_gpu_raises_g3error():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    import g3py_amd as g3
    X, y = problem(16)
    gp = g3.GaussianProcess(space=X, location=g3.Zero(), kernel=g3.SE(X))
    gp.observed(X, y)
    with pytest.raises(g3.G3Error):
        gp.cv()
    with pytest.raises(g3.G3Error):
        gp.scores(cv=4)


def test_cv_is_refused_on_a_distributed_process_and_without_observations():
    import g3py_amd as g3
    X, y = problem(16)
    gp = g3.GaussianProcess(space=X, location=g3.Zero(), kernel=g3.SE(X))
    with pytest.raises(g3.G3Error, match='cv needs observations'):
        gp.cv()
    gp.observed(X, y)
    gp.distribute(None, 0, 1)
    tp = g3.StudentTProcess(space=X, location=g3.Zero(), kernel=g3.SE(X))
    tp.observed(X, y)
    tp.predict = lambda *a, **k: g3.libs.DictObj(mean=np.zeros(len(X)))      # scores' own prediction needs a device
    tp.hidden = np.zeros(len(X))
    with pytest.raises(g3.G3Error, match='not available for StudentTProcess'):
        tp.scores(cv=4)
    with pytest.raises(g3.G3Error, match='cv runs on one GPU'):
        gp.cv()
