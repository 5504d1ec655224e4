"""Host-side checks of the chain prediction (no GPU): the batched cross entry points exist in the cross-compiled library,
the header and the ctypes table; predict_chain / average exist and route -- a plain Gaussian process to the batched block
path, warped, Student-t, transport-free fallbacks and a distributed process to the loop of single predictions; average's
arithmetic (incl. the mixture moments) against NumPy on a stubbed predict_chain."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('g3_gp_cross_batched', 'g3_gp_cross_batched_fields')


def test_entry_points_exported_declared_and_bound():
    from g3py_amd import _lib
    lib = _lib.load()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'g3hip.h')).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), 'libg3hip.so does not export ' + name
        assert re.search(r'\bint\s+%s\s*\(' % name, src), 'g3hip.h does not declare ' + name
        args, res = _lib._SIGS[name]
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype is ctypes.c_int
    # ctx, progs, batch, Xs, M, ldxs, X, N, ldx, d, L, ldl, kstride, invd, a, dt, mu, ss, kdiag
    assert len(_lib._SIGS[NEW[0]][0]) == 19
    assert len(_lib._SIGS[NEW[1]][0]) == 22          # the template form: + fields, offsets, nfield
    # the C prototypes have as many parameters as the ctypes table
    for name in NEW:
        proto = re.search(r'\bint\s+%s\s*\((.*?)\)\s*;' % name, src, flags=re.S).group(1)
        assert len(proto.split(',')) == len(_lib._SIGS[name][0]), name
    # a null context is an error, not a crash
    assert lib.g3_gp_cross_batched(*([None] * 2 + [1, None, 1, 1, None, 1, 1, 1, None, 0, 0, None, None, 0, None, None, None])) == -1
    assert lib.g3_gp_cross_batched_fields(*([None] * 2 + [1, None, None, 0, None, 1, 1, None, 1, 1, 1, None, 0, 0, None, None, 0,
                                                           None, None, None])) == -1


def _gp(cls=None, **kw):
    import g3py_amd as g3
    x = np.linspace(0, 1, 9)[:, None]
    cls = cls or g3.GaussianProcess
    gp = cls(space=x[:4], location=g3.Bias(), kernel=g3.SE(x), **kw)
    gp.observed(x, np.sin(3 * x[:, 0]))
    return gp


def test_methods_exist_with_the_documented_signature():
    import inspect
    import g3py_amd as g3
    for cls in (g3.GaussianProcess, g3.WarpedGaussianProcess, g3.StudentTProcess):
        assert callable(getattr(cls, 'predict_chain')) and callable(getattr(cls, 'average'))
    sig = inspect.signature(g3.GaussianProcess.predict_chain)
    assert list(sig.parameters)[1:] == ['chain', 'space', 'inputs', 'outputs', 'mean', 'std', 'var', 'median', 'quantiles',
                                        'noise', 'prior', 'batch']
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d['mean'], d['std'], d['var'], d['median'], d['quantiles'], d['noise'], d['prior'], d['batch']) == \
        (True, True, False, False, False, False, False, None)
    assert inspect.signature(g3.GaussianProcess.average).parameters['mixture'].default is False
    assert hasattr(g3.Device, 'gp_cross_batched') and hasattr(g3.Device, 'gp_cross_batched_fields')


def test_average_arithmetic_and_mixture_on_a_stubbed_predict_chain():
    gp = _gp()
    rng = np.random.default_rng(0)
    R, M = 7, 4
    fake = dict(mean=rng.standard_normal((R, M)), std=rng.uniform(0.1, 1, (R, M)), variance=rng.uniform(0.1, 1, (R, M)),
                median=rng.standard_normal((R, M)))
    seen = {}

    def stub(chain, space=None, inputs=None, outputs=None, mean=True, std=True, var=False, median=False, quantiles=False,
             noise=False, prior=False, batch=None):
        seen.update(mean=mean, std=std, var=var, median=median, noise=noise, batch=batch, rows=np.asarray(chain).shape)
        keys = [k for k, on in (('mean', mean), ('variance', var), ('std', std), ('median', median)) if on]
        return {k: fake[k] for k in keys}
    gp.predict_chain = stub
    chain = np.zeros((R, gp.active.ndim))
    out = gp.average(chain, noise=True, batch=3)
    assert set(out) == {'mean', 'std'} and seen['noise'] is True and seen['batch'] == 3 and not seen['var']
    np.testing.assert_array_equal(out['mean'], fake['mean'].mean(axis=0))
    np.testing.assert_array_equal(out.std, fake['std'].mean(axis=0))
    out = gp.average(chain, mean=False, std=False, median=True, mixture=True)
    assert set(out) == {'median', 'mixture_mean', 'mixture_variance'} and seen['mean'] and seen['var']
    np.testing.assert_array_equal(out['median'], fake['median'].mean(axis=0))
    np.testing.assert_array_equal(out['mixture_mean'], fake['mean'].mean(axis=0))
    np.testing.assert_allclose(out['mixture_variance'], fake['variance'].mean(axis=0) + fake['mean'].var(axis=0), rtol=1e-15)
    out = gp.average(chain, var=True, mixture=True)
    assert set(out) == {'mean', 'variance', 'std', 'mixture_mean', 'mixture_variance'}

    class Trace:                      # anything with `.values` of the chain's shape (a DataFrame trace)
        values = np.zeros((R, gp.active.ndim + 2))
    del gp.predict_chain
    rows = gp._chain_rows(Trace())
    assert rows.shape == (R, gp.active.ndim)


def _stub_predict(gp, calls):
    def predict(params=None, space=None, inputs=None, outputs=None, mean=True, std=True, var=False, cov=False, median=False,
                quantiles=False, quantiles_noise=False, samples=0, distribution=False, prior=False, noise=False,
                simulations=None):
        row = gp.active.dict_to_array(params)
        calls.append((row.copy(), bool(noise), bool(prior)))
        out = {}
        if mean:
            out['mean'] = np.full(4, row.sum())
        if var:
            out['variance'] = np.full(4, (row ** 2).sum())
        if std:
            out['std'] = np.full(4, np.sqrt((row ** 2).sum()))
        return out
    gp.predict = predict


def test_fallback_routing_to_the_loop_of_single_predictions():
    import g3py_amd as g3
    rng = np.random.default_rng(1)
    made = [_gp(g3.WarpedGaussianProcess, mapping=g3.LogShifted()), _gp(g3.StudentTProcess), _gp()]
    made[2]._dist = dict(dgp=None)               # a distributed process (what distribute() leaves behind)
    for gp in made:
        assert not gp._chain_predict_batched()
        chain = rng.standard_normal((5, gp.active.ndim))
        calls = []
        _stub_predict(gp, calls)

        def boom(*a, **k):
            raise AssertionError('the batched block path must not be taken')
        gp._predict_chain_blocks = boom
        out = gp.predict_chain(chain, var=True, noise=True)
        assert len(calls) == 5 and all(c[1] and not c[2] for c in calls)
        np.testing.assert_array_equal(np.stack([c[0] for c in calls]), chain)
        assert set(out) == {'mean', 'variance', 'std'} and out['mean'].shape == (5, 4)
        np.testing.assert_allclose(out['mean'][:, 0], chain.sum(axis=1))
        np.testing.assert_allclose(out['variance'][:, 0], (chain ** 2).sum(axis=1))
        avg = gp.average(chain, std=False)
        np.testing.assert_allclose(avg['mean'], np.full(4, chain.sum(axis=1).mean()))


def test_plain_gaussian_process_takes_the_block_path():
    gp = _gp()
    assert gp._chain_predict_batched()
    got = {}

    def blocks(rows, space, inputs, outputs, switches, noise, prior, batch):
        got.update(rows=rows, switches=switches, noise=noise, prior=prior, batch=batch)
        return 'blocks'
    gp._predict_chain_blocks = blocks
    gp.predict = None                            # the loop would fail
    chain = np.arange(2.0 * gp.active.ndim).reshape(2, -1)
    assert gp.predict_chain(chain, quantiles=True, batch=1) == 'blocks'
    assert got['switches'] == dict(mean=True, std=True, var=False, median=False, quantiles=True)
    assert got['batch'] == 1 and got['prior'] is False and got['noise'] is False
    np.testing.assert_array_equal(got['rows'], chain)
    # nothing observed: the prior, as predict does (stochastic.py:475-476)
    gp.is_observed = False
    gp.predict_chain(chain)
    assert got['prior'] is True
    # a Gaussian process with a warping of its observations has no row form of the forward map: the loop
    import g3py_amd as g3
    assert not _gp(mapping=g3.LinearMapping())._chain_predict_batched()
