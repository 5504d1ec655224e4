"""Host-side checks of the chain draws (no GPU): the batched robust factor and the batched draws entry points exist in the
cross-compiled library, the header and the ctypes table; sample_chain / particles exist with the documented signatures
and route -- a plain Gaussian process to the batched block path, warped, Student-t and distributed processes to the loop
of single sampler calls; particles cycles over the rows, concatenates and validates `rand` on a stubbed sample_chain."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('g3_potrf_robust_batched', 'g3_gp_draws_batched', 'g3_gp_draws_batched_fields')


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
        proto = re.search(r'\bint\s+%s\s*\((.*?)\)\s*;' % name, src, flags=re.S).group(1)
        assert len(proto.split(',')) == len(args), name
    # ctx, K, ldk, kstride, L, ldl, lstride, batch, n, dt, maxtries, tries, fallback, jitter
    assert len(_lib._SIGS[NEW[0]][0]) == 14
    # ctx, progs, batch, Xs, M, ldxs, X, N, ldx, d, L, ldl, kstride, invd, a, dt, lift, loc, Z, S, out, C, Lp, maxtries,
    # tries, fallback, jitter
    assert len(_lib._SIGS[NEW[1]][0]) == 27
    assert len(_lib._SIGS[NEW[2]][0]) == 30          # the template form: + fields, offsets, nfield
    # a null context is an error, not a crash
    assert lib.g3_potrf_robust_batched(None, None, 1, 1, None, 128, 128 * 128, 1, 1, 0, 20, None, None, None) == -1
    tail = [None, 0, 0, None, None, 0, 0, None, None, 1, None, None, None, 20, None, None, None]
    assert lib.g3_gp_draws_batched(*([None, None, 1, None, 1, 1, None, 1, 1, 1] + tail)) == -1
    assert lib.g3_gp_draws_batched_fields(*([None, None, 1, None, None, 0, None, 1, 1, None, 1, 1, 1] + tail)) == -1


def _gp(cls=None, **kw):
    import g3py_amd as g3
    x = np.linspace(0, 1, 9)[:, None]
    cls = cls or g3.GaussianProcess
    gp = cls(space=x[:4], location=g3.Bias(), kernel=g3.SE(x), **kw)
    gp.observed(x, np.sin(3 * x[:, 0]))
    return gp


def test_methods_exist_with_the_documented_signatures():
    import g3py_amd as g3
    for cls in (g3.GaussianProcess, g3.WarpedGaussianProcess, g3.StudentTProcess):
        assert callable(getattr(cls, 'sample_chain')) and callable(getattr(cls, 'particles'))
    sig = inspect.signature(g3.GaussianProcess.sample_chain)
    assert list(sig.parameters)[1:] == ['chain', 'space', 'inputs', 'outputs', 'samples', 'prior', 'noise', 'rand', 'batch',
                                        'return_info']
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d['space'], d['inputs'], d['outputs'], d['samples'], d['prior'], d['noise'], d['rand'], d['batch'],
            d['return_info']) == (None, None, None, 1, False, False, None, None, False)
    sig = inspect.signature(g3.GaussianProcess.particles)
    assert list(sig.parameters)[1:] == ['chain', 'nsamples', 'space', 'inputs', 'outputs', 'samples', 'prior', 'noise', 'rand',
                                        'batch']
    d = {k: p.default for k, p in sig.parameters.items()}
    assert (d['nsamples'], d['samples'], d['prior'], d['noise'], d['rand'], d['batch']) == (None, 1, False, False, None, None)
    kinds = {k: p.kind for k, p in sig.parameters.items()}
    assert kinds['nsamples'] is inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert all(kinds[k] is inspect.Parameter.KEYWORD_ONLY for k in list(sig.parameters)[3:])
    for name in ('potrf_robust_batched', 'gp_draws_batched', 'gp_draws_batched_fields'):
        assert hasattr(g3.Device, name)
    # predict_chain and average keep their signatures
    assert list(inspect.signature(g3.GaussianProcess.predict_chain).parameters)[1:] == \
        ['chain', 'space', 'inputs', 'outputs', 'mean', 'std', 'var', 'median', 'quantiles', 'noise', 'prior', 'batch']
    assert list(inspect.signature(g3.GaussianProcess.average).parameters)[-1] == 'mixture'


def test_plain_gaussian_process_takes_the_block_path():
    gp = _gp()
    assert gp._chain_predict_batched()
    got = {}

    def blocks(rows, space, inputs, outputs, rand, noise, prior, batch):
        got.update(rows=rows, rand=rand, noise=noise, prior=prior, batch=batch, space=space)
        n = len(rows)
        return np.zeros((n, 4, rand.shape[2])), np.arange(n), np.zeros(n, bool), np.ones(n)
    gp._sample_chain_blocks = blocks
    gp.sampler = None                            # the loop would fail
    chain = np.arange(3.0 * gp.active.ndim).reshape(3, -1)
    rand = np.random.default_rng(0).standard_normal((3, 4, 2))
    out, info = gp.sample_chain(chain, samples=2, noise=True, rand=rand, batch=2, return_info=True)
    assert out.shape == (3, 4, 2) and got['noise'] is True and got['prior'] is False and got['batch'] == 2
    np.testing.assert_array_equal(got['rows'], chain)
    np.testing.assert_array_equal(got['rand'], rand)
    np.testing.assert_array_equal(info['tries'], np.arange(3))
    assert set(info) == {'tries', 'fallback', 'jitter'}
    # the default normals: randn(rows, M, samples) takes from the global stream what the loop's randn(M, samples) calls take
    np.random.seed(5)
    want = np.stack([np.random.randn(4, 3) for _ in range(3)])
    np.random.seed(5)
    assert gp.sample_chain(chain, samples=3).shape == (3, 4, 3)
    np.testing.assert_array_equal(got['rand'], want)
    with pytest.raises(ValueError):
        gp.sample_chain(chain, samples=2, rand=np.zeros((3, 4, 1)))
    # nothing observed: the prior, as predict does
    gp.is_observed = False
    gp.sample_chain(chain)
    assert got['prior'] is True


def test_fallback_routing_to_the_loop_of_single_sampler_calls():
    import g3py_amd as g3
    rng = np.random.default_rng(1)
    made = [_gp(g3.WarpedGaussianProcess, mapping=g3.LogShifted()), _gp(g3.StudentTProcess), _gp()]
    made[2]._dist = dict(dgp=None)               # a distributed process (what distribute() leaves behind)
    for gp in made:
        assert not gp._chain_predict_batched()
        chain = rng.standard_normal((5, gp.active.ndim))
        calls = []

        def sampler(params=None, space=None, inputs=None, outputs=None, samples=1, prior=False, noise=False, rand=None,
                    _gp=gp, _calls=calls):
            row = _gp.active.dict_to_array(params)
            _calls.append((row.copy(), samples, bool(prior), bool(noise), rand))
            return np.full((4, samples), row.sum())
        gp.sampler = sampler

        def boom(*a, **k):
            raise AssertionError('the batched block path must not be taken')
        gp._sample_chain_blocks = boom
        rand = rng.standard_normal((5, 4, 2))
        out, info = gp.sample_chain(chain, samples=2, noise=True, rand=rand, return_info=True)
        assert out.shape == (5, 4, 2) and len(calls) == 5 and info['tries'] is None
        np.testing.assert_array_equal(np.stack([c[0] for c in calls]), chain)
        assert all(c[1] == 2 and not c[2] and c[3] for c in calls)
        for i, c in enumerate(calls):
            np.testing.assert_array_equal(c[4], rand[i])
        np.testing.assert_allclose(out[:, 0, 0], chain.sum(axis=1))
        # without `rand` every sampler call draws its own normals, in the loop's order
        del calls[:]
        gp.sample_chain(chain)
        assert len(calls) == 5 and all(c[4] is None for c in calls)


def test_particles_cycles_concatenates_and_validates_rand():
    gp = _gp()
    R, M, S = 3, 4, 2
    chain = np.arange(float(R * gp.active.ndim)).reshape(R, -1)
    seen = {}

    def stub(rows, space=None, inputs=None, outputs=None, samples=1, prior=False, noise=False, rand=None, batch=None,
             return_info=False):
        rows = np.asarray(rows)
        seen.update(rows=rows.copy(), samples=samples, prior=prior, noise=noise, rand=rand, batch=batch)
        # draw (i, m, s) = 100 * first parameter of the row + 10 * m + s
        return rows[:, 0][:, None, None] * 100 + 10 * np.arange(M)[None, :, None] + np.arange(samples)[None, None, :]
    gp.sample_chain = stub
    for ns in (2, R, R + 2, None):               # below, equal to and above the row count; the default: one per row
        out = gp.particles(chain, ns, samples=S, noise=True, batch=7)
        n = R if ns is None else ns
        assert out.shape == (M, n * S) and seen['samples'] == S and seen['noise'] is True and seen['batch'] == 7
        picked = chain[np.arange(n) % R]
        np.testing.assert_array_equal(seen['rows'], picked)
        for i in range(n):
            for s in range(S):
                np.testing.assert_array_equal(out[:, i * S + s], picked[i, 0] * 100 + 10 * np.arange(M) + s)
    rand = np.zeros((R + 2, M, S))
    gp.particles(chain, R + 2, samples=S, rand=rand)
    assert seen['rand'] is rand
    with pytest.raises(ValueError):
        gp.particles(chain, R + 2, samples=S, rand=np.zeros((R, M, S)))
    with pytest.raises(ValueError):
        gp.particles(np.zeros((0, gp.active.ndim)), 2)
    assert gp.particles(chain, 0).shape == (M, 0)
    with pytest.raises(TypeError):
        gp.particles(chain, 2, chain[:2])        # everything after nsamples is keyword-only
