"""GPU tests of the gradient of the leave-one-out log predictive: the C entry points g3_gp_dloo and
g3_gp_dloo_batched_fields, Device.gp_dloo(_batched_fields) and GaussianProcess.dloo / dloo_chain.  Reference:
tests/dloo_reference.py -- the closed form from np.linalg.inv through the oracle's kernel, mean and mapping derivatives
(checked against central differences on the CPU, test_dloo_host.py; nothing here uses finite differences).

fp64 bound: 1e-8 of the reference's norm, the project's fp64 bar.  fp32 bound: 10 x dloo_reference.fp32_gap, the measured
|closed form in float32 - in float64| / |in float64| on the same inputs; the device sums in another order than NumPy."""
import ctypes as C
import functools

import numpy as np
import pytest

import dloo_reference as dr
import hostile_memory as hm
from hostile_memory import CANARY_BYTE, NAN_BYTE
from loo_reference import problem
from oracle import g3_oracle as orc
from test_gpu_vjp import PROGRAMS

pytestmark = pytest.mark.gpu

RATE = np.array([0.9, 1.2])
SE_SPEC = ('SE', 1.3, RATE, None)
# the panel and stream thresholds of the K^-1 sweep (test_gpu_loo.py): one panel up to 128, one stream up to 256, two streams
# from 257 on; 64 x 64 tiles of the weight pass: one tile row at N = 1 .. 64, a last tile that is all padding at 129 and 257
SINGLE_N = [1, 97, 128, 129, 256, 257, 385, 1100]


def _params(gp, **nat):
    p = gp.params_test
    by = {v.name: v for v in gp.model.vars}
    for k, val in nat.items():
        v = by[gp.name + '_' + k]
        p[v.key] = (np.log(val) if v.positive else np.asarray(val, dtype=float)) * np.ones(v.shape)
    return p


def _se_gp(g3, X, y, dtype=np.float64, device=None):
    gp = g3.GaussianProcess(space=X[:2], location=g3.Zero(), kernel=g3.SE(X), dtype=dtype, device=device)
    gp.observed(X, y)
    return gp, _params(gp, SE_var=1.3, SE_rate=RATE, Noise_var=0.1)


@functools.lru_cache(maxsize=None)
def _reference(N):
    """problem and closed form of the SE + noise 0.1 process at N, computed once for all tests"""
    X, y = problem(N)
    ref = dr.reference(orc.GP(SE_SPEC, 0.1), X, y)
    vec = dr.natural_vector(ref)
    for a in (X, y, vec, ref['u'], ref['alpha'], ref['c']):
        a.setflags(write=False)
    return X, y, vec, ref['u'], ref['alpha'], ref['c']


def _rel(got, ref):
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64) - ref) / np.linalg.norm(ref))


def _entry(gp, p, Y=None, Kinv=None):
    """g3_gp_dloo on the buffers logp left; returns (slots, alpha, kdiag, u (Np entries each), Kinv (Np x Np))"""
    from g3py_amd import _lib
    gp.logp(p)
    dev, ch = gp.device, gp._cache
    N, d, Np, dt = ch['N'], ch['d'], ch['Np'], gp.dtype
    prog = gp._prog(gp.f_kernel_noise, gp._values(p)[0], d)
    gmap = dev.grad_layout(prog)
    Y = dev.alloc(Np, Np, dt) if Y is None else Y
    Kinv = dev.upload(np.full((Np, Np), 7.0, dtype=dt)) if Kinv is None else Kinv
    vecs = [dev.upload(np.full((1, Np), 7.0, dtype=dt)) for _ in range(3)]
    slots = dev.gp_dloo(prog, gmap, ch['Xd'], N, d, ch['Kd'], ch['Wd'], ch['ad'], Y, Kinv, *vecs)
    assert Np == _lib.roundup(N)
    return (slots,) + tuple(dev.download(v)[0] for v in vecs) + (dev.download(Kinv),)


# ------------------------------------------------------------------------------------------------ 1. entry point, fp64
@pytest.mark.parametrize('N', SINGLE_N)
def test_entry_point_fp64(N):
    import g3py_amd as g3
    X, y, vec, u, alpha, c = _reference(N)
    gp, p = _se_gp(g3, X, y)
    slots, a1, c1, u1, Ki = _entry(gp, p)
    err = _rel(slots, vec)
    print('g3_gp_dloo fp64 N=%d: slots %s, rel error %.2e (bound 1e-8); max rel err u %.2e alpha %.2e kdiag %.2e' % (
        N, slots, err, np.abs(u1[:N] - u).max() / np.abs(u).max(), np.abs(a1[:N] - alpha).max() / np.abs(alpha).max(),
        np.abs(c1[:N] / c - 1).max()))
    assert slots.shape == vec.shape and err <= 1e-8
    np.testing.assert_allclose(u1[:N], u, rtol=1e-8, atol=1e-8 * np.abs(u).max())
    np.testing.assert_allclose(a1[:N], alpha, rtol=1e-8, atol=1e-8 * np.abs(alpha).max())
    np.testing.assert_allclose(c1[:N], c, rtol=1e-8, atol=0)
    for v in (a1, c1, u1):
        assert len(v) == gp._cache['Np'] and np.all(v[N:] == 0.0)
    # a second call: the same bits
    slots2, a2, c2, u2, Ki2 = _entry(gp, p)
    assert np.array_equal(slots, slots2) and np.array_equal(a1, a2) and np.array_equal(c1, c2) and np.array_equal(u1, u2)
    # Kinv is what g3_gp_dlogp leaves: the lower triangle of K^-1
    dev, ch = gp.device, gp._cache
    Np = ch['Np']
    prog = gp._prog(gp.f_kernel_noise, gp._values(p)[0], ch['d'])
    Kd = dev.upload(np.full((Np, Np), 7.0))
    dev.gp_dlogp(prog, dev.grad_layout(prog), ch['Xd'], N, ch['d'], ch['Kd'], ch['Wd'], ch['ad'], dev.alloc(Np, Np, np.float64), Kd,
                 dev.alloc(1, Np, np.float64))
    low = hm.tril_mask(Np)
    hm.same_bits(np.where(low, Ki, 0.0), np.where(low, dev.download(Kd), 0.0), what='Kinv against g3_gp_dlogp')
    assert np.array_equal(Ki, Ki2)
    np.testing.assert_allclose(np.diag(Ki)[:N], c, rtol=1e-8, atol=0)


# ------------------------------------------------------------------------------------------------ 2. entry point, fp32
@pytest.mark.parametrize('N', [128, 200, 385])
def test_entry_point_fp32(N):
    import g3py_amd as g3
    X, y = problem(N, dtype=np.float32)
    gap, ref = dr.fp32_gap(orc.GP(SE_SPEC, 0.1), X, y)
    gp, p = _se_gp(g3, X, y, dtype=np.float32)
    slots, a1, c1, u1, _ = _entry(gp, p)
    err = _rel(slots, dr.natural_vector(ref))
    print('g3_gp_dloo fp32 N=%d: rel error against the float64 closed form %.3e, float32 closed form %.3e (bound 10 x)' % (N, err, gap))
    assert a1.dtype == np.float32 and np.all(u1[N:] == 0.0) and np.all(c1[N:] == 0.0) and np.all(a1[N:] == 0.0)
    assert err <= 10 * gap


# ------------------------------------------------------------------------------------------------ 3. process
def _blocks(gp, nat, parts):
    """the reference in the order and space of gp.dloo: per variable (name, natural-space gradient mapped to transformed
    space); parts: variable suffix -> natural-space gradient"""
    out = []
    for v in gp.model.vars:
        key = v.name[len(gp.name) + 1:]
        g = np.asarray(parts[key], dtype=np.float64).reshape(-1)
        if v.positive:
            g = g * np.broadcast_to(np.asarray(nat[key], dtype=np.float64), g.shape)
        assert g.size == v.size, (v.name, g.size, v.size)
        out.append((v.name, g))
    return out


def _check_blocks(got, blocks, what, bound=1e-8):
    got = np.asarray(got, dtype=np.float64)
    at = 0
    assert got.shape == (sum(len(g) for _, g in blocks),)
    for name, ref in blocks:
        g = got[at:at + len(ref)]
        at += len(ref)
        err = np.linalg.norm(g - ref) / np.linalg.norm(ref)
        print('dloo %s %s: %s reference %s rel error %.2e (bound %.1e)' % (what, name, g, ref, err, bound))
        assert err <= bound, (what, name)


def _leaf(ref, leaf, pname, nd=None):
    s = ref['slots']
    return s[(leaf, pname, None)] if nd is None else np.array([s[(leaf, pname, k)] for k in range(nd)])


def _process_case(g3, kind):
    """(gp, natural values, oracle process, X, y, reference -> parts)"""
    if kind == 'se_bias':
        N, d = 200, 2
        X, y = problem(N, seed=5)
        gp = g3.GaussianProcess(space=X[:2], location=g3.Bias(), kernel=g3.SE(X))
        nat = dict(SE_var=1.3, SE_rate=RATE, Noise_var=0.1, Bias_Bias=0.4)
        o = orc.GP(SE_SPEC, 0.1, ('Bias', 0.4))
        parts = lambda r: dict(SE_var=_leaf(r, 0, 'var'), SE_rate=_leaf(r, 0, 'rate', d), Noise_var=_leaf(r, 1, 'var'),
                               Bias_Bias=r['mean'][0][2])
    elif kind == 'composite':
        N = 150
        d, spec = PROGRAMS['mat52cos_rq_noise']
        X, y = problem(N, d=d, seed=6)
        gp = g3.GaussianProcess(space=X[:2], location=g3.Zero(), kernel=g3.MAT52(X) * g3.COS(X) + g3.RQ(X))
        (_, (_, m52, cos), rq), noise = spec[1], spec[2]
        nat = dict(MAT52_var=m52[1], MAT52_rate=m52[2], COS_freq=cos[2], RQ_var=rq[1], RQ_rate=rq[2], RQ_alpha=rq[3], Noise_var=noise[1])
        o = orc.GP(spec[1], noise[1])
        parts = lambda r: dict(MAT52_var=_leaf(r, 0, 'var'), MAT52_rate=_leaf(r, 0, 'rate', d), COS_freq=_leaf(r, 1, 'freq', d),
                               RQ_var=_leaf(r, 2, 'var'), RQ_alpha=_leaf(r, 2, 'alpha'), RQ_rate=_leaf(r, 2, 'rate', d),
                               Noise_var=_leaf(r, 3, 'var'))
    else:
        N, d = 200, 2
        X, y = problem(N, seed=3)
        y = np.sinh(y)
        gp = g3.WarpedGaussianProcess(space=X[:2], location=g3.Zero(), kernel=g3.SE(X), mapping=g3.ArcsinhLinear())
        nat = dict(SE_var=1.3, SE_rate=RATE, Noise_var=0.1, ArcsinhLinear_shift=0.1, ArcsinhLinear_scale=0.8)
        o = orc.GP(SE_SPEC, 0.1, ('Zero',), ('ArcsinhLinear', 0.1, 0.8))
        parts = lambda r: dict(SE_var=_leaf(r, 0, 'var'), SE_rate=_leaf(r, 0, 'rate', d), Noise_var=_leaf(r, 1, 'var'),
                               ArcsinhLinear_shift=r['mapping'][0][1], ArcsinhLinear_scale=r['mapping'][1][1])
    gp.observed(X, y)
    return gp, nat, o, X, y, parts


@pytest.mark.parametrize('kind', ['se_bias', 'composite', 'warped'])
def test_process_dloo_matches_the_closed_form(kind):
    import g3py_amd as g3
    gp, nat, o, X, y, parts = _process_case(g3, kind)
    p = _params(gp, **nat)
    before = gp.device.grad_path_stats()
    got = gp.dloo(p)
    after = gp.device.grad_path_stats()
    assert got.dtype == np.float64 and got.shape == (gp.active.ndim,)
    _check_blocks(got, _blocks(gp, nat, parts(dr.reference(o, X, y))), kind)
    step = {k: after[k] - before[k] for k in after}
    print('dloo %s: gradient paths %s' % (kind, step))
    # SE (+ noise) takes the compile-time table, the composite kernel the generated (without hipRTC: the interpreted) one
    assert step == ({'table': 0, 'generated': step['generated'], 'interpreted': 1 - step['generated']} if kind == 'composite'
                    else {'table': 1, 'generated': 0, 'interpreted': 0}), step


# ------------------------------------------------------------------------------------------------ 4. independent route
def test_factor_vjp_of_the_score_reproduces_the_kernel_entries():
    """Lbar = 2 tril(W L) through g3_potrf_vjp and g3_gram_vjp: 5 1/3 N^3 flops of generic reverse mode against the dedicated
    path; the location entry does not pass through the factor"""
    import g3py_amd as g3
    gp, nat, o, X, y, _ = _process_case(g3, 'se_bias')
    p = _params(gp, **nat)
    want = np.asarray(gp.dloo(p), dtype=np.float64)
    got = np.asarray(gp.factor_vjp(p, dr.lbar(o, X, y)), dtype=np.float64)
    at = np.cumsum([0] + [v.size for v in gp.model.vars])
    for i, v in enumerate(gp.model.vars):
        g, w = got[at[i]:at[i + 1]], want[at[i]:at[i + 1]]
        print('factor_vjp route %s: %s against dloo %s' % (v.name, g, w))
        if 'Bias' in v.name:
            assert np.all(g == 0.0) and np.all(w != 0.0)
        else:
            np.testing.assert_allclose(g, w, rtol=1e-8, atol=0)


# ------------------------------------------------------------------------------------------------ 5. chains
def _chain(gp, rng, rows=5):
    out = []
    for _ in range(rows):
        out.append(gp.active.dict_to_array(_params(gp, SE_var=rng.uniform(0.8, 1.8), SE_rate=RATE * rng.uniform(0.8, 1.25, 2),
                                                   Noise_var=rng.uniform(0.05, 0.2))))
    return np.stack(out)


def _row_reference(gp, row, X, y, fp32=False):
    """(reference of the row in gp.dloo's order and space as one vector, fp32 gap or None)"""
    v = {k: np.exp(val) for k, val in gp.active.array_to_dict(row).items()}
    nat = dict(SE_var=float(v['GP_SE_var_log_']), SE_rate=v['GP_SE_rate_log_'], Noise_var=float(v['GP_Noise_var_log_']))
    o = orc.GP(('SE', nat['SE_var'], nat['SE_rate'], None), nat['Noise_var'])
    gap, r = dr.fp32_gap(o, X, y) if fp32 else (None, dr.reference(o, X, y))
    parts = dict(SE_var=_leaf(r, 0, 'var'), SE_rate=_leaf(r, 0, 'rate', 2), Noise_var=_leaf(r, 1, 'var'))
    return np.concatenate([g for _, g in _blocks(gp, nat, parts)]), gap


@pytest.mark.parametrize('N', [97, 200, 300])
def test_chain_fp64(N):
    import g3py_amd as g3
    X, y = _reference(N)[:2]
    gp, _ = _se_gp(g3, X, y)
    chain = _chain(gp, np.random.default_rng(N))
    got = gp.dloo_chain(chain)
    assert got.shape == (5, gp.active.ndim) and got.dtype == np.float64
    single = np.stack([gp.dloo(gp.active.array_to_dict(r)) for r in chain])
    ref = np.stack([_row_reference(gp, r, X, y)[0] for r in chain])
    two = gp.dloo_chain(chain, batch=2)
    print('dloo_chain N=%d: max rel |chain - single| %.2e, row-norm |chain - closed form| %.2e, max rel |batch=2 - default| %.2e' % (
        N, np.abs(got / single - 1).max(), max(_rel(g, r) for g, r in zip(got, ref)), np.abs(two / got - 1).max()))
    np.testing.assert_allclose(got, single, rtol=1e-10, atol=0)
    for g, r in zip(got, ref):
        assert _rel(g, r) <= 1e-8
    # blocks of 2 + 2 + 1: a member's block mates are not its business
    np.testing.assert_allclose(two, got, rtol=1e-12, atol=0)


def test_chain_longer_than_one_launch_group():
    """N = 1100: a member's M is 1152^2 doubles, 25 of them fill the 256 MB of workspace one launch group may take; a block
    of 26 rows runs as groups of 25 + 1 and equals two blocks of 13, each a group of its own"""
    import g3py_amd as g3
    N = 1100
    X, y = _reference(N)[:2]
    gp, _ = _se_gp(g3, X, y)
    chain = np.tile(_chain(gp, np.random.default_rng(N), rows=2), (13, 1)) + 0.01 * np.arange(26)[:, None]
    got = gp.dloo_chain(chain)
    halves = gp.dloo_chain(chain, batch=13)
    print('dloo_chain N=%d, 26 rows: max rel |one block - two blocks| %.2e' % (N, np.abs(got / halves - 1).max()))
    assert got.shape == (26, gp.active.ndim) and np.all(np.isfinite(got)) and np.all(got != 0.0)
    np.testing.assert_allclose(got, halves, rtol=1e-12, atol=0)
    np.testing.assert_allclose(got[25], gp.dloo(gp.active.array_to_dict(chain[25])), rtol=1e-10, atol=0)


def test_chain_fp32():
    import g3py_amd as g3
    N = 200
    X, y = problem(N, dtype=np.float32)
    gp, _ = _se_gp(g3, X, y, dtype=np.float32)
    chain = _chain(gp, np.random.default_rng(N + 1))
    got = gp.dloo_chain(chain)
    assert got.dtype == np.float32 and got.shape == (5, gp.active.ndim)
    for i, row in enumerate(chain):
        ref, gap = _row_reference(gp, row, X, y, fp32=True)
        err = _rel(got[i], ref)
        print('dloo_chain fp32 N=%d row %d: rel error against the float64 closed form %.3e, float32 closed form %.3e (bound 10 x)' % (
            N, i, err, gap))
        assert err <= 10 * gap


def test_chain_member_whose_first_factorisation_fails():
    """the member of test_gpu_loo.test_chain_member_whose_first_factorisation_fails: it goes through the jitter schedule on its
    own and is differentiated at the factor that was kept, like its single dloo; the others do not notice"""
    import g3py_amd as g3
    N = 100
    rng = np.random.default_rng(N)
    X = np.repeat(rng.uniform(0, 6, (N // 2, 1)), 2, axis=0)
    y = np.sin(X[:, 0]) + 0.5 + 0.05 * rng.standard_normal(N)
    gp = g3.GaussianProcess(space=X[:2], location=g3.Zero(), kernel=g3.SE(X))
    gp.observed(X, y)
    rows = [gp.active.dict_to_array(_params(gp, SE_var=sv, SE_rate=[1.0], Noise_var=nv))
            for sv, nv in ((1.0, 0.1), (1.3, 0.2), (1e6, 1e-12), (0.8, 0.05), (1.1, 0.15))]
    chain = np.stack(rows)
    one = np.asarray(gp.dloo(gp.active.array_to_dict(chain[2])), dtype=np.float64)
    assert gp._cache['stats']['tries'] >= 1 and not gp._cache['stats']['fallback']
    got = gp.dloo_chain(chain)
    clean = gp.dloo_chain(np.delete(chain, 2, axis=0))
    np.testing.assert_allclose(np.delete(got, 2, axis=0), clean, rtol=1e-12, atol=0)
    bound = 1e-10
    print('dloo_chain jittered member: chain %s single %s rel diff %.2e (bound %.1e)' % (got[2], one, np.abs(got[2] / one - 1).max(), bound))
    assert np.all(np.isfinite(got[2])) and np.any(got[2] != 0.0)
    np.testing.assert_allclose(got[2], one, rtol=bound, atol=0)


def test_chain_sentinel_rows():
    """a row loo_chain sends to -1e30 gets zeros; its neighbours are untouched"""
    import g3py_amd as g3
    X, y = _reference(97)[:2]
    gp = g3.GaussianProcess(space=X[:2], location=g3.Bias(), kernel=g3.SE(X))
    gp.observed(X, y)
    rows = []
    for bias in (0.1, np.inf, -0.2):
        rows.append(gp.active.dict_to_array(_params(gp, SE_var=1.3, SE_rate=RATE, Noise_var=0.1, Bias_Bias=bias)))
    chain = np.stack(rows)
    got = gp.dloo_chain(chain)
    assert gp.loo_chain(chain)[1] == np.float32(-1e30)
    assert np.all(got[1] == 0.0) and np.all(gp.dloo(gp.active.array_to_dict(chain[1])) == 0.0)
    for i in (0, 2):
        np.testing.assert_allclose(got[i], gp.dloo(gp.active.array_to_dict(chain[i])), rtol=1e-10, atol=0)
        assert np.all(got[i] != 0.0)


# ------------------------------------------------------------------------------------------------ 6. call order
def test_dloo_after_logp_builds_and_factors_nothing():
    """logp(p) then dloo(p): the Gram launch counter and the factorisation's profiling tag stay where logp put them; dloo adds
    its K^-1 sweep (`trsm`), one launch of the kernel-parameter sums (counted by grad_path_stats; that pass carries the
    `gram` tag, as in dlogp) and nothing on a second call.  loo's bits do not depend on a dloo before it."""
    import g3py_amd as g3
    X, y = _reference(385)[:2]
    dev = g3.Device(0)
    try:
        gp, p = _se_gp(g3, X, y, device=dev)
        q = _params(gp, SE_var=1.0, SE_rate=RATE, Noise_var=0.2)
        alone = gp.loo(q, var=True)                       # loo on its own, on parameters nothing else has seen
        dev.prof_enable(True)
        dev.prof_reset()
        gp.logp(p)
        grams, grads, prof = dev.gram_path_stats(), dev.grad_path_stats(), dev.prof_collect()
        assert prof['gram']['count'] >= 1 and prof['potrf']['count'] >= 1
        g = gp.dloo(p)
        grams2, grads2, prof2 = dev.gram_path_stats(), dev.grad_path_stats(), dev.prof_collect()
        assert grams2 == grams and prof2['potrf']['count'] == prof['potrf']['count']
        assert sum(grads2.values()) == sum(grads.values()) + 1
        assert prof2['gram']['count'] == prof['gram']['count'] + 1 and prof2['trsm']['count'] == prof['trsm']['count'] + 1
        assert gp._cache.get('loo') is None
        assert np.array_equal(gp.dloo(p), g)              # kept with the factor: no device work at all
        prof3 = dev.prof_collect()
        assert all(prof3[k]['count'] == prof2[k]['count'] for k in prof2)
        assert _rel(g, np.concatenate([b for _, b in _blocks(gp, dict(SE_var=1.3, SE_rate=RATE, Noise_var=0.1), dict(
            zip(('SE_var', 'SE_rate', 'Noise_var'), np.split(_reference(385)[2], [1, 3]))))])) <= 1e-8
        # dloo(q) first, a dlogp in between (they share Y, Kinv and alpha), then loo(q): the bits loo returns alone
        gq = gp.dloo(q)
        gl = gp.dlogp(q)
        after = gp.loo(q, var=True)
        assert after.logpredictive == alone.logpredictive
        assert np.array_equal(after.mean, alone.mean) and np.array_equal(after.variance, alone.variance)
        assert np.array_equal(gp.dloo(q), gq) and np.all(np.isfinite(gl))
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ 7. memory contract
def _hostile_run(dv, X, y, N, dt, hostile=True):
    """g3_gp_factor, then g3_gp_dloo on its buffers.  hostile: every operand inside NaN / canary guards with slack in its
    leading dimension; L, invd, a and X must come back byte for byte and nothing outside the documented outputs may be
    written.  Returns dict(slots, alpha, kdiag, u, Kinv (lower triangle))."""
    from g3py_amd import _lib
    from g3py_amd.device import compile_spec
    d, Np = X.shape[1], _lib.roundup(N)
    prog = compile_spec(('sum', SE_SPEC, ('NOISE', 0.1)), d)
    gmap = dv.grad_layout(prog)
    sl = hm.slack(dt) if hostile else 0
    fill = (lambda b: b) if hostile else (lambda b: 0)
    Xd, Xo = hm.embed(dv, X.astype(dt), N, d + sl, dt, fill(NAN_BYTE))
    dl, _ = hm.embed(dv, y.astype(dt), 1, N + sl, dt, fill(NAN_BYTE))
    K, Ko = hm.embed(dv, (Np + 128, Np), Np + 128, Np + sl, dt, fill(CANARY_BYTE))
    W, Wo = hm.embed(dv, (Np, 128), Np, 128, dt, fill(CANARY_BYTE))
    a, ao = hm.embed(dv, (1, Np), 1, Np + sl, dt, fill(CANARY_BYTE))
    st = dv.gp_factor(prog, Xd, N, d, dl, K, W, a)
    assert st['info'] == 0 and st['tries'] == 0
    dv.sync()
    for o in (Ko, Wo, ao):                 # from here on the factor's outputs are inputs: what they hold now must stay
        o.image = o.download_all()
    Y, Yo = hm.embed(dv, (Np, Np), Np, Np + sl, dt, fill(CANARY_BYTE))
    Ki, Kio = hm.embed(dv, (Np, Np), Np, Np + sl, dt, fill(CANARY_BYTE))
    vecs = [hm.embed(dv, (1, Np), 1, Np + sl, dt, fill(CANARY_BYTE)) for _ in range(3)]
    slots = dv.gp_dloo(prog, gmap, Xd, N, d, K, W, a, Y, Ki, *[v for v, _ in vecs])
    dv.sync()
    if hostile:
        for o, what in ((Xo, 'X'), (Ko, 'L'), (Wo, 'invd'), (ao, 'a')):
            hm.check_untouched(dv, o, what=what)
        hm.check_untouched(dv, Yo, np.ones((Np, Np), bool), what='Y')
    # (Kinv is a roundup(N)-square output as in g3_gp_dlogp: the sweep may write zeros above the diagonal of its diagonal
    #  tiles; only the lower triangle is defined, and compared)
    whole = hm.check_untouched(dv, Kio, np.ones((Np, Np), bool), what='Kinv') if hostile else None
    out = dict(slots=slots, Kinv=np.where(hm.tril_mask(Np), Kio.block(whole), 0).astype(dt))
    for name, (_, o) in zip(('alpha', 'kdiag', 'u'), vecs):
        whole = hm.check_untouched(dv, o, np.ones((1, Np), bool), what=name) if hostile else None
        out[name] = o.block(whole)
    return out


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_memory_contract_and_reproducibility(dtype):
    import g3py_amd as g3
    N = 200
    X, y = problem(N, dtype=np.float32)          # float32-representable in both dtypes
    X, y = X.astype(np.float64), y.astype(np.float64)
    fresh = g3.Device(0)
    try:
        first = _hostile_run(fresh, X, y, N, dtype)
        second = _hostile_run(fresh, X, y, N, dtype)
    finally:
        fresh.close()
    dirty = hm.dirty_device()
    try:
        used = _hostile_run(dirty, X, y, N, dtype)
    finally:
        dirty.close()
    plain = _hostile_run(g3.Device.default(), X, y, N, dtype, hostile=False)
    for k in ('slots', 'alpha', 'kdiag', 'u', 'Kinv'):
        hm.same_bits(first[k], second[k], what='%s: fresh context, second call' % k)
        hm.same_bits(first[k], used[k], what='%s: used context' % k)
        hm.same_bits(first[k], plain[k], what='%s: plain buffers on the default context' % k)
    for k in ('alpha', 'kdiag', 'u'):
        assert np.all(first[k][0, N:] == 0.0), k
    gap, ref = dr.fp32_gap(orc.GP(SE_SPEC, 0.1), X, y)
    assert _rel(first['slots'], dr.natural_vector(ref)) <= (1e-8 if dtype == np.float64 else 10 * gap)


# ------------------------------------------------------------------------------------------------ 8. argument checks
def test_argument_checks():
    """sizes and pointers are refused with the number of the argument, as g3_gp_dlogp / g3_gp_dlogp_batched_fields do"""
    import g3py_amd as g3
    from g3py_amd.device import compile_spec
    dev = g3.Device.default()
    lib, ctx = dev.lib, dev.ctx
    buf = dev.alloc(384, 128, np.float64)
    p = buf.ptr
    prog = compile_spec(('sum', SE_SPEC, ('NOISE', 0.1)), 2)
    gmap = dev.grad_layout(prog)
    out = (C.c_double * 8)()
    pr, gm = C.byref(prog), C.byref(gmap)

    def one(**kw):
        a = dict(prog=pr, map=gm, X=p, N=100, ldx=2, d=2, L=p, ldl=128, invd=p, a=p, dt=0, Y=p, ldy=128, Kinv=p, ldc=128, alpha=p,
                 kdiag=p, u=p, out=out)
        a.update(kw)
        return lib.g3_gp_dloo(ctx, *a.values())
    assert one(prog=None) == -2 and one(map=None) == -3 and one(X=None) == -4 and one(N=0) == -5
    assert one(ldx=1) == -6 and one(d=0) == -7 and one(L=None) == -8
    assert one(N=129, ldy=256, ldc=256) == -9                   # ldl below roundup(N, 128)
    assert one(invd=None) == -10 and one(a=None) == -11 and one(dt=7) == -12 and one(Y=None) == -13 and one(ldy=127) == -14
    assert one(Kinv=None) == -15 and one(ldc=127) == -16 and one(alpha=None) == -17 and one(kdiag=None) == -18
    assert one(u=None) == -19 and one(out=None) == -20
    bad = dev.grad_layout(prog)
    bad.var[0] = bad.nslots
    assert one(map=C.byref(bad)) == -3

    fields = np.array([[1.3]])
    offs = np.array([type(prog).leaf.offset + type(prog.leaf[0]).var.offset], dtype=np.int32)

    def many(**kw):
        a = dict(tmpl=pr, batch=1, fields=fields.ctypes.data, offsets=offs.ctypes.data, nfield=1, map=gm, X=p, N=100, ldx=2, d=2, L=p,
                 ldl=128, kstride=256 * 128, invd=p, a=p, dt=0, Y=p, Kinv=p, alpha=p, kdiag=p, u=p, out=out)
        a.update(kw)
        return lib.g3_gp_dloo_batched_fields(ctx, *a.values())
    assert many(tmpl=None) == -2 and many(batch=0) == -3 and many(batch=4097) == -3 and many(fields=None) == -4
    assert many(nfield=-1) == -6 and many(map=None) == -7 and many(X=None) == -8 and many(N=0) == -9 and many(ldx=1) == -10
    assert many(d=0) == -11 and many(L=None) == -12 and many(ldl=127) == -13
    assert many(kstride=127 * 128) == -14                       # members would overlap
    assert many(invd=None) == -15 and many(a=None) == -16 and many(dt=7) == -17 and many(Y=None) == -18 and many(Kinv=None) == -19
    assert many(alpha=None) == -20 and many(kdiag=None) == -21 and many(u=None) == -22 and many(out=None) == -23
