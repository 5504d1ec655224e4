"""GPU tests of the chain prediction: predict_chain / average (GaussianProcess) and the C entry points
g3_gp_cross_batched(_fields) -- rectangular batched Gram + the block forward solve of g3_crossb.hip.
Tolerances are the project's stated ones: fp64 mean / variance 1e-8 * scale against the single
prediction of the same row with scale = max(1, max |mean|), fp32 a plain 1e-4."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KW = dict(var=True, median=True, quantiles=True)


def _params(gp, **nat):
    p = gp.params_test
    by = {v.name: v for v in gp.model.vars}
    for k, val in nat.items():
        v = by[gp.name + '_' + k]
        p[v.key] = (np.log(val) if v.positive else np.asarray(val, dtype=float)) * np.ones(v.shape)
    return p


def _single(gp, chain, **kw):
    """the loop the batched path replaces: one predict per row"""
    rows = [gp.predict(gp.active.array_to_dict(r), **kw) for r in chain]
    return {k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0]}


def _check_rows(got, want, f32=False, what=''):
    assert set(got) == set(want), (set(got), set(want))
    scale = max(1.0, np.nanmax(np.abs(want['mean'][np.isfinite(want['mean'])]), initial=1.0)) if 'mean' in want else 1.0
    tol = 1e-4 if f32 else 1e-8 * scale
    worst = {}
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (k, got[k].shape, want[k].shape)
        with np.errstate(invalid='ignore'):
            worst[k] = float(np.nanmax(np.abs(got[k].astype(np.float64) - want[k].astype(np.float64)), initial=0.0))
    print('predict_chain %s: max |batched - single| per key %s (bound %.1e)' % (what, worst, tol))
    for k in want:
        np.testing.assert_allclose(got[k], want[k], rtol=0, atol=tol, equal_nan=True, err_msg='%s %s' % (what, k))


def _se_problem(N, d, dtype, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, N ** (1 / d), (N, d))
    y = np.sin(X.sum(1) / 2) + 0.1 * rng.standard_normal(N)
    S = rng.uniform(0, N ** (1 / d), (300, d))
    return rng, X.astype(dtype), y.astype(dtype), S.astype(dtype)


# N <= 256: the one-workgroup chain kernel; 300 ... 1024: the cooperative kernel and the lock-step sweep; 1500: members
# beyond the one-launch solve (the single-member cross path per member)
CASES = ([(N, 'small') for N in (64, 100, 128, 200, 256)] +
         [(N, m) for N in (300, 512, 700, 1024) for m in ('coop', 'sweep')] + [(1500, 'sweep')])


@pytest.mark.parametrize('N,mode', CASES)
def test_every_row_equals_the_single_prediction(monkeypatch, N, mode):
    """rows of predict_chain == predict of that row, N x M x noise of the issue, both chain kernels, several batch blocks"""
    import g3py_amd as g3
    monkeypatch.setenv('G3_COOP_MIN_BATCH', '2')
    monkeypatch.setenv('G3_COOP_MAX_N', '0' if mode == 'sweep' else '1024')
    dev = g3.Device(0)                             # the knobs are read when a context is created
    try:
        rng, X, y, S = _se_problem(N, 3, np.float64, N)
        gp = g3.GaussianProcess(space=S, location=g3.Bias(), kernel=g3.SE(X), device=dev)
        gp.observed(X, y)
        a0 = gp.active.dict_to_array(_params(gp, SE_var=1.2, SE_rate=[0.8, 1.0, 1.3], Noise_var=0.1, Bias_Bias=0.1))
        chain = a0 + 0.15 * rng.standard_normal((5, len(a0)))
        chain[0] = a0
        for M in (1, 100, 128, 300):
            for noise in (False, True):
                want = _single(gp, chain, space=S[:M], noise=noise, **KW)
                got = gp.predict_chain(chain, space=S[:M], noise=noise, batch=2, **KW)      # blocks of 2 + 2 + 1 members
                _check_rows(got, want, what='N=%d %s M=%d noise=%d' % (N, mode, M, noise))
        one = gp.predict_chain(chain, space=S[:100], noise=True, **KW)                       # one block, default batch
        _check_rows(one, _single(gp, chain, space=S[:100], noise=True, **KW), what='N=%d one block' % N)
    finally:
        dev.close()


@pytest.mark.parametrize('N', [128, 256, 640])
def test_fp32_rows(N):
    import g3py_amd as g3
    rng, X, y, S = _se_problem(N, 3, np.float32, N + 1)
    gp = g3.GaussianProcess(space=S[:100], location=g3.Bias(), kernel=g3.SE(X), dtype=np.float32)
    gp.observed(X, y)
    a0 = gp.active.dict_to_array(_params(gp, SE_var=1.2, SE_rate=[0.8, 1.0, 1.3], Noise_var=0.1, Bias_Bias=0.1))
    chain = a0 + 0.15 * rng.standard_normal((6, len(a0)))
    for noise in (False, True):
        got = gp.predict_chain(chain, noise=noise, batch=4, **KW)
        assert got['mean'].dtype == np.float32
        _check_rows(got, _single(gp, chain, noise=noise, **KW), f32=True, what='fp32 N=%d noise=%d' % (N, noise))


def test_row0_reproduces_the_oracle_fixture(golden_dir):
    import g3py_amd as g3
    g = np.load(os.path.join(golden_dir, 'oracle_process.npz'))
    X, Xs, y = g['X'], g['Xs'], g['gp_se_bias_y']
    gp = g3.GaussianProcess(space=Xs, location=g3.Bias(), kernel=g3.SE(X))
    gp.observed(X, y)
    a0 = gp.active.dict_to_array(_params(gp, SE_var=1.1, SE_rate=[0.9, 1.2], Noise_var=0.1, Bias_Bias=0.3))
    rng = np.random.default_rng(5)
    chain = a0 + 0.2 * rng.standard_normal((9, len(a0)))
    chain[0] = a0
    scale = max(1.0, np.abs(g['gp_se_bias_mean_n0']).max())
    p0 = gp.predict_chain(chain, var=True, noise=False, batch=4)
    p1 = gp.predict_chain(chain, var=True, noise=True, batch=4)
    print('oracle pin: mean %.2e var_n0 %.2e var_n1 %.2e' % (np.abs(p0['mean'][0] - g['gp_se_bias_mean_n0']).max(),
                                                             np.abs(p0['variance'][0] - g['gp_se_bias_var_n0']).max(),
                                                             np.abs(p1['variance'][0] - g['gp_se_bias_var_n1']).max()))
    np.testing.assert_allclose(p0['mean'][0], g['gp_se_bias_mean_n0'], rtol=0, atol=1e-8 * scale)
    np.testing.assert_allclose(p0['variance'][0], g['gp_se_bias_var_n0'], rtol=0, atol=1e-8 * scale)
    np.testing.assert_allclose(p1['variance'][0], g['gp_se_bias_var_n1'], rtol=0, atol=1e-8 * scale)


KERNELS = {
    'composite_se_cos_plus_lin': lambda g3, X: g3.SE(X) * g3.COS(X) + g3.LIN(X),
    'periodic_mat52_plus_cos': lambda g3, X: g3.MAT52(X) + g3.COS(X),
    'nn': lambda g3, X: g3.NN(X),
    'pol3_times_ou': lambda g3, X: g3.POL(X, 3) * g3.OU(X),
    'wn_cross_counts': lambda g3, X: g3.SE(X) + g3.WN(X),
}


@pytest.mark.parametrize('jit', [1, 0])
@pytest.mark.parametrize('name', sorted(KERNELS))
@pytest.mark.parametrize('N', [150, 400])
def test_kernel_zoo_generated_and_interpreted(monkeypatch, name, N, jit):
    """composite, periodic and dot-product expressions through the rectangular batched Gram: the kernel generated for the
    expression (G3_GRAM_JIT=1) and the interpreter (G3_GRAM_JIT=0); the single predictions they are compared with take
    the library's own choice for one member (compile-time table, generated or interpreted)"""
    import g3py_amd as g3
    monkeypatch.setenv('G3_GRAM_JIT', str(jit))
    dev = g3.Device(0)
    try:
        rng = np.random.default_rng(N + jit)
        X = 1.5 * rng.standard_normal((N, 2))
        X[3] = X[2]
        y = 0.4 * X[:, 0] + np.sin(X.sum(1)) + 0.3 * rng.standard_normal(N)
        S = np.concatenate([1.5 * rng.standard_normal((60, 2)), X[:10]])       # some query points ARE inputs (WN counts them)
        gp = g3.GaussianProcess(space=S, location=g3.Bias(), kernel=KERNELS[name](g3, X), device=dev)
        gp.observed(X, y)
        a0 = gp.active.dict_to_array(gp.params_default)
        chain = a0 + 0.1 * rng.standard_normal((6, len(a0)))     # two blocks of three members
        before = dev.gram_path_stats()
        got = gp.predict_chain(chain, batch=3, noise=True, **KW)
        after = dev.gram_path_stats()
        assert after['table'] == before['table']               # the chain's launches carry the batch: never the table
        if jit:
            assert after['generated'] > before['generated'] and after['interpreted'] == before['interpreted'], (before, after)
        else:
            assert after['interpreted'] > before['interpreted'] and after['generated'] == before['generated'], (before, after)
        want = _single(gp, chain, noise=True, **KW)
        assert np.all(np.isfinite(want['mean'])) and np.all(np.isfinite(want['variance']))
        _check_rows(got, want, what='%s N=%d jit=%d' % (name, N, jit))
    finally:
        dev.close()


@pytest.mark.parametrize('N', [80, 400])
def test_edge_members_in_one_batch(N):
    """a member that needs the jitter schedule (duplicated inputs, no noise) and members whose delta is not finite
    (an infinite mean) beside ordinary ones: each equals its single prediction"""
    import g3py_amd as g3
    rng = np.random.default_rng(N)
    X = np.repeat(rng.uniform(0, 6, (N // 2, 1)), 2, axis=0)          # every input twice: singular without noise
    y = np.sin(X[:, 0]) + 0.5
    S = np.linspace(-1, 7, 50)[:, None]
    gp = g3.GaussianProcess(space=S, location=g3.Bias(), kernel=g3.SE(X))
    gp.observed(X, y)
    rows = []
    for noise, bias in [(0.1, 0.2), (0.0, 0.2), (0.2, np.inf), (0.05, -0.3), (0.1, np.nan)]:
        p = _params(gp, SE_var=1.0, SE_rate=[1.0], Noise_var=max(noise, 1e-300), Bias_Bias=0.0)
        if noise == 0.0:
            p['GP_Noise_var_log_'] = np.asarray(-800.0)                # exp underflows: no noise, the first factorisation fails
        p['GP_Bias_Bias'] = np.asarray(bias)
        rows.append(gp.active.dict_to_array(p))
    chain = np.stack(rows)
    want = _single(gp, chain, **KW)
    assert np.all(np.isinf(want['mean'][2])) and np.all(np.isnan(want['mean'][4])) and np.all(np.isfinite(want['mean'][[0, 1, 3]]))
    # the jittered member: its single evaluation retried
    gp.predict(gp.active.array_to_dict(chain[1]))
    assert gp._cache['stats']['tries'] >= 1
    for batch in (None, 2):
        got = gp.predict_chain(chain, batch=batch, **KW)
        # member 1 sits on a jittered factor (kappa ~ 1e6 / jitter): compared at the same absolute bound as the others
        _check_rows(got, want, what='edge members N=%d batch=%s' % (N, batch))
    # observations that are not finite: tt_to_num(mapping.inv(y)) feeds the posterior (elliptical.py:63)
    y2 = y.copy()
    y2[3], y2[5] = np.nan, np.inf
    got = gp.predict_chain(chain[[0, 3]], outputs=y2, **KW)
    _check_rows(got, _single(gp, chain[[0, 3]], outputs=y2, **KW), what='non-finite y N=%d' % N)


def _abi_setup(N, M, B, dtype=np.float64, kernel=None):
    import g3py_amd as g3
    from g3py_amd import _lib
    from g3py_amd.device import compile_spec, compile_spec_rows
    rng = np.random.default_rng(N + M)
    d = 2
    X = rng.uniform(0, 5, (N, d))
    y = np.sin(X.sum(1))
    S = rng.uniform(0, 5, (M, d))
    gp = g3.GaussianProcess(space=S, location=g3.Zero(), kernel=kernel(g3, X) if kernel else g3.SE(X) * g3.COS(X) + 0.5 * g3.RQ(X),
                            dtype=dtype)
    gp.observed(X, y)
    a0 = gp.active.dict_to_array(gp.params_default)
    chain = a0 + 0.2 * rng.standard_normal((B, len(a0)))
    values_b, _ = gp._values_rows(chain)
    v0 = gp._values_row(values_b, 0)
    tmpl, offs, fields = compile_spec_rows(gp.f_kernel_noise.spec(values_b, d), gp.f_kernel_noise.spec(v0, d), d, B)
    ctm, coffs, cfields = compile_spec_rows(gp.f_kernel.spec(values_b, d), gp.f_kernel.spec(v0, d), d, B)
    cprogs = [compile_spec(gp.f_kernel.spec(gp._values_row(values_b, j), d), d) for j in range(B)]
    dev = gp.device
    Np, Mp = _lib.roundup(N), _lib.roundup(M, 128)
    kstride = (Np + _lib.G3_RHS_PAD) * Np
    buf = dict(K=dev.alloc(B * (Np + _lib.G3_RHS_PAD), Np, dtype), W=dev.alloc(B * Np, _lib.G3_PAD, dtype), a=dev.alloc(B, Np, dtype),
               Xd=dev.upload(X.astype(dtype)), Sd=dev.upload(S.astype(dtype)), dd=dev.upload(np.tile(y, (B, 1)).astype(dtype)))
    dev.gp_factor_batched_fields(tmpl, offs, fields, buf['Xd'], N, d, buf['dd'], buf['K'], kstride, buf['W'], buf['a'])
    return gp, dev, buf, dict(N=N, M=M, B=B, d=d, Np=Np, Mp=Mp, kstride=kstride), (ctm, coffs, cfields), cprogs


@pytest.mark.parametrize('N,dtype', [(96, np.float64), (700, np.float64), (1300, np.float64), (200, np.float32)])
def test_fields_form_equals_programs_form_and_is_repeatable(N, dtype):
    """g3_gp_cross_batched_fields == g3_gp_cross_batched on the expanded programs, bit for bit; two calls give the same
    bits; mu / ss / kdiag may each be left out without changing the others"""
    gp, dev, buf, s, (ctm, coffs, cfields), cprogs = _abi_setup(N, 70, 9, dtype)
    outs = []
    for call in ('progs', 'fields', 'fields'):
        mu, ss, kd = (dev.alloc(s['B'], s['Mp'], dtype, zero=True) for _ in range(3))
        if call == 'progs':
            dev.gp_cross_batched(cprogs, buf['Sd'], s['M'], buf['Xd'], s['N'], s['d'], buf['K'], s['kstride'], buf['W'], buf['a'], mu, ss, kd)
        else:
            dev.gp_cross_batched_fields(ctm, coffs, cfields, buf['Sd'], s['M'], buf['Xd'], s['N'], s['d'], buf['K'], s['kstride'],
                                        buf['W'], buf['a'], mu, ss, kd)
        outs.append([dev.download(o, s['B'], s['M']) for o in (mu, ss, kd)])
    for o in outs[1:]:
        for x, z in zip(outs[0], o):
            np.testing.assert_array_equal(x, z)
    assert np.all(np.isfinite(outs[0][0])) and np.all(outs[0][1] >= 0) and np.all(outs[0][2] > 0)
    for keep in range(3):
        o = [dev.alloc(s['B'], s['Mp'], dtype, zero=True) if i == keep else None for i in range(3)]
        dev.gp_cross_batched_fields(ctm, coffs, cfields, buf['Sd'], s['M'], buf['Xd'], s['N'], s['d'], buf['K'], s['kstride'],
                                    buf['W'], buf['a'], *o)
        np.testing.assert_array_equal(dev.download(o[keep], s['B'], s['M']), outs[0][keep])
    # the prior's call: no factor at all
    kd = dev.alloc(s['B'], s['Mp'], dtype, zero=True)
    dev.gp_cross_batched_fields(ctm, coffs, cfields, buf['Sd'], s['M'], buf['Sd'], s['M'], s['d'], None, 0, None, None, None, None, kd)
    np.testing.assert_array_equal(dev.download(kd, s['B'], s['M']), outs[0][2])


def test_bad_arguments_return_the_documented_codes():
    import ctypes as C
    import g3py_amd as g3
    from g3py_amd import _lib
    gp, dev, buf, s, (ctm, coffs, cfields), cprogs = _abi_setup(200, 40, 4)
    lib, ctx = dev.lib, dev.ctx
    arr = (_lib.KernelProg * s['B'])(*cprogs)
    mu, ss, kd = (dev.alloc(s['B'], s['Mp'], np.float64) for _ in range(3))
    good = dict(progs=arr, batch=s['B'], Xs=buf['Sd'].ptr, M=s['M'], ldxs=s['d'], X=buf['Xd'].ptr, N=s['N'], ldx=s['d'], d=s['d'],
                L=buf['K'].ptr, ldl=s['Np'], kstride=s['kstride'], invd=buf['W'].ptr, a=buf['a'].ptr, dt=0, mu=mu.ptr, ss=ss.ptr,
                kdiag=kd.ptr)
    order = list(good)

    def call(**over):
        v = dict(good, **over)
        return lib.g3_gp_cross_batched(ctx, *[v[k] for k in order])
    assert call() == 0
    other = (_lib.KernelProg * s['B'])(*cprogs)
    other[2].leaf[0].kind = _lib.KINDS['OU']                 # another structure
    for over, code in [(dict(progs=None), -2), (dict(progs=other), -2), (dict(batch=0), -3), (dict(batch=_lib.G3_MAX_BATCH + 1), -3),
                       (dict(Xs=None), -4), (dict(M=0), -5), (dict(ldxs=1), -6), (dict(X=None), -7), (dict(N=0), -8),
                       (dict(ldx=1), -9), (dict(d=0), -10), (dict(d=_lib.G3_MAXCOLS + 1), -10), (dict(L=None), -11),
                       (dict(ldl=s['Np'] - 2), -12), (dict(ldl=s['Np'] + 1), -12), (dict(kstride=s['Np'] * s['Np'] - 2), -13),
                       (dict(invd=None), -14), (dict(a=None), -15), (dict(dt=7), -16)]:
        assert call(**over) == code, (over, call(**over), code)
    assert call(a=None, mu=None) == 0                        # a is only needed for mu
    assert call(L=None, invd=None, a=None, mu=None, ss=None) == 0
    assert lib.g3_gp_cross_batched(None, *[good[k] for k in order]) == -1
    # the template form: its own first six arguments, then the same list three places further
    f = np.ascontiguousarray(cfields)
    o = np.ascontiguousarray(coffs, dtype=np.int32)
    tail = [good[k] for k in order[2:]]

    def callf(tm=C.byref(ctm), batch=s['B'], fields=f.ctypes.data, offs=o.ctypes.data, nf=len(o), tail=tail):
        return lib.g3_gp_cross_batched_fields(ctx, tm, batch, fields, offs, nf, *tail)
    assert callf() == 0
    assert callf(tm=None) == -2 and callf(batch=0) == -3 and callf(fields=None) == -4 and callf(nf=10 ** 6) == -6
    for bad in (4, 0, _lib.KernelProg.leaf.offset + 8, 10 ** 6):          # not 8-aligned / nleaf / a leaf's dims / outside
        o2 = o.copy()
        o2[0] = bad
        assert callf(offs=o2.ctypes.data) == -5
    for key, code in [('Xs', -7), ('M', -8), ('X', -10), ('N', -11), ('L', -14), ('invd', -17), ('a', -18)]:
        v = dict(good, **{key: None if key not in ('M', 'N') else 0})
        assert callf(tail=[v[k] for k in order[2:]]) == code, key
    # the exponent of a POL leaf is structure: its offset is refused, as in g3_gp_factor_batched_fields
    gp2, dev2, buf2, s2, (ctm2, coffs2, cfields2), _ = _abi_setup(150, 30, 3, kernel=lambda g3, X: g3.POL(X, 3) + g3.SE(X))
    leaf0 = _lib.KernelProg.leaf.offset
    pol = [i for i in range(ctm2.nleaf) if ctm2.leaf[i].kind == _lib.KINDS['DOT']][0]
    o3 = np.ascontiguousarray(coffs2, dtype=np.int32).copy()
    o3[0] = leaf0 + pol * C.sizeof(_lib.Leaf) + _lib.Leaf.freq.offset
    kd2 = dev2.alloc(s2['B'], s2['Mp'], np.float64)
    with pytest.raises(g3.G3Error, match='status -5'):
        dev2.gp_cross_batched_fields(ctm2, o3, cfields2, buf2['Sd'], s2['M'], buf2['Xd'], s2['N'], s2['d'], buf2['K'], s2['kstride'],
                                     buf2['W'], buf2['a'], None, None, kd2)


@pytest.mark.parametrize('N', [128, 600])
def test_repeatable_and_no_interference_with_the_other_chain_calls(N):
    """two predict_chain calls give the same bits; logp_chain and dlogp_chain interleaved with predict_chain on one
    process object (one shared workspace that only grows) return what they return alone"""
    import g3py_amd as g3
    rng, X, y, S = _se_problem(N, 3, np.float64, N + 7)

    def make():
        gp = g3.GaussianProcess(space=S[:90], location=g3.Bias(), kernel=g3.SE(X))
        gp.observed(X, y)
        return gp
    gp = make()
    a0 = gp.active.dict_to_array(_params(gp, SE_var=1.2, SE_rate=[0.8, 1.0, 1.3], Noise_var=0.1, Bias_Bias=0.1))
    chain = a0 + 0.15 * rng.standard_normal((12, len(a0)))
    lp_alone, dl_alone = make().logp_chain(chain), make().dlogp_chain(chain)
    pc_alone = make().predict_chain(chain, **KW)
    p1 = gp.predict_chain(chain[:5], **KW)                     # a small workspace first: it has to grow below
    lp = gp.logp_chain(chain)
    p2 = gp.predict_chain(chain, **KW)
    dl = gp.dlogp_chain(chain)
    p3 = gp.predict_chain(chain, **KW)
    lp2 = gp.logp_chain(chain)
    np.testing.assert_array_equal(lp, lp_alone)
    np.testing.assert_array_equal(lp2, lp_alone)
    np.testing.assert_array_equal(dl, dl_alone)
    for k in pc_alone:
        np.testing.assert_array_equal(p2[k], pc_alone[k])
        np.testing.assert_array_equal(p3[k], pc_alone[k])
        np.testing.assert_array_equal(p1[k], pc_alone[k][:5])
    assert gp._chain_ws['cap'] >= 12 and gp._chain_ws['grad'] and gp._chain_ws['pred'] >= 128
    # the single-row cache of the process is untouched by the chain calls
    one = gp.predict(gp.active.array_to_dict(chain[3]), **KW)
    _check_rows({k: v[3:4] for k, v in p3.items()}, {k: np.asarray(v)[None] for k, v in one.items()}, what='after chains')


def test_prior_chain_and_unobserved_process():
    import g3py_amd as g3
    rng, X, y, S = _se_problem(120, 3, np.float64, 3)
    gp = g3.GaussianProcess(space=S[:77], location=g3.Bias(), kernel=g3.SE(X) + g3.LIN(X))
    a0 = gp.active.dict_to_array(gp.params_default)
    chain = a0 + 0.2 * rng.standard_normal((6, len(a0)))
    for noise in (False, True):                                   # nothing observed: the prior
        _check_rows(gp.predict_chain(chain, noise=noise, batch=4, **KW), _single(gp, chain, noise=noise, **KW), what='unobserved')
    assert getattr(gp, '_chain_ws', None) is None                 # no factor workspace was made for it
    gp.observed(X, y)
    for noise in (False, True):
        _check_rows(gp.predict_chain(chain, prior=True, noise=noise, **KW), _single(gp, chain, prior=True, noise=noise, **KW),
                    what='prior=True')


def test_average_equals_the_mean_of_single_predictions():
    import g3py_amd as g3
    rng, X, y, S = _se_problem(180, 3, np.float64, 11)
    gp = g3.GaussianProcess(space=S[:64], location=g3.Bias(), kernel=g3.SE(X))
    gp.observed(X, y)
    a0 = gp.active.dict_to_array(_params(gp, SE_var=1.2, SE_rate=[0.8, 1.0, 1.3], Noise_var=0.1, Bias_Bias=0.1))
    chain = a0 + 0.2 * rng.standard_normal((30, len(a0)))            # the reference notebooks average N = 30 ... 125 rows
    want = _single(gp, chain, var=True, noise=True)
    avg = gp.average(chain, var=True, noise=True, mixture=True, batch=16)
    assert set(avg) == {'mean', 'variance', 'std', 'mixture_mean', 'mixture_variance'}
    scale = max(1.0, np.abs(want['mean']).max())
    for k in ('mean', 'variance', 'std'):
        np.testing.assert_allclose(avg[k], want[k].mean(axis=0), rtol=0, atol=1e-8 * scale)
    np.testing.assert_allclose(avg['mixture_mean'], want['mean'].mean(axis=0), rtol=0, atol=1e-8 * scale)
    np.testing.assert_allclose(avg['mixture_variance'], want['variance'].mean(axis=0) + want['mean'].var(axis=0), rtol=0,
                               atol=1e-8 * scale)

    class Trace:                                                   # what a DataFrame trace looks like to average
        values = np.concatenate([chain, np.zeros((30, 2))], axis=1)
    avg2 = gp.average(Trace(), var=True, noise=True)
    for k in ('mean', 'variance', 'std'):
        np.testing.assert_array_equal(avg2[k], avg[k])
