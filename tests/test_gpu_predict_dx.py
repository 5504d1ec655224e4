"""GPU tests of the gradients of the posterior location and variance with respect to the query inputs:
EllipticalProcess.predict_dx and the C entry points g3_gp_cross_dx (W = V L^-1 as one MFMA product, one pass over the M x N
pairs, the column splits added in a fixed order) and g3_gram_diag_dx.  References: tests/predict_dx_reference.py -- the
closed form from np.linalg.inv with a NumPy restatement of every leaf partial, and central differences through the oracle.

fp64 bound: the project's 1e-8, relative to the largest entry of each array (kappa(K) ~ 1e2 on loo_reference.problem's
inputs: the reference alone sits near 1e-13).  fp32 bound: 10 x the measured |closed form in float32 - closed form in
float64| on the same inputs (predict_dx_reference.fp32_gap), per quantity."""
import ctypes as C
import functools

import numpy as np
import pytest

import hostile_memory as hm
from dot_reference import kernel_cov_ext, zoo_inputs
from loo_reference import problem
from oracle import g3_oracle as orc
from predict_dx_reference import LEAVES, TREES, central, closed_form, d1, dkss, fp32_gap

pytestmark = pytest.mark.gpu

# Thresholds of cross_dx_kernel (g3_cross_dx.hip): a workgroup owns ROWS query rows (one per wave) and walks TILE-column tiles;
# the columns are split over about BLOCKS / ceil(M / ROWS) workgroups, each split a whole number of tiles, so a split holds
# more than one tile only when ceil(M / ROWS) > BLOCKS / ceil(N / TILE); a launch covers WINDOW columns of the query.
ROWS, TILE, WINDOW, BLOCKS = 4, 64, 8, 2048
RATE = np.array([0.9, 1.2, 0.7])
SE_SPEC = ('SE', 1.3, RATE, None)
KEYS = ('location', 'kernel_diag', 'kernel_sd')


def _params(gp, **nat):
    p = gp.params_test
    by = {v.name: v for v in gp.model.vars}
    for k, val in nat.items():
        v = by[gp.name + '_' + k]
        p[v.key] = (np.log(val) if v.positive else np.asarray(val, dtype=float)) * np.ones(v.shape)
    return p


def _spec_kernel(spec):
    """a kernel object with a fixed spec tree and no hyper-parameters: any leaf kind through the process API"""
    from g3py_amd.processes.hypers.kernels import Kernel

    class SpecKernel(Kernel):
        def __init__(self, tree):
            Kernel.__init__(self, None, 'Spec', var=1.0)
            self.tree = tree

        def spec(self, values, d):
            return self.tree
    return SpecKernel(spec)


def _spec_gp(g3, spec, X, y, dtype=np.float64, cls=None, noisy=True, **kw):
    gp = (cls or g3.GaussianProcess)(space=X[:2], kernel=_spec_kernel(spec), dtype=dtype, noisy=noisy,
                                     **dict(dict(location=g3.Zero()), **kw))
    gp.observed(X, y)
    return gp


def _queries(N, M, d, seed=0):
    rng = np.random.default_rng(5000 + 13 * N + M + seed)
    return rng.uniform(0.0, max(N, 2) ** (1.0 / d), (M, d))


@functools.lru_cache(maxsize=None)
def _reference(N, M, d=3):
    """problem, queries and closed form of the SE + noise 0.1 process, computed once for all tests"""
    X, y = problem(N, d=d)
    Xs = _queries(N, M, d)
    spec = ('SE', 1.3, RATE[:d], None)
    ref = closed_form(orc.GP(spec, 0.1), X, y, Xs)
    for a in (X, y, Xs) + ref:
        a.setflags(write=False)
    return X, y, Xs, spec, ref


def _check(r, ref, what, bound=1e-8, keys=KEYS):
    for k, want in zip(KEYS, ref):
        if k not in keys:
            continue
        scale = np.abs(want).max()
        err = np.abs(r[k] - want).max()
        print('predict_dx %s: %s max err %.2e of max |.| = %.3e (bound %.1e)' % (what, k, err / (scale or 1.0), scale, bound))
        assert r[k].shape == want.shape
        assert err <= bound * scale, (what, k, err, scale)


def _kept_jitter(gp, kn, X):
    """what the schedule of g3_gp_factor added to the diagonal of the factor the process holds: 0 when the first
    factorisation went through, else mean(diag K) * 1e-6f * 10^(tries - 1)"""
    st = gp._cache['stats']
    assert not st['fallback'], st
    if st['tries'] == 0:
        return 0.0
    return float(np.diag(kernel_cov_ext(kn, X)).mean() * np.float32(1e-6) * np.float32(10) ** (st['tries'] - 1))


def _run(gp, p, Xs, **kw):
    return gp.predict_dx(p, space=Xs, kernel_sd=True, **kw)


# ------------------------------------------------------------------ 1. fp64 against the closed form
@pytest.mark.parametrize('M', [1, 65, 130])
@pytest.mark.parametrize('N', [1, 97, 128, 129, 300])
def test_sizes_fp64(N, M):
    import g3py_amd as g3
    X, y, Xs, spec, ref = _reference(N, M)
    gp = _spec_gp(g3, spec, X, y)
    r = _run(gp, _params(gp, Noise_var=0.1), Xs)
    assert list(r) == list(KEYS) and r.location.dtype == np.float64
    _check(r, ref, 'N=%d M=%d' % (N, M))


@pytest.mark.parametrize('N,M', [(TILE, ROWS), (TILE + 1, ROWS + 1), (300, ROWS * (BLOCKS // 5)), (300, ROWS * (BLOCKS // 5) + 1)])
def test_row_group_tile_and_split_thresholds(N, M):
    """one row group and one tile / one more of each; with ceil(N / TILE) = 5, the last M whose BLOCKS // 5 = 409 row groups
    leave five splits of one tile, and the first whose 410 leave four: three splits of two tiles, the last one short"""
    import g3py_amd as g3
    X, y, Xs, spec, ref = _reference(N, M)
    gp = _spec_gp(g3, spec, X, y)
    _check(_run(gp, _params(gp, Noise_var=0.1), Xs), ref, 'N=%d M=%d' % (N, M))


@pytest.mark.parametrize('d', [1, WINDOW, WINDOW + 1, 40])
def test_column_windows(d):
    """d = 1; one window, two windows; d = 40 with a 32-column leaf inside columns 4 .. 35: five windows"""
    import g3py_amd as g3
    N, M = 97, 9
    X, y = problem(N, d=d)
    Xs = _queries(N, M, d)
    r = np.linspace(0.5, 0.9, d)
    if d == 40:
        rest = np.r_[0:4, 36:40]
        spec = ('sum', ('SE', 1.0, r[4:36], np.arange(4, 36)), ('MAT32', 0.5, r[rest], rest))
    else:
        spec = ('SE', 1.3, r, None)
    gp = _spec_gp(g3, spec, X, y)
    _check(_run(gp, _params(gp, Noise_var=0.1), Xs), closed_form(orc.GP(spec, 0.1), X, y, Xs), 'd=%d' % d)


def _zoo_problem(spec, N=97, M=65, d=3, seed=7):
    X, Xs = zoo_inputs(spec, N, d, seed), zoo_inputs(spec, M, d, seed + 1)
    y = np.sin(X.sum(axis=1)) + 0.3 * np.random.default_rng(seed).standard_normal(N)
    return X, y, Xs


@pytest.mark.parametrize('name', sorted(LEAVES) + sorted(TREES))
def test_every_leaf_and_mixed_trees(name):
    """every leaf kind alone and three trees (products of two and of three factors, scale, shift, dims subsets) at N = 97,
    M = 65; inputs strictly positive where BW occurs.  SIN, with its positive exponent as written, is no covariance on its
    own: K + 0.1 I is indefinite on these inputs, the factor goes through the jitter schedule, and the closed form is taken
    at the factor that was kept, as for any jittered factor"""
    import g3py_amd as g3
    spec = dict(LEAVES, **TREES)[name]
    X, y, Xs = _zoo_problem(spec)
    gp = _spec_gp(g3, spec, X, y)
    r = _run(gp, _params(gp, Noise_var=0.1), Xs)
    o = orc.GP(spec, 0.1)
    jitter = _kept_jitter(gp, o.kn, X)
    assert (jitter > 0) == (name in ('SIN', '2*MAT52*SIN+0.1+noise')), (name, gp._cache['stats'])
    _check(r, closed_form(o, X, y, Xs, jitter=jitter), name)


def test_noise_flag_means_prior_and_warping():
    import g3py_amd as g3
    X, y, Xs, spec, ref = _reference(97, 65)
    o = orc.GP(spec, 0.1)
    gp = _spec_gp(g3, spec, X, y)
    p = _params(gp, Noise_var=0.1)
    _check(_run(gp, p, Xs, noise=True), closed_form(o, X, y, Xs, noise=True), 'noise=True')
    _check(_run(gp, p, Xs, prior=True), closed_form(o, X, y, Xs, prior=True), 'prior=True')
    only = gp.predict_dx(p, space=Xs, kernel_diag=False)
    assert list(only) == ['location'] and np.array_equal(only.location, _run(gp, p, Xs).location)
    # an unobserved process falls back to the prior
    un = g3.GaussianProcess(space=X[:2], location=g3.Zero(), kernel=_spec_kernel(spec))
    _check(_run(un, _params(un, Noise_var=0.1), Xs), closed_form(o, X, y, Xs, prior=True), 'unobserved')
    coeff = np.array([0.3, -0.2, 0.15])
    gp = _spec_gp(g3, spec, X, y, location=g3.Bias())
    _check(_run(gp, _params(gp, Noise_var=0.1, Bias_Bias=0.3), Xs), closed_form(orc.GP(spec, 0.1, ('Bias', 0.3)), X, y, Xs), 'Bias')
    gp = _spec_gp(g3, spec, X, y, location=g3.Linear())
    _check(_run(gp, _params(gp, Noise_var=0.1, Linear_Constant=0.1, Linear_Coeff=coeff), Xs),
           closed_form(orc.GP(spec, 0.1, ('Linear', 0.1, coeff)), X, y, Xs), 'Linear')
    # a warped process: the latent gradients, with the observations pulled back through the mapping
    yw = np.sinh(y)
    gp = _spec_gp(g3, spec, X, yw, cls=g3.WarpedGaussianProcess, mapping=g3.ArcsinhLinear())
    _check(_run(gp, _params(gp, Noise_var=0.1, ArcsinhLinear_shift=0.1, ArcsinhLinear_scale=0.8), Xs),
           closed_form(orc.GP(spec, 0.1, ('Zero',), ('ArcsinhLinear', 0.1, 0.8)), X, yw, Xs), 'warped')


# ------------------------------------------------------------------ 2. fp32
@pytest.mark.parametrize('N,M', [(97, 65), (300, 130)])
def test_fp32_within_ten_times_the_float32_closed_form(N, M):
    import g3py_amd as g3
    X, y, Xs, spec, _ = _reference(N, M)
    gap, ref = fp32_gap(orc.GP(spec, 0.1), X, y, Xs)
    gp = _spec_gp(g3, spec, X.astype(np.float32), y.astype(np.float32), dtype=np.float32)
    r = _run(gp, _params(gp, Noise_var=0.1), Xs.astype(np.float32))
    for k, want in zip(KEYS, ref):
        err = np.abs(r[k].astype(np.float64) - want).max()
        print('predict_dx fp32 N=%d M=%d: %s err %.2e, float32 closed form %.2e (bound 10 x)' % (N, M, k, err, gap[k]))
        assert r[k].dtype == np.float32 and err <= 10 * gap[k]


# ------------------------------------------------------------------ 3. central differences through the oracle
def test_matches_central_differences_of_the_oracle():
    import g3py_amd as g3
    X, y, Xs, spec, _ = _reference(97, 9)
    dloc, ddiag = central(orc.GP(spec, 0.1), X, y, Xs, 1e-5)
    gp = _spec_gp(g3, spec, X, y)
    r = gp.predict_dx(_params(gp, Noise_var=0.1), space=Xs)
    for k, want in (('location', dloc), ('kernel_diag', ddiag)):
        err, scale = np.abs(r[k] - want).max(), np.abs(want).max()
        print('predict_dx against central differences: %s max err %.2e of %.3e (bound 1e-6)' % (k, err / scale, scale))
        assert err <= 1e-6 * scale


# ------------------------------------------------------------------ 4. the entry points
class _Buffers:
    """the operands of g3_gp_cross_dx on the factor logp and a location left, every one embedded in hostile memory: NaN
    around what is read, a canary around what is written, ldg > d"""

    def __init__(self, N, M, dtype=np.float64):
        import g3py_amd as g3
        from g3py_amd import _lib
        from g3py_amd.device import compile_spec
        self.N, self.M, self.d = N, M, 3
        self.X, self.y, self.Xs, self.spec, _ = _reference(N, M)
        gp = _spec_gp(g3, self.spec, self.X, self.y)
        p = _params(gp, Noise_var=0.1)
        gp.logp(p)
        gp.location(p, space=self.Xs)
        self.gp, self.dev, ch = gp, gp.device, gp._cache
        dev, d = self.dev, self.d
        self.Np, self.Mp = _lib.roundup(N), _lib.roundup(M)
        Np, Mp, sl = self.Np, self.Mp, hm.slack(dtype)
        Y = dev.alloc(Np, Np, dtype)
        vec = dev.alloc(2, Np, dtype)
        dev.gp_loo(N, ch['Kd'], ch['Wd'], ch['ad'], Y, vec, dev.wrap(vec.offset(1), 1, Np, Np, dtype, keep=vec))
        self.prog = compile_spec(self.spec, d)
        self.own = {}

        def put(name, a, rows, ld, fill):
            self.own[name] = hm.embed(dev, a, rows, ld, dtype, fill)
        put('Xs', self.Xs, M, d + 3, hm.NAN_BYTE)
        put('X', self.X, N, d + 1, hm.NAN_BYTE)
        put('alpha', dev.download(vec, 1, Np), 1, Np + sl, hm.NAN_BYTE)
        put('V', dev.download(ch['cross']['out'][0], Mp, Np), Mp, Np + sl, hm.NAN_BYTE)
        put('Y', dev.download(Y), Np, Np + sl, hm.NAN_BYTE)
        self.fresh_outputs()

    def fresh_outputs(self):
        sl = hm.slack(np.float64)
        for name, shape, ld in (('W', (self.Mp, self.Np), self.Np + sl), ('dmu', (self.M, self.d), self.d + 5),
                                ('dss', (self.M, self.d), self.d + 5), ('dk', (self.M, self.d), self.d + 5)):
            self.own[name] = hm.embed(self.dev, shape, shape[0], ld, np.float64, hm.CANARY_BYTE)

    def view(self, name):
        return self.own[name][0]

    def args(self, **over):
        v = self.view
        a = dict(prog=C.byref(self.prog), Xs=v('Xs').ptr, M=self.M, ldxs=v('Xs').ld, X=v('X').ptr, N=self.N, ldx=v('X').ld, d=self.d,
                 dt=0, alpha=v('alpha').ptr, V=v('V').ptr, ldv=v('V').ld, Y=v('Y').ptr, ldy=v('Y').ld, W=v('W').ptr, ldw=v('W').ld,
                 dmu=v('dmu').ptr, dss=v('dss').ptr, ldg=v('dmu').ld)
        a.update(over)
        return [a[k] for k in ('prog', 'Xs', 'M', 'ldxs', 'X', 'N', 'ldx', 'd', 'dt', 'alpha', 'V', 'ldv', 'Y', 'ldy', 'W', 'ldw',
                               'dmu', 'dss', 'ldg')]

    def call(self, **over):
        return self.dev.lib.g3_gp_cross_dx(self.dev.ctx, *self.args(**over))

    def block(self, name):
        return self.own[name][1].block()

    def inputs_untouched(self):
        for name in ('Xs', 'X', 'alpha', 'V', 'Y'):
            hm.check_untouched(self.dev, self.own[name][1], None, name)


@pytest.mark.parametrize('N,M', [(97, 65), (300, 130)])
def test_entry_points_on_hostile_memory(N, M):
    b = _Buffers(N, M)
    o = orc.GP(b.spec, 0.1)
    A = np.linalg.inv(orc.tt_to_cov(kernel_cov_ext(o.kn, b.X)))
    alpha = A.dot(b.y)
    k, g = d1(b.spec, b.Xs, b.X)
    w = k.dot(A)
    want_mu, want_ss = np.einsum('j,ijc->ic', alpha, g), 2 * np.einsum('ij,ijc->ic', w, g)
    assert b.call() == 0
    b.dev.sync()
    b.inputs_untouched()
    full = np.ones((M, b.d), dtype=bool)
    hm.check_untouched(b.dev, b.own['dmu'][1], full, 'dmu')
    hm.check_untouched(b.dev, b.own['dss'][1], full, 'dss')
    hm.check_untouched(b.dev, b.own['W'][1], np.ones((b.Mp, b.Np), dtype=bool), 'W')
    dmu, dss, W = b.block('dmu'), b.block('dss'), b.block('W')
    for name, got, want in (('dmu', dmu, want_mu), ('dss', dss, want_ss), ('W', W[:M, :N], w)):
        err, scale = np.abs(got - want).max(), np.abs(want).max()
        print('g3_gp_cross_dx N=%d M=%d: %s max err %.2e of %.3e (bound 1e-8)' % (N, M, name, err / scale, scale))
        assert err <= 1e-8 * scale
    assert not W[:, N:].any() and not W[M:, :].any()
    # the derivative of the prior diagonal
    dkv = b.view('dk')
    assert b.dev.lib.g3_gram_diag_dx(b.dev.ctx, C.byref(b.prog), b.view('Xs').ptr, M, b.view('Xs').ld, b.d, 0, dkv.ptr, dkv.ld) == 0
    hm.check_untouched(b.dev, b.own['dk'][1], full, 'dk')
    np.testing.assert_allclose(b.block('dk'), dkss(b.spec, b.Xs), rtol=0, atol=1e-8)
    tree = TREES['POL*SE+COS']
    from g3py_amd.device import compile_spec
    assert b.dev.lib.g3_gram_diag_dx(b.dev.ctx, C.byref(compile_spec(tree, b.d)), b.view('Xs').ptr, M, b.view('Xs').ld, b.d, 0,
                                     dkv.ptr, dkv.ld) == 0
    want = dkss(tree, b.Xs)
    assert np.abs(b.block('dk') - want).max() <= 1e-8 * np.abs(want).max()
    # the same bits twice; either output alone has the bits of the joint call
    b.fresh_outputs()
    assert b.call() == 0
    hm.same_bits(dmu, b.block('dmu'), None, 'dmu, second call')
    hm.same_bits(dss, b.block('dss'), None, 'dss, second call')
    b.fresh_outputs()
    assert b.call(dss=None, V=None, Y=None, W=None) == 0
    hm.same_bits(dmu, b.block('dmu'), None, 'dmu alone')
    hm.check_untouched(b.dev, b.own['dss'][1], None, 'dss of a call without it')
    hm.check_untouched(b.dev, b.own['W'][1], None, 'W of a call without dss')
    b.fresh_outputs()
    assert b.call(dmu=None, alpha=None) == 0
    hm.same_bits(dss, b.block('dss'), None, 'dss alone')
    hm.check_untouched(b.dev, b.own['dmu'][1], None, 'dmu of a call without it')


def test_argument_codes_and_a_refused_call_writes_nothing():
    b = _Buffers(97, 9)
    refusals = [(dict(prog=None), -2), (dict(Xs=None), -3), (dict(M=0), -4), (dict(ldxs=b.d - 1), -5), (dict(X=None), -6),
                (dict(N=0), -7), (dict(ldx=b.d - 1), -8), (dict(d=0), -9), (dict(d=41), -9), (dict(dt=2), -10),
                (dict(alpha=None), -11), (dict(V=None), -12), (dict(ldv=b.Np - 1), -13), (dict(ldv=b.Np + 1), -13),
                (dict(Y=None), -14), (dict(ldy=b.Np - 1), -15), (dict(ldy=b.Np + 1), -15), (dict(W=None), -16),
                (dict(ldw=b.Np - 1), -17), (dict(ldw=b.Np + 1), -17), (dict(dmu=None, dss=None), -18), (dict(ldg=b.d - 1), -20)]
    for over, code in refusals:
        assert b.call(**over) == code, (over, code)
    assert b.dev.lib.g3_gp_cross_dx(None, *b.args()) == -1
    dk, xs, lib, ctx = b.view('dk'), b.view('Xs'), b.dev.lib, b.dev.ctx
    prog = C.byref(b.prog)
    for args, code in (((None, xs.ptr, 9, xs.ld, b.d, 0, dk.ptr, dk.ld), -2), ((prog, None, 9, xs.ld, b.d, 0, dk.ptr, dk.ld), -3),
                       ((prog, xs.ptr, 0, xs.ld, b.d, 0, dk.ptr, dk.ld), -4), ((prog, xs.ptr, 9, b.d - 1, b.d, 0, dk.ptr, dk.ld), -5),
                       ((prog, xs.ptr, 9, xs.ld, 41, 0, dk.ptr, dk.ld), -6), ((prog, xs.ptr, 9, xs.ld, b.d, 2, dk.ptr, dk.ld), -7),
                       ((prog, xs.ptr, 9, xs.ld, b.d, 0, None, dk.ld), -8), ((prog, xs.ptr, 9, xs.ld, b.d, 0, dk.ptr, b.d - 1), -9)):
        assert lib.g3_gram_diag_dx(ctx, *args) == code, code
    b.dev.sync()
    b.inputs_untouched()
    for name in ('W', 'dmu', 'dss', 'dk'):
        hm.check_untouched(b.dev, b.own[name][1], None, name + ' after refused calls')


# ------------------------------------------------------------------ 5. a query row holding NaN
def test_nan_query_row_gives_zero_rows_and_leaves_the_others_alone():
    import g3py_amd as g3
    X, y, Xs, spec, _ = _reference(97, 65)
    bad = Xs.copy()
    bad[3, 1] = np.nan

    def run(S):
        gp = _spec_gp(g3, spec, X, y)
        return _run(gp, _params(gp, Noise_var=0.1), S)
    r, clean, short = run(bad), run(Xs), run(np.delete(Xs, 3, axis=0))
    keep = np.arange(65) != 3
    for k in KEYS:
        assert not r[k][3].any(), k
        hm.same_bits(clean[k][keep], r[k][keep], None, k + ' beside a NaN row')
        hm.same_bits(short[k], r[k][keep], None, k + ' without that row')


# ------------------------------------------------------------------ 6. a jitter-rescued factor
def test_jittered_factor_is_differentiated_as_it_was_kept():
    """duplicated inputs and no noise: the first factorisation fails and the schedule of g3_gp_factor adds
    jitter = mean(diag K) * 1e-6f * 10^(tries - 1) to the diagonal.  Both sides then invert K + jitter I, whose condition
    number kappa is what each loses: bound 100 kappa eps, relative to the largest entry."""
    import g3py_amd as g3
    X0, y0 = problem(60, d=3)
    X, y = np.concatenate([X0, X0[:40]]), np.concatenate([y0, y0[:40]])
    Xs = _queries(60, 17, 3)
    gp = _spec_gp(g3, SE_SPEC, X, y, noisy=False)
    r = _run(gp, gp.params_test, Xs)
    st = gp._cache['stats']
    K = kernel_cov_ext(SE_SPEC, X)
    jitter = _kept_jitter(gp, SE_SPEC, X)
    assert jitter > 0, st
    kappa = np.linalg.cond(K + jitter * np.eye(len(X)))
    bound = 100 * kappa * np.finfo(np.float64).eps
    print('jittered factor: tries %d jitter %.3e kappa %.2e bound %.2e' % (st['tries'], jitter, kappa, bound))
    assert bound < 1e-4
    _check(r, closed_form(orc.GP(SE_SPEC, None), X, y, Xs, jitter=jitter), 'jittered', bound=bound)


# ------------------------------------------------------------------ 7. call order: the cached L^-T
def test_call_order_does_not_change_the_bits():
    import g3py_amd as g3
    X, y, Xs, spec, _ = _reference(300, 65)
    other = _queries(300, 33, 3, seed=1)

    def new():
        gp = _spec_gp(g3, spec, X, y)
        return gp, _params(gp, Noise_var=0.1)
    gp, p = new()
    fresh = _run(gp, p, Xs)

    def same(r, what):
        for k in KEYS:
            hm.same_bits(fresh[k], r[k], None, '%s: %s' % (what, k))
    gp, p = new()
    same(_run(gp, p, Xs), 'another process')
    gp.dlogp(p)
    assert gp._cache.get('dx') is not None
    same(_run(gp, p, Xs), 'predict_dx -> dlogp -> predict_dx')
    gp, p = new()
    gp.loo(p)
    same(_run(gp, p, Xs), 'loo -> predict_dx')
    gp, p = new()
    gp.predict(p, space=Xs, var=True)
    _run(gp, p, other)
    same(_run(gp, p, Xs), 'predict -> predict_dx at another space -> predict_dx')
