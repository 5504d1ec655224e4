"""GPU tests of appending observations without a refit: the C entry points g3_gp_append / g3_gp_cross_append
(include/g3hip_online.h) and EllipticalProcess.observe_more.  References: tests/append_reference.py -- SciPy's factor of the
whole N1 x N1 covariance from the oracle's kernel -- and the library's own g3_gp_factor / g3_gp_cross at N1, and a fresh
process observed on everything.

Bounds, the project's own: fp64 rtol 1e-8 on scalars and variances, atol 1e-8 max|.| on vectors and matrices; fp32 1e-4.  The
covariances (SE + noise 0.1, constant density, d = 3) have kappa ~ 1e2: the fp64 reference itself sits near 1e-14.

Every C-level case starts from buffers that hold NaN wherever the precondition promises nothing: the rows from n0 =
rounddown(N0, 128) on, the strict upper triangle, the slack columns behind Np1, the block inverses and a from n0 on."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import append_reference as ar
import stream_order as so
from stream_order import Call

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
D, P = ar.D, ar.P
SLACK = 128                 # columns of the buffers behind Np1: never read, never written
CASES = [(1, 1, F64), (100, 20, F64), (100, 28, F64), (100, 29, F64), (128, 1, F64), (128, 128, F64), (300, 1, F64),
         (300, 300, F64), (256, 3200, F64), (4224, 5, F64), (300, 1, F32), (300, 300, F32)]


def _tol(dt):
    return 1e-8 if np.dtype(dt) == F64 else 1e-4


@pytest.fixture(scope='module', autouse=True)
def _torch_runtime_first():
    """The stream-order cases below hand torch streams to the library, and torch brings a HIP runtime of its own: it is
    initialised here, before this module's contexts do any work, the order every program that uses both (bench.py, the
    multi-GPU helpers) has."""
    import torch
    torch.cuda.init()
    assert torch.cuda.is_available()


@pytest.fixture(scope='module')
def dev():
    import g3py_amd as g3
    d = g3.Device(0)
    yield d
    d.close()


def _prog(spec=ar.SPEC):
    from g3py_amd.device import compile_spec
    return compile_spec(spec, D)


def _nan(rows, cols, dt):
    return np.full((rows, cols), np.nan, dtype=dt)


class State:
    """the device operands of one append and host copies of what they held before it"""

    def __init__(self, dev, dt, N0, N1, X, y, prog):
        self.dev, self.dt, self.N0, self.N1, self.prog = dev, dt, N0, N1, prog
        self.n0, self.Np1, self.r = ar.plan(N0, N1)
        ld = self.Np1 + SLACK
        self.X, self.y = dev.upload(np.asarray(X, dtype=dt)), dev.upload(np.asarray(y, dtype=dt))
        self.K = dev.upload(_nan(self.Np1 + P, ld, dt))
        self.W = dev.upload(_nan(self.Np1, P, dt))
        self.a = dev.upload(_nan(1, ld, dt))
        self.st0 = dev.gp_factor(prog, self.X, N0, D, self.y, self.K, self.W, self.a)
        # what the precondition does not cover goes back to NaN
        K, W, a = dev.download(self.K, self.K.rows, ld), dev.download(self.W), dev.download(self.a, 1, ld)
        K[self.n0:] = np.nan
        K[np.triu_indices(self.Np1 + P, 1, ld)] = np.nan
        W[self.n0:] = np.nan
        a[0, self.n0:] = np.nan
        self.before = (K, W, a)
        self.restore()

    def restore(self):
        for d, h in zip((self.K, self.W, self.a), self.before):
            self.dev.copy_in(d, h)

    def append(self):
        return self.dev.gp_append(self.prog, self.X, self.N0, self.N1, D, self.y, self.K, self.W, self.a)

    def read(self):
        dev = self.dev
        return dev.download(self.K, self.K.rows, self.K.ld), dev.download(self.W), dev.download(self.a, 1, self.K.ld)


def _fresh(dev, dt, N, X, y, prog):
    """(lower factor Np x Np, block inverses, a, stats) of g3_gp_factor on buffers of its own"""
    Np = ar.roundup(N)
    K, W, a = dev.alloc(Np + P, Np, dt), dev.alloc_inverses(Np, dt), dev.alloc(1, Np, dt)
    st = dev.gp_factor(prog, dev.upload(np.asarray(X, dtype=dt)), N, D, dev.upload(np.asarray(y, dtype=dt)), K, W, a)
    return np.tril(dev.download(K, Np, Np)).astype(F64), dev.download(W).astype(F64), dev.download(a)[0].astype(F64), st


def _check_factor(got, want, tol, what):
    """(L, a, logdet, quad) against (L, a, logdet, quad)"""
    (L, a, logdet, quad), (Lr, ar_, logdet_r, quad_r) = got, want
    e = (np.abs(L - Lr).max() / np.abs(Lr).max(), np.abs(a - ar_).max() / np.abs(ar_).max(), abs(logdet - logdet_r) / abs(logdet_r),
         abs(quad / quad_r - 1))
    print('%s: max err L %.2e a %.2e of their max, rel err logdet %.2e quad %.2e (bound %.0e)' % ((what,) + e + (tol,)))
    np.testing.assert_allclose(L, Lr, rtol=0, atol=tol * np.abs(Lr).max(), err_msg=what + ': L')
    np.testing.assert_allclose(a, ar_, rtol=0, atol=tol * np.abs(ar_).max(), err_msg=what + ': a')
    assert abs(logdet - logdet_r) <= tol * abs(logdet_r), (what, logdet, logdet_r)
    assert abs(quad - quad_r) <= tol * abs(quad_r), (what, quad, quad_r)


# ---------------------------------------------------------------------------------------------- C level
@pytest.mark.parametrize('N0,m,dt', CASES, ids=['%d+%d-%s' % (a, b, np.dtype(c).name) for a, b, c in CASES])
def test_append_matches_scipy_and_a_fresh_factor(dev, N0, m, dt):
    N1 = N0 + m
    X, y, _ = ar.problem(N1)
    s = State(dev, dt, N0, N1, X, y, _prog())
    assert s.st0['tries'] == 0 and not s.st0['fallback'] and s.st0['info'] == 0
    st = s.append()
    assert (st['tries'], st['fallback'], st['info'], st['refused']) == (0, False, 0, False) and st['nonfinite'] == 0
    K, W, a = s.read()
    Kb, Wb, ab = s.before
    n0, Np1, tol = s.n0, s.Np1, _tol(dt)
    # nothing below n0 was written, nothing behind Np1 either
    assert so.same_bits(K[:n0], Kb[:n0]) and so.same_bits(W[:n0], Wb[:n0]) and so.same_bits(a[0, :n0], ab[0, :n0])
    assert np.isnan(K[:, Np1:]).all() and np.isnan(a[0, Np1:]).all()
    L = np.tril(K[:Np1, :Np1]).astype(F64)
    assert np.isfinite(L).all() and np.isfinite(W).all() and np.isfinite(a[0, :Np1]).all()
    got = (L, a[0, :Np1].astype(F64), st['logdet'], st['quad'])
    _check_factor(got, ar.reference(N1), tol, 'append %d -> %d against SciPy' % (N0, N1))
    Lf, Wf, af, stf = _fresh(dev, dt, N1, X, y, s.prog)
    _check_factor(got, (Lf, af, stf['logdet'], stf['quad']), tol, 'append %d -> %d against g3_gp_factor' % (N0, N1))
    np.testing.assert_allclose(W.astype(F64), Wf, rtol=0, atol=tol * np.abs(Wf).max(), err_msg='block inverses')
    # a second identical call gives identical bits
    s.restore()
    st2 = s.append()
    K2, W2, a2 = s.read()
    assert so.same_bits(K2, K) and so.same_bits(W2, W) and so.same_bits(a2, a)
    assert (st2['logdet'], st2['quad']) == (st['logdet'], st['quad'])


def test_thirty_single_appends_equal_one_append_of_thirty(dev):
    N0, m = 120, 30
    N1 = N0 + m
    X, y, _ = ar.problem(N1)
    prog = _prog()
    one = State(dev, F64, N0, N1, X, y, prog)
    st1 = one.append()
    K1, _, a1 = one.read()
    step = State(dev, F64, N0, N1, X, y, prog)      # buffers sized for N1, factored at N0
    for n in range(N0, N1):
        st = dev.gp_append(prog, step.X, n, n + 1, D, step.y, step.K, step.W, step.a)
        assert st['info'] == 0 and not st['refused']
    K, _, a = step.read()
    Np1 = one.Np1
    got = (np.tril(K[:Np1, :Np1]), a[0, :Np1], st['logdet'], st['quad'])
    _check_factor(got, (np.tril(K1[:Np1, :Np1]), a1[0, :Np1], st1['logdet'], st1['quad']), 1e-8, '30 x 1 against 1 x 30')
    Lf, _, af, stf = _fresh(dev, F64, N1, X, y, prog)
    _check_factor(got, (Lf, af, stf['logdet'], stf['quad']), 1e-8, '30 x 1 against g3_gp_factor')
    _check_factor(got, ar.reference(N1), 1e-8, '30 x 1 against SciPy')


def test_argument_checks_in_signature_order(dev):
    lib, ctx = dev.lib, dev.ctx
    prog, bad = _prog(), _prog()
    bad.nleaf = 99
    p, byref = 4096, C.byref          # any non-null pointer: a refused call launches nothing and reads nothing
    ok = dict(prog=byref(prog), X=p, N0=100, N1=129, ldx=D, d=D, delta=p, dt=0, K=p, ldk=256, W=p, a=p)
    out = (C.c_double * 8)()

    def call(**kw):
        v = dict(ok, **kw)
        return lib.g3_gp_append(ctx, v['prog'], v['X'], v['N0'], v['N1'], v['ldx'], v['d'], v['delta'], v['dt'], v['K'], v['ldk'],
                                v['W'], v['a'], kw.get('out', out))
    assert call(prog=None) == -2 and call(prog=byref(bad)) == -2
    assert call(X=None) == -3
    assert call(N0=0) == -4 and call(N0=0, N1=0) == -4
    assert call(N1=100) == -5 and call(N1=99) == -5
    assert call(ldx=2) == -6
    assert call(d=0) == -7 and call(d=41, ldx=41) == -7
    assert call(delta=None) == -8
    assert call(dt=7) == -9
    assert call(K=None) == -10
    assert call(ldk=128) == -11 and call(ldk=257) == -11          # below Np1 = 256; not a multiple of 16 bytes
    assert call(W=None) == -12
    assert call(a=None) == -13
    assert call(out=None) == -14
    assert call(X=None, N0=0, K=None) == -3                        # the first offence decides
    okc = dict(prog=byref(prog), Xs=p, M=10, ldxs=D, X=p, N0=100, N1=129, ldx=D, d=D, L=p, ldl=256, W=p, a=p, dt=0, V=p, ldv=256,
               mu=p, ss=p)

    def cross(**kw):
        v = dict(okc, **kw)
        return lib.g3_gp_cross_append(ctx, v['prog'], v['Xs'], v['M'], v['ldxs'], v['X'], v['N0'], v['N1'], v['ldx'], v['d'],
                                      v['L'], v['ldl'], v['W'], v['a'], v['dt'], v['V'], v['ldv'], v['mu'], v['ss'])
    assert cross(prog=None) == -2 and cross(Xs=None) == -3 and cross(M=0) == -4 and cross(ldxs=2) == -5 and cross(X=None) == -6
    assert cross(N0=0) == -7 and cross(N1=100) == -8 and cross(ldx=1) == -9 and cross(d=0) == -10 and cross(L=None) == -11
    assert cross(ldl=128) == -12 and cross(W=None) == -13 and cross(a=None) == -14 and cross(dt=5) == -15
    assert cross(V=None) == -16 and cross(ldv=255) == -17
    assert cross(Xs=None, L=None) == -3
    dev.sync()


@pytest.mark.parametrize('N0,m', [(100, 20), (300, 100)])
@pytest.mark.parametrize('M', [1, 100, 300])
def test_cross_append_matches_a_fresh_cross_solve(dev, N0, m, M):
    N1 = N0 + m
    X, y, Xs = ar.problem(N1, M)
    prog, cross = _prog(), _prog(ar.SE)
    s = State(dev, F64, N0, N1, X, y, prog)
    Mp, ld = ar.roundup(M), s.Np1 + SLACK
    Xsd = dev.upload(Xs)
    V, mu, ss = dev.upload(_nan(Mp, ld, F64)), dev.upload(_nan(1, Mp, F64)), dev.upload(_nan(1, Mp, F64))
    s.restore()
    # the cross solve at N0 needs the whole factor at N0: put it back, solve, then take away what the precondition leaves open
    dev.gp_factor(prog, s.X, N0, D, s.y, s.K, s.W, s.a)
    dev.gp_cross(cross, Xsd, M, s.X, N0, D, s.K, s.W, s.a, V, mu, ss)
    V0 = dev.download(V, Mp, ld)
    V0[:, s.n0:] = np.nan
    dev.copy_in(V, V0)
    dev.copy_in(mu, _nan(1, Mp, F64))
    s.restore()
    assert s.append()['info'] == 0
    dev.gp_cross_append(cross, Xsd, M, s.X, N0, N1, D, s.K, s.W, s.a, V, mu, ss)
    V1 = dev.download(V, Mp, ld)
    assert so.same_bits(V1[:, :s.n0], V0[:, :s.n0]) and np.isnan(V1[:, s.Np1:]).all() and np.isfinite(V1[:, :s.Np1]).all()
    # a fresh factor and cross solve at N1 on buffers of their own
    Np = s.Np1
    K, W, a = dev.alloc(Np + P, Np, F64), dev.alloc_inverses(Np, F64), dev.alloc(1, Np, F64)
    dev.gp_factor(prog, s.X, N1, D, s.y, K, W, a)
    Vf, muf, ssf = dev.alloc(Mp, Np, F64), dev.alloc(1, Mp, F64), dev.alloc(1, Mp, F64)
    dev.gp_cross(cross, Xsd, M, s.X, N1, D, K, W, a, Vf, muf, ssf)
    Vf, muf, ssf = dev.download(Vf), dev.download(muf, 1, M)[0], dev.download(ssf, 1, M)[0]
    got_mu, got_ss = dev.download(mu, 1, M)[0], dev.download(ss, 1, M)[0]
    print('cross append M=%d %d -> %d: max err V %.2e mu %.2e of their max, rel err ss %.2e (bound 1e-8)' % (
        M, N0, N1, np.abs(V1[:, :Np] - Vf).max() / np.abs(Vf).max(), np.abs(got_mu - muf).max() / np.abs(muf).max(),
        np.abs(got_ss / ssf - 1).max()))
    np.testing.assert_allclose(V1[:, :Np], Vf, rtol=0, atol=1e-8 * np.abs(Vf).max())
    np.testing.assert_allclose(got_mu, muf, rtol=0, atol=1e-8 * np.abs(muf).max())
    np.testing.assert_allclose(got_ss, ssf, rtol=1e-8, atol=0)
    # and the block formulas
    from oracle import g3_oracle as orc
    Lr, a_r, _, _ = ar.reference(N1)
    Vr, mur, ssr = ar.cross(orc.tt_to_num(orc.kernel_cov(ar.SE, Xs, X)), Lr, a_r, N1)
    np.testing.assert_allclose(V1[:M, :Np], Vr, rtol=0, atol=1e-8 * np.abs(Vr).max())
    np.testing.assert_allclose(got_mu, mur, rtol=0, atol=1e-8 * np.abs(mur).max())
    np.testing.assert_allclose(got_ss, ssr, rtol=1e-8, atol=0)


# ---------------------------------------------------------------------------------------------- stream order
def _adopted(monkeypatch, tmp_path):
    from test_gpu_kernel_variants import variant_context
    return variant_context(monkeypatch, tmp_path)


def _append_operands(run, bufs, N0, N1, M):
    """device operands in torch tensors: the factor at N0 with NaN wherever the precondition leaves open, staged"""
    dev = run.dev
    X, y, Xs = ar.problem(N1, M)
    prog, cross = _prog(), _prog(ar.SE)
    s = State(dev, F64, N0, N1, X, y, prog)
    Mp, ld = ar.roundup(M), s.Np1 + SLACK
    V, mu, ss = dev.upload(_nan(Mp, ld, F64)), dev.alloc(1, Mp, F64), dev.alloc(1, Mp, F64)
    dev.gp_factor(prog, s.X, N0, D, s.y, s.K, s.W, s.a)
    dev.gp_cross(cross, dev.upload(Xs), M, s.X, N0, D, s.K, s.W, s.a, V, mu, ss)
    V0 = dev.download(V, Mp, ld)
    V0[:, s.n0:] = np.nan
    return s, prog, cross, (X, y, Xs), V0


def test_append_synchronises_and_reads_inputs_in_stream_order(monkeypatch, tmp_path):
    """g3_gp_append has a host out-parameter: it drains the stream; its inputs are produced on the busy adopted stream"""
    import torch
    N0, N1 = 300, 429
    with _adopted(monkeypatch, tmp_path) as run:
        dev = run.dev
        s, prog, _, (X, y, _), _ = _append_operands(run, None, N0, N1, 1)
        stream = torch.cuda.Stream()
        dev.set_stream(stream.cuda_stream)
        bufs = so.Buffers(dev, stream)
        Xd, yd = bufs.inp('X', X, F64), bufs.inp('y', y[None, :], F64)
        K, W, a = (bufs.inp(n, h, F64, output=True) for n, h in zip('KWa', s.before))
        host = {}

        def append():
            out = (C.c_double * 8)()
            rc = dev.lib.g3_gp_append(dev.ctx, C.byref(prog), Xd.ptr, N0, N1, Xd.ld, D, yd.ptr, 0, K.ptr, K.ld, W.ptr, a.ptr, out)
            host['out'] = np.array(out[:])
            return rc

        def check(out, hst):
            Np1 = s.Np1
            got = (np.tril(out['K'][:Np1, :Np1]), out['a'][0, :Np1], hst['out'][0], hst['out'][1])
            _check_factor(got, ar.reference(N1), 1e-8, 'stream order')
            assert hst['out'][5] == 0 and hst['out'][6] == 0
        torch.cuda.synchronize()
        so.run_passes(dev, stream, bufs, [Call('g3_gp_append', append, True)], host, check, 'g3_gp_append 300 -> 429')
        dev.set_stream(None)


def test_cross_append_is_asynchronous_and_stream_ordered(monkeypatch, tmp_path):
    """g3_gp_cross_append returns while a marker queued before it is pending, and a copy queued behind it sees its outputs"""
    import torch
    N0, N1, M = 300, 429, 130
    with _adopted(monkeypatch, tmp_path) as run:
        dev = run.dev
        s, prog, cross, (X, y, Xs), V0 = _append_operands(run, None, N0, N1, M)
        s.restore()
        assert s.append()['info'] == 0
        K1, W1, a1 = s.read()
        stream = torch.cuda.Stream()
        dev.set_stream(stream.cuda_stream)
        bufs = so.Buffers(dev, stream)
        Xd, Xsd = bufs.inp('X', X, F64), bufs.inp('Xs', Xs, F64)
        K, W, a = (bufs.inp(n, h, F64) for n, h in zip('KWa', (K1, W1, a1)))
        V = bufs.inp('V', V0, F64, output=True)
        Mp = ar.roundup(M)
        mu, ss = bufs.out('mu', 1, Mp, F64), bufs.out('ss', 1, Mp, F64)

        def call():
            return dev.lib.g3_gp_cross_append(dev.ctx, C.byref(cross), Xsd.ptr, M, Xsd.ld, Xd.ptr, N0, N1, Xd.ld, D, K.ptr, K.ld,
                                              W.ptr, a.ptr, 0, V.ptr, V.ld, mu.ptr, ss.ptr)

        def check(out, hst):
            from oracle import g3_oracle as orc
            Lr, a_r, _, _ = ar.reference(N1)
            Vr, mur, ssr = ar.cross(orc.tt_to_num(orc.kernel_cov(ar.SE, Xs, X)), Lr, a_r, N1)
            np.testing.assert_allclose(out['V'][:M, :s.Np1], Vr, rtol=0, atol=1e-8 * np.abs(Vr).max())
            np.testing.assert_allclose(out['mu'][0, :M], mur, rtol=0, atol=1e-8 * np.abs(mur).max())
            np.testing.assert_allclose(out['ss'][0, :M], ssr, rtol=1e-8, atol=0)
        torch.cuda.synchronize()
        so.run_passes(dev, stream, bufs, [Call('g3_gp_cross_append', call, False)], {}, check, 'g3_gp_cross_append 300 -> 429',
                      after_each=True, snapshot=True)
        dev.set_stream(None)


# ---------------------------------------------------------------------------------------------- refusals
def test_a_zero_prior_diagonal_is_refused_and_nothing_is_written(dev):
    """a dot-product kernel without noise is 0 at x = 0: tt_to_cov would lift the whole diagonal, the append declines"""
    dot = _prog(('DOT', 1.3, np.ones(D), 0.0, 1, None))
    X = np.vstack([ar.problem(2)[0] + 0.5, np.zeros((1, D))])
    y = np.array([0.3, -0.2, 0.1])
    s = State(dev, F64, 2, 3, X, y, dot)
    st = s.append()
    assert st['refused'] and st['info'] == 0 and (st['logdet'], st['quad']) == (0.0, 0.0)
    for got, want in zip(s.read(), s.before):
        assert so.same_bits(got, want)
    # a NaN input: the diagonal holds a non-finite value
    Xn = np.vstack([X[:2], np.full((1, D), np.nan)])
    s = State(dev, F64, 2, 3, Xn, y, _prog())
    assert s.append()['refused']
    for got, want in zip(s.read(), s.before):
        assert so.same_bits(got, want)


def _duplicates(N0, m):
    X, y, _ = ar.problem(N0)
    return np.vstack([X, X[:m]]), np.concatenate([y, y[:m]])


@pytest.mark.parametrize('N0', [100, 128])
def test_duplicated_points_without_noise_fail_a_corner_pivot(dev, N0):
    """new points that repeat old ones make the covariance singular: the pivot flag names a row among the new ones"""
    X, y = _duplicates(N0, 20)
    s = State(dev, F64, N0, N0 + 20, X, y, _prog(ar.SE))
    assert s.st0['tries'] == 0 and s.st0['info'] == 0
    st = s.append()
    assert not st['refused'] and N0 < st['info'] <= N0 + 20, st
    K, W, a = s.read()
    assert so.same_bits(K[:s.n0], s.before[0][:s.n0]) and so.same_bits(a[0, :s.n0], s.before[2][0, :s.n0])


# ---------------------------------------------------------------------------------------------- process level
def _params(gp, **nat):
    p = gp.params_test
    by = {v.name: v for v in gp.model.vars}
    for k, val in nat.items():
        v = by[gp.name + '_' + k]
        p[v.key] = (np.log(val) if v.positive else np.asarray(val, dtype=float)) * np.ones(v.shape)
    return p


KINDS = {
    'gp': lambda g3, X, Xs, dt: g3.GaussianProcess(space=Xs, location=g3.Zero(), kernel=g3.SE(X), dtype=dt),
    'warped': lambda g3, X, Xs, dt: g3.WarpedGaussianProcess(space=Xs, location=g3.Bias(), kernel=g3.SE(X), mapping=g3.BoxCoxLinear(),
                                                            dtype=dt),
    'student': lambda g3, X, Xs, dt: g3.StudentTProcess(space=Xs, location=g3.Zero(), kernel=g3.SE(X), dtype=dt),
}
HYPERS = {'gp': {}, 'student': {},
          'warped': dict(Bias_Bias=0.2, BoxCoxLinear_shift=1.0, BoxCoxLinear_scale=1.0, BoxCoxLinear_power=1.2)}


def _make(kind, X, y, Xs, dt=F64, noisy=True):
    import g3py_amd as g3
    gp = KINDS[kind](g3, X, Xs, dt) if noisy else g3.GaussianProcess(space=Xs, location=g3.Zero(), kernel=g3.SE(X), noisy=False,
                                                                    dtype=dt)
    gp.observed(X, y)
    nat = dict(SE_var=1.3, SE_rate=ar.RATE, **HYPERS[kind])
    if noisy:
        nat['Noise_var'] = ar.NOISE
    return gp, _params(gp, **nat)


def _statistics(gp, p, loo=True):
    out = dict(logp=np.asarray(gp.logp(p)), dlogp=np.asarray(gp.dlogp(p)))
    pred = gp.predict(p, var=True)
    out.update(mean=pred.mean, variance=pred.variance)
    if loo and hasattr(gp, 'loo'):
        r = gp.loo(p, var=True)
        out.update(loo_mean=r.mean, loo_variance=r.variance, loo_logpredictive=np.asarray(r.logpredictive))
    return out


def _same_statistics(got, want, tol, what):
    assert set(got) == set(want)
    for k in want:
        g, w = np.asarray(got[k], dtype=F64), np.asarray(want[k], dtype=F64)
        print('%s %s: max err %.2e of max |.| = %.3e (bound %.0e)' % (what, k, np.abs(g - w).max() / (np.abs(w).max() or 1.0),
                                                                      np.abs(w).max(), tol))
        if k.endswith('variance') or g.ndim == 0:
            np.testing.assert_allclose(g, w, rtol=tol, atol=0, err_msg='%s: %s' % (what, k))
        else:
            np.testing.assert_allclose(g, w, rtol=0, atol=tol * np.abs(w).max(), err_msg='%s: %s' % (what, k))


@pytest.mark.parametrize('kind,dt', [('gp', F64), ('gp', F32), ('warped', F64), ('student', F64)],
                         ids=['gp-float64', 'gp-float32', 'warped-float64', 'student-float64'])
def test_observe_more_equals_a_fresh_process(kind, dt):
    N0, m1, m2, M = 300, 1, 150, 40
    X, y, Xs = ar.problem(N0 + m1 + m2, M)
    if kind == 'warped':
        y = np.abs(y) + 0.5                                        # inside BoxCox's domain
    gp, p = _make(kind, X[:N0], y[:N0], Xs, dt)
    gp.predict(p, var=True)                                        # a factor and a cross solve at the fixed space
    assert gp._cache['stats']['tries'] == 0
    K0 = gp._workspace['Kd']
    assert (K0.rows, K0.cols, K0.ld) == (384 + 128, 384, 384)      # never appended to: allocated as ever
    gp.observe_more(X[N0:N0 + m1], y[N0:N0 + m1], p)               # inside the last block
    assert gp.append_stats == dict(appended=1, cross_appended=1, refit=0)
    key = gp._cache['key']
    mid = gp.predict(p, var=True)
    assert gp._cache['key'] == key and gp._cache['stats']['tries'] == 0 and gp._cache['N'] == N0 + m1      # the cache was hit
    gp.observe_more(X[N0 + m1:], y[N0 + m1:], p)                   # across a block boundary: the workspace grows
    assert gp.append_stats == dict(appended=2, cross_appended=2, refit=0)
    assert gp.inputs.shape == (N0 + m1 + m2, D) and gp.is_observed and gp._cache['Kd'].ld >= 512
    got = _statistics(gp, p)
    assert gp.append_stats == dict(appended=2, cross_appended=2, refit=0)
    fresh, pf = _make(kind, X, y, Xs, dt)
    want = _statistics(fresh, pf)
    _same_statistics(got, want, _tol(dt), '%s %s' % (kind, np.dtype(dt).name))
    half, ph = _make(kind, X[:N0 + m1], y[:N0 + m1], Xs, dt)
    _same_statistics(dict(mean=mid.mean, variance=mid.variance), {k: v for k, v in _statistics(half, ph, loo=False).items()
                                                                  if k in ('mean', 'variance')}, _tol(dt), '%s after one point' % kind)
    for name in ('inputs', 'outputs', 'index', 'order'):
        np.testing.assert_array_equal(getattr(gp, name), getattr(fresh, name), err_msg=name)
    # observed() afterwards resets
    gp.observed(X[:N0], y[:N0])
    start, ps = _make(kind, X[:N0], y[:N0], Xs, dt)
    _same_statistics(_statistics(gp, p, loo=False), _statistics(start, ps, loo=False), _tol(dt), '%s after observed()' % kind)
    assert gp._workspace['Kd'].ld == 384 and gp.append_stats['appended'] == 2


def _refit_case(gp, p, Xn, yn, fresh, pf, what, params=None):
    before = dict(gp.append_stats)
    gp.observe_more(Xn, yn, params if params is not None else p)
    assert gp.append_stats == dict(before, refit=before['refit'] + 1), (what, gp.append_stats)
    got, want = _statistics(gp, p, loo=False), _statistics(fresh, pf, loo=False)
    _same_statistics(got, want, 1e-8, what)
    assert gp._cache['stats']['tries'] == fresh._cache['stats']['tries'], what
    return gp._cache['stats']['tries']


def test_everything_else_refits():
    N0, m, M = 200, 30, 20
    X, y, Xs = ar.problem(N0 + m, M)
    fresh, pf = _make('gp', X, y, Xs)
    # no cached factor
    gp, p = _make('gp', X[:N0], y[:N0], Xs)
    _refit_case(gp, p, X[N0:], y[N0:], fresh, pf, 'no cached factor')
    # a factor for other parameters
    gp, p = _make('gp', X[:N0], y[:N0], Xs)
    q = _params(gp, SE_var=0.7, SE_rate=ar.RATE, Noise_var=0.2)
    gp.logp(q)
    _refit_case(gp, p, X[N0:], y[N0:], fresh, pf, 'other params')
    # several GPUs
    gp, p = _make('gp', X[:N0], y[:N0], Xs)
    gp.distribute(None, 0, 1)
    before = dict(gp.append_stats)
    gp.observe_more(X[N0:], y[N0:], p)
    assert gp.append_stats == dict(before, refit=1)
    gp.undistribute()
    _same_statistics(_statistics(gp, p, loo=False), _statistics(fresh, pf, loo=False), 1e-8, 'distributed')
    # a jittered factor: duplicated inputs, no noise
    Xj, yj = _duplicates(60, 40)
    Xa, ya = np.vstack([Xj, X[N0:]]), np.concatenate([yj, y[N0:]])
    gp, p = _make('gp', Xj, yj, Xs, noisy=False)
    gp.logp(p)
    assert gp._cache['stats']['tries'] >= 1
    fj, pj = _make('gp', Xa, ya, Xs, noisy=False)
    assert _refit_case(gp, p, X[N0:], y[N0:], fj, pj, 'a jittered factor') >= 1
    # new points that repeat old ones, no noise: the corner's pivot fails, the refit jitters as the fresh process does
    Xd, yd = _duplicates(100, 20)
    gp, p = _make('gp', Xd[:100], yd[:100], Xs, noisy=False)
    gp.logp(p)
    assert gp._cache['stats']['tries'] == 0
    fd, pd = _make('gp', Xd, yd, Xs, noisy=False)
    assert _refit_case(gp, p, Xd[100:], yd[100:], fd, pd, 'duplicated points') >= 1


def test_one_point_appends_reallocate_o_log_times(monkeypatch):
    import g3py_amd as g3
    N0, m = 100, 40
    X, y, Xs = ar.problem(N0 + m, 5)
    gp, p = _make('gp', X[:N0], y[:N0], Xs)
    gp.logp(p)
    K0 = gp._workspace['Kd']
    assert (K0.rows, K0.cols, K0.ld) == (256, 128, 128)
    tall, real = [], g3.Device.alloc

    def counting(self, rows, cols, dtype, ld=None, zero=False):
        if rows == cols + 128 and rows > 256 - 1 and cols % 128 == 0:
            tall.append((rows, cols))
        return real(self, rows, cols, dtype, ld=ld, zero=zero)
    monkeypatch.setattr(g3.Device, 'alloc', counting)
    for n in range(N0, N0 + m):
        gp.observe_more(X[n:n + 1], y[n:n + 1], p)
    monkeypatch.undo()
    assert gp.append_stats == dict(appended=m, cross_appended=0, refit=0)
    bound = math.ceil(math.log(256 / 128, 1.5)) + 1
    print('Kd reallocations over %d one-point appends: %r (bound %d)' % (m, tall, bound))
    assert 1 <= len(tall) <= bound and gp._cache['Kd'].ld >= 256
    fresh, pf = _make('gp', X, y, Xs)
    _same_statistics(_statistics(gp, p), _statistics(fresh, pf), 1e-8, 'forty one-point appends')
