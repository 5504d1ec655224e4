"""GPU tests of the reverse mode through the Cholesky factor: g3_potrf_vjp (CholeskyRobust.grad, g3py/libs/tensors.py:224-260),
g3_gram_vjp (the covariance adjoint pulled back to the kernel parameters) and the Python layers over them --
Device.potrf_vjp / gram_vjp, CholeskyRobust.grad, factor_vjp of the Gaussian and the Student-t process.
Reference: oracle.cholesky_grad through tests/vjp_reference.py.

fp64 bound: 1e-8 of the Frobenius norm, the project's fp64 bar (the formulation itself, restated in NumPy, sits at 1e-15:
test_vjp_host.py).  fp32 bound: 10 x vjp_reference.fp32_gap(n), the measured |cholesky_grad in float32 - in float64| on the
same inputs; the device sums in another order than NumPy.  Nothing here uses finite differences."""
import numpy as np
import pytest
import scipy.linalg

import hostile_memory as hm
import vjp_reference as vr
from hostile_memory import CANARY_BYTE, NAN_BYTE
from oracle import g3_oracle as orc

pytestmark = pytest.mark.gpu

# the panel and stream thresholds of the Y sweep (test_gpu_loo.py): one panel up to 128, one stream up to 256, two streams
# from 257 on; with them padding, one / two / three+ 128-blocks and a block count that is no power of two
SIZES = [1, 97, 128, 129, 256, 257, 385, 1100]


@pytest.fixture(scope='module')
def dev():
    import g3py_amd as g3
    return g3.Device.default()


@pytest.fixture(scope='module')
def dirty():
    d = hm.dirty_device()
    yield d
    d.close()


def _params(gp, **nat):
    p = gp.params_test
    by = {v.name: v for v in gp.model.vars}
    for k, val in nat.items():
        v = by[gp.name + '_' + k]
        p[v.key] = (np.log(val) if v.positive else np.asarray(val, dtype=float)) * np.ones(v.shape)
    return p


def _vjp(dev, L, Lbar, dtype=np.float64):
    n = len(L)
    Kb = dev.upload(np.full((n, n), 7.0, dtype=dtype))          # neither zero nor the result
    dev.potrf_vjp(dev.upload(L, dtype=dtype), dev.upload(Lbar, dtype=dtype), n, Kb)
    return dev.download(Kb)


def _rel(got, ref):
    return float(np.linalg.norm(np.asarray(got, dtype=np.float64) - ref) / np.linalg.norm(ref))


# ------------------------------------------------------------------------------------------------ 1. parity, fp64
@pytest.mark.parametrize('n', SIZES)
def test_fp64_matches_the_oracle(dev, n):
    p = vr.problem(n)
    ref = vr.reference(p['L'], p['Lbar'])
    got = _vjp(dev, p['L'], vr.with_nan_above(p['Lbar']))
    err = _rel(got, ref)
    print('potrf_vjp fp64 n=%d: rel Frobenius error %.2e (bound 1e-8)' % (n, err))
    assert got.dtype == np.float64 and got.shape == (n, n)
    assert np.all(np.triu(got, 1) == 0.0)
    assert err <= 1e-8


# ------------------------------------------------------------------------------------------------ 2. fp32
@pytest.mark.parametrize('n', [128, 200, 385])
def test_fp32_within_ten_times_the_float32_gap(dev, n):
    gap, ref64, L32, B32 = vr.fp32_gap(n)
    got = _vjp(dev, L32, vr.with_nan_above(B32), np.float32)
    err = _rel(got, ref64)
    print('potrf_vjp fp32 n=%d: rel Frobenius error %.2e, fp32_gap %.2e (bound 10 x gap)' % (n, err, gap))
    assert got.dtype == np.float32
    assert np.all(np.triu(got, 1) == 0.0)
    assert err <= 10 * gap


# ------------------------------------------------------------------------------------------------ 3. adjoint identity
@pytest.mark.parametrize('n', [200, 385])
def test_adjoint_identity_with_the_exact_forward_mode(dev, n):
    """<tril Lbar, dL> = <Kbar, tril dK> for a random symmetric dK and dL = L Phi(L^-1 dK L^-T)"""
    p = vr.problem(n)
    Kbar = _vjp(dev, p['L'], vr.with_nan_above(p['Lbar']))
    dL = vr.forward_mode(p['L'], p['dK'])
    lhs, rhs = float(np.sum(np.tril(p['Lbar']) * dL)), float(np.sum(Kbar * np.tril(p['dK'])))
    print('adjoint identity n=%d: lhs %.15e rhs %.15e, rel %.2e (bound 1e-8)' % (n, lhs, rhs, abs(lhs - rhs) / abs(rhs)))
    assert abs(lhs - rhs) <= 1e-8 * abs(rhs)


# ------------------------------------------------------------------------------------------------ 4. tt_to_num, kept factor
def test_cholesky_robust_grad_uses_the_factor_the_forward_call_kept(dev):
    """a rank-deficient K (duplicated inputs, no noise): the forward call goes through the jitter schedule, and grad is
    oracle.cholesky_grad at the factor it kept"""
    from g3py_amd.libs.tensors import CholeskyRobust
    p = vr.problem(97)
    X = np.concatenate([p['X'][:60], p['X'][:37]])                  # 37 duplicated rows
    K = np.asarray(orc.GP(vr.SE_SPEC, None).prior_kernel(X, False), dtype=np.float64)
    op = CholeskyRobust(device=dev)
    L = op(K)
    assert op.last['tries'] > 0 or op.last['fallback']
    Lbar = vr.with_nan_above(p['Lbar'])
    got, = op.grad([K], [Lbar])
    ref = vr.reference(L, p['Lbar'])
    err = _rel(got, ref)
    print('CholeskyRobust.grad, rank-deficient K (tries %d, fallback %s): rel error %.2e (bound 1e-8)'
          % (op.last['tries'], op.last['fallback'], err))
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == K.shape
    assert np.all(np.isfinite(got))
    assert err <= 1e-8
    # the input's dtype comes back
    got32, = op.grad([K.astype(np.float32)], [Lbar.astype(np.float32)])
    assert got32.dtype == np.float32 and np.all(np.isfinite(got32))


def test_an_infinite_entry_of_lbar_is_scrubbed_as_tt_to_num_does(dev):
    """one +Inf in the lower triangle of Lbar: the product L^T Lbar gets +-Inf and NaN (0 * Inf) in that column, and
    tt_to_num turns them into 1e10 and 0 before Phi (tensors.py:90-92, 255)"""
    n = 97
    p = vr.problem(n)
    L = p['L']
    Lbar = np.tril(p['Lbar'])
    Lbar[40, 13] = np.inf
    with np.errstate(invalid='ignore'):
        P = L.T.dot(Lbar)
    assert np.isnan(P).any() and np.isinf(P).any()
    P = np.where(np.isnan(P), 0.0, np.where(np.isinf(P), 1e10, P))
    P = vr.phi(P)
    s = scipy.linalg.solve_triangular(L, scipy.linalg.solve_triangular(L, P.T, lower=True, trans='T').T, lower=True, trans='T')
    ref = np.tril(s + s.T) - np.diag(np.diag(s))
    got = _vjp(dev, L, vr.with_nan_above(Lbar))
    err = _rel(got, ref)
    print('potrf_vjp with one +Inf in Lbar: rel error %.2e (bound 1e-8)' % err)
    assert np.all(np.isfinite(got))
    assert err <= 1e-8


# ------------------------------------------------------------------------------------------------ 5. memory contract
def _hostile_run(dv, L, Lbar, n, dt):
    """every operand inside NaN / canary guards with slack in its leading dimension; returns Kbar's n x n block after
    checking that the inputs are unchanged byte for byte and nothing outside the block was written"""
    ld = n + hm.slack(dt)
    Ld, Lo = hm.embed(dv, L.astype(dt), n, ld, dt, NAN_BYTE)
    Bd, Bo = hm.embed(dv, Lbar.astype(dt), n, ld, dt, NAN_BYTE)
    Kd, Ko = hm.embed(dv, (n, n), n, ld, dt, CANARY_BYTE)
    dv.potrf_vjp(Ld, Bd, n, Kd)
    dv.sync()
    hm.check_untouched(dv, Lo, what='L')
    hm.check_untouched(dv, Bo, what='Lbar')
    whole = hm.check_untouched(dv, Ko, np.ones((n, n), bool), what='Kbar')
    return Ko.block(whole)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_memory_contract_and_reproducibility(dev, dirty, dtype):
    import g3py_amd as g3
    n = 200
    p = vr.problem(n)
    L = vr.with_nan_above(p['L'])              # only the lower triangles are read
    Lbar = vr.with_nan_above(p['Lbar'])
    fresh = g3.Device(0)
    try:
        first = _hostile_run(fresh, L, Lbar, n, dtype)
        second = _hostile_run(fresh, L, Lbar, n, dtype)
    finally:
        fresh.close()
    used = _hostile_run(dirty, L, Lbar, n, dtype)
    plain = _vjp(dev, np.tril(p['L']), Lbar, dtype)
    hm.same_bits(first, second, what='fresh context, second call')
    hm.same_bits(first, used, what='used context')
    hm.same_bits(first, plain, what='plain buffers on the default context')
    assert np.all(np.triu(first, 1) == 0.0)
    ref = vr.reference(p['L'].astype(dtype).astype(np.float64), np.tril(p['Lbar']).astype(dtype).astype(np.float64))
    assert _rel(first, ref) <= (1e-8 if dtype == np.float64 else 10 * vr.fp32_gap(n)[0])


# ------------------------------------------------------------------------------------------------ 6. g3_gram_vjp
PROGRAMS = {
    'se_noise': (2, ('sum', ('SE', 1.3, vr.RATE, None), ('NOISE', 0.1))),
    'mat52cos_rq_noise': (3, ('sum', ('sum', ('prod', ('MAT52', 1.1, np.array([0.9, 1.2, 0.7]), None),
                                               ('COS', 1.0, np.array([0.11, 0.07, 0.05]), None)),
                                      ('RQ', 0.6, np.array([0.7, 0.5, 0.8]), 1.7, None)), ('NOISE', 0.1))),
}


@pytest.mark.parametrize('N', [97, 300])
def test_gram_vjp_equals_gram_grad_on_the_same_weight(dev, N):
    """Kbar = tril(G) with the diagonal halved, G = alpha alpha^T - K^-1: g3_gram_vjp is g3_gram_grad on (K^-1, alpha) -- the
    same kernels in the same order, only the weight is formed differently"""
    from g3py_amd.device import compile_spec
    from loo_reference import problem as loo_problem
    moved = {'table': 0, 'generated': 0, 'interpreted': 0}
    for name, (d, spec) in PROGRAMS.items():
        X, y = loo_problem(N, d=d)
        K = np.asarray(orc.GP(('SE', 1.3, np.ones(d), None), 0.1).prior_kernel(X, True), dtype=np.float64)
        Kinv = np.linalg.inv(K)
        Kinv = 0.5 * (Kinv + Kinv.T)
        alpha = Kinv.dot(y)
        G = np.outer(alpha, alpha) - Kinv
        Kbar = vr.phi(G)
        prog = compile_spec(spec, d)
        gmap = dev.grad_layout(prog)
        Xd = dev.upload(X)
        want = dev.gram_grad(prog, gmap, Xd, N, d, dev.upload(np.tril(Kinv)), dev.upload(alpha))
        before = dev.grad_path_stats()
        got = dev.gram_vjp(prog, gmap, Xd, N, d, dev.upload(vr.with_nan_above(Kbar)))
        after = dev.grad_path_stats()
        again = dev.gram_vjp(prog, gmap, Xd, N, d, dev.upload(vr.with_nan_above(Kbar)))
        err = np.linalg.norm(got - want) / np.linalg.norm(want)
        print('gram_vjp %s N=%d: %d slots, rel error against gram_grad %.2e (bound 1e-12), paths %s -> %s'
              % (name, N, gmap.nslots, err, before, after))
        assert got.shape == (gmap.nslots,) and np.all(np.isfinite(got))
        assert err <= 1e-12
        assert np.array_equal(got, again)
        step = {k: after[k] - before[k] for k in after}
        assert sum(step.values()) == 1, step
        for k, v in step.items():
            moved[k] += v
    # between the two programs the compile-time table and the generated (or, without hipRTC, the interpreted) kernel ran
    assert moved['table'] == 1 and moved['generated'] + moved['interpreted'] == 1, moved


# ------------------------------------------------------------------------------------------------ 7. end to end
def _logp_lbar(y, scale_of):
    """Lbar of the log marginal likelihood as a function of the factor: -diag(1 / L_ii) + s tril((L^-T a) a^T), a = L^-1 delta
    (delta = y: Zero location, identity mapping), s = scale_of(|a|^2) -- the density's d logp / d |a|^2 = -s / 2"""
    def lbar(L):
        a = scipy.linalg.solve_triangular(L, y, lower=True)
        u = scipy.linalg.solve_triangular(L, a, lower=True, trans='T')
        return -np.diag(1.0 / np.diag(L)) + scale_of(float(a.dot(a))) * np.tril(np.outer(u, a))
    return lbar


@pytest.mark.parametrize('kind', ['GP', 'TP'])
def test_factor_vjp_of_the_log_likelihood_reproduces_dlogp(kind):
    import g3py_amd as g3
    N = 200
    pr = vr.problem(N)
    X, y = pr['X'], pr['y']
    if kind == 'GP':
        gp = g3.GaussianProcess(space=X[:2], location=g3.Zero(), kernel=g3.SE(X))
        nat = dict(SE_var=1.3, SE_rate=vr.RATE, Noise_var=0.1)
        scale_of = lambda quad: 1.0
    else:
        gp = g3.StudentTProcess(space=X[:2], location=g3.Zero(), kernel=g3.SE(X))
        nat = dict(SE_var=1.3, SE_rate=vr.RATE, Noise_var=0.1, Freedom_degree=3.5)
        # the Student-t density's own scale of the quadratic term, (nu + N) / (nu - 2 + quad), as dlogp takes it
        scale_of = lambda quad: float(gp._dlogp_scale(gp._nu(gp._values(p)[0]), quad, N, {}))
    gp.observed(X, y)
    p = _params(gp, **nat)
    want = np.asarray(gp.dlogp(p), dtype=np.float64)
    seen = []

    def lbar(L):
        seen.append(_logp_lbar(y, scale_of)(L))
        return seen[-1]
    got = gp.factor_vjp(p, lbar)
    same = gp.factor_vjp(p, seen[0])
    assert got.shape == want.shape and got.dtype == gp.dtype
    assert np.array_equal(got, same)                         # the callable form and the array form: the same bits
    at = np.cumsum([0] + [v.size for v in gp.model.vars])
    for i, v in enumerate(gp.model.vars):
        g, w = got[at[i]:at[i + 1]], want[at[i]:at[i + 1]]
        if 'Freedom' in v.name:
            assert np.all(g == 0.0)                          # the covariance does not depend on it
            continue
        print('%s factor_vjp %s: %s against dlogp %s' % (kind, v.name, g, w))
        np.testing.assert_allclose(g, w, rtol=1e-8, atol=0)


def test_factor_vjp_leaves_the_location_entry_zero():
    import g3py_amd as g3
    N = 200
    pr = vr.problem(N)
    X, y = pr['X'], pr['y']
    gp = g3.GaussianProcess(space=X[:2], location=g3.Bias(), kernel=g3.SE(X))
    gp.observed(X, y)
    p = _params(gp, SE_var=1.3, SE_rate=vr.RATE, Noise_var=0.1, Bias_Bias=0.4)
    got = gp.factor_vjp(p, _logp_lbar(y - 0.4, lambda quad: 1.0))
    want = np.asarray(gp.dlogp(p), dtype=np.float64)
    at = np.cumsum([0] + [v.size for v in gp.model.vars])
    for i, v in enumerate(gp.model.vars):
        g, w = got[at[i]:at[i + 1]], want[at[i]:at[i + 1]]
        if 'Bias' in v.name:
            assert np.all(g == 0.0) and np.all(w != 0.0)
        else:
            np.testing.assert_allclose(g, w, rtol=1e-8, atol=0)
