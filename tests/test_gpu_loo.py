"""GPU tests of leave-one-out cross-validation from the Cholesky factor: GaussianProcess.loo / loo_chain / scores(loo=True)
and the C entry points g3_gp_loo (the Y half of the K^-1 sweep + one pass over Y's triangle) and g3_gp_loo_batched (one
workgroup per chain member up to N = 256).  References: tests/loo_reference.py -- the closed form from np.linalg.inv and N
refits of the oracle's GP.

fp64 bound: rtol 1e-8, the project's logp bar (kappa(K) ~ 1e2 for these inputs: the reference alone sits near 1e-14).  loc
= z - alpha / c is a difference of numbers the size of z (it is exactly 0 at N = 1): its 1e-8 is relative to max |z|.
fp32 bound: 10 x the measured |closed form in float32 - closed form in float64| on the same inputs (loo_reference.fp32_gap),
per quantity; the device sums in another order than NumPy."""
import functools

import numpy as np
import pytest

from loo_reference import brute_force, closed_form, fp32_gap, problem
from oracle import g3_oracle as orc

pytestmark = pytest.mark.gpu

RATE = np.array([0.9, 1.2])
SE_SPEC = ('SE', 1.3, RATE, None)
# Thresholds of the Y sweep (g3i_potri) with default knobs: panels are 128 wide up to 4096 padded rows, so N <= 128 is ONE
# panel, 129 .. 256 two panels on one stream, and from three panels on (N >= 257) the sweep runs on two streams.
ONE_PANEL_MAX, ONE_STREAM_MAX = 128, 256
SINGLE_N = [1, 97, ONE_PANEL_MAX, ONE_PANEL_MAX + 1, ONE_STREAM_MAX, ONE_STREAM_MAX + 1, 385, 1100]


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
    ref = closed_form(orc.GP(SE_SPEC, 0.1), X, y)
    for a in (X, y) + tuple(r for r in ref if isinstance(r, np.ndarray)):
        a.setflags(write=False)
    return X, y, ref


def _check64(r, loc, var, lp, what, zmax):
    e = (np.abs(r.mean - loc).max() / zmax, np.abs(r.variance / var - 1).max(), abs(r.logpredictive / lp - 1))
    print('loo %s: max err loc %.2e of max |z|, rel err variance %.2e logpredictive %.2e (bound 1e-8)' % ((what,) + e))
    np.testing.assert_allclose(r.mean, loc, rtol=1e-8, atol=1e-8 * zmax)
    np.testing.assert_allclose(r.variance, var, rtol=1e-8, atol=0)
    np.testing.assert_allclose(r.std, np.sqrt(var), rtol=1e-8, atol=0)
    assert abs(r.logpredictive - lp) <= 1e-8 * abs(lp)


@pytest.mark.parametrize('N', SINGLE_N)
def test_single_path_fp64_matches_the_closed_form(N):
    import g3py_amd as g3
    X, y, (alpha, c, loc, var, lp) = _reference(N)
    gp, p = _se_gp(g3, X, y)
    r = gp.loo(p, var=True)
    assert list(r) == ['mean', 'variance', 'std', 'logpredictive'] and r.mean.shape == (N,) and r.mean.dtype == np.float64
    _check64(r, loc, var, lp, 'N=%d' % N, np.abs(y).max())


def test_n97_matches_the_refits():
    import g3py_amd as g3
    X, y, _ = _reference(97)
    bf = brute_force(orc.GP(SE_SPEC, 0.1), X, y)
    gp, p = _se_gp(g3, X, y)
    r = gp.loo(p, var=True, median=True)
    _check64(r, bf['loc'], bf['var'], bf['logpredictive'], 'N=97 against 97 refits', np.abs(y).max())
    np.testing.assert_allclose(r.median, bf['median'], rtol=1e-8, atol=1e-8 * np.abs(y).max())


@pytest.mark.parametrize('N', [97, 129, 300])
def test_entry_point_pads_with_zeros_and_is_reproducible(N):
    """g3_gp_loo on the buffers logp left: alpha and kdiag themselves, their padding exactly 0, the same bits twice"""
    import g3py_amd as g3
    from g3py_amd import _lib
    X, y, (alpha, c, _, _, _) = _reference(N)
    gp, p = _se_gp(g3, X, y)
    gp.logp(p)
    dev, ch, Np = gp.device, gp._cache, _lib.roundup(N)
    Y = dev.alloc(Np, Np, np.float64)
    runs = []
    for _ in range(2):
        av, cv = dev.upload(np.full((1, Np), 7.0)), dev.upload(np.full((1, Np), 7.0))
        dev.gp_loo(N, ch['Kd'], ch['Wd'], ch['ad'], Y, av, cv)
        runs.append((dev.download(av)[0], dev.download(cv)[0]))
    (a1, c1), (a2, c2) = runs
    assert np.array_equal(a1, a2) and np.array_equal(c1, c2)
    assert np.all(a1[N:] == 0.0) and np.all(c1[N:] == 0.0) and len(a1) == Np
    np.testing.assert_allclose(a1[:N], alpha, rtol=1e-8, atol=1e-8 * np.abs(alpha).max())
    np.testing.assert_allclose(c1[:N], c, rtol=1e-8, atol=0)
    # Y is L^-T: upper triangular, and K^-1 = Y Y^T
    Yh = dev.download(Y)
    assert np.all(np.tril(Yh, -1) == 0.0)
    np.testing.assert_allclose(np.diag(Yh.dot(Yh.T))[:N], c, rtol=1e-8, atol=0)
    # the batched entry point on the same member (one workgroup up to N = 256, the single path above)
    av, cv = dev.upload(np.full((1, Np), 7.0)), dev.upload(np.full((1, Np), 7.0))
    dev.gp_loo_batched(1, N, ch['Kd'], (Np + 128) * Np, ch['Wd'], ch['ad'], Y if N > 256 else None, av, cv)
    np.testing.assert_allclose(dev.download(av)[0, :N], alpha, rtol=1e-8, atol=1e-8 * np.abs(alpha).max())
    np.testing.assert_allclose(dev.download(cv)[0, :N], c, rtol=1e-8, atol=0)
    assert np.all(dev.download(cv)[0, N:] == 0.0)


def test_composite_kernel():
    """SE x COS + MAT32 at N = 385"""
    import g3py_amd as g3
    N = 385
    X, y = problem(N, seed=2)
    gp = g3.GaussianProcess(space=X[:2], location=g3.Zero(), kernel=g3.SE(X) * g3.COS(X) + g3.MAT32(X))
    gp.observed(X, y)
    f, r2 = np.array([0.11, 0.07]), np.array([0.7, 0.5])
    p = _params(gp, SE_var=1.1, SE_rate=RATE, COS_freq=f, MAT32_var=0.6, MAT32_rate=r2, Noise_var=0.1)    # (COS in a product: unit variance)
    spec = ('sum', ('prod', ('SE', 1.1, RATE, None), ('COS', 1.0, f, None)), ('MAT32', 0.6, r2, None))
    _, _, loc, var, lp = closed_form(orc.GP(spec, 0.1), X, y)
    _check64(gp.loo(p, var=True), loc, var, lp, 'SE*COS+MAT32 N=385', np.abs(y).max())


def test_warped_gp_arcsinh():
    """mean / variance by Gauss-Hermite on (loc, sd), median and logpredictive through the warping, N = 200"""
    import g3py_amd as g3
    N = 200
    X, y = problem(N, seed=3)
    y = np.sinh(y)
    gp = g3.WarpedGaussianProcess(space=X[:2], location=g3.Zero(), kernel=g3.SE(X), mapping=g3.ArcsinhLinear())
    gp.observed(X, y)
    p = _params(gp, SE_var=1.3, SE_rate=RATE, Noise_var=0.1, ArcsinhLinear_shift=0.1, ArcsinhLinear_scale=0.8)
    o = orc.GP(SE_SPEC, 0.1, ('Zero',), ('ArcsinhLinear', 0.1, 0.8))
    _, _, loc, var, lp = closed_form(o, X, y)
    sd = np.sqrt(var)
    mean = o.gauss_hermite(lambda v: o.map(v), loc, sd)
    variance = o.gauss_hermite(lambda v: o.map(v) ** 2, loc, sd) - mean ** 2
    r = gp.loo(p, var=True, median=True)
    assert list(r) == ['mean', 'variance', 'std', 'median', 'logpredictive']
    scale = max(1.0, np.abs(mean).max())
    print('loo warped: max err mean %.2e variance %.2e median %.2e logpredictive rel %.2e' % (
        np.abs(r.mean - mean).max(), np.abs(r.variance - variance).max(), np.abs(r.median - o.map(loc)).max(),
        abs(r.logpredictive / lp - 1)))
    np.testing.assert_allclose(r.mean, mean, rtol=1e-8, atol=1e-8 * scale)
    np.testing.assert_allclose(r.variance, variance, rtol=1e-8, atol=1e-8 * scale ** 2)
    np.testing.assert_allclose(r.median, o.map(loc), rtol=1e-8, atol=1e-8 * scale)
    assert abs(r.logpredictive - lp) <= 1e-8 * abs(lp)


def _check32(got_loc, got_var, got_lp, gap, ref, what):
    l64, v64, p64 = ref
    e = (np.abs(got_loc - l64).max(), np.abs(got_var - v64).max(), abs(float(got_lp) - p64))
    print('loo fp32 %s: err loc %.3e (float32 closed form %.3e) var %.3e (%.3e) logpredictive %.3e (%.3e); bound 10 x' % (
        what, e[0], gap['loc'], e[1], gap['var'], e[2], gap['logpredictive']))
    assert e[0] <= 10 * gap['loc'] and e[1] <= 10 * gap['var'] and e[2] <= 10 * gap['logpredictive']


@pytest.mark.parametrize('N', [129, 385])
def test_single_path_fp32(N):
    """Measured on an MI355X, error against the float64 closed form, device / NumPy's float32 closed form (the bound is 10 x
    the latter): N = 129 loc 2.0e-6 / 7.5e-7, variance 1.1e-6 / 2.8e-7, logpredictive 2.6e-5 / 4.7e-6; N = 385 loc 1.4e-6 /
    2.1e-6, variance 5.6e-7 / 2.7e-7, logpredictive 1.5e-5 / 7.6e-5 (profiles/loo.md)."""
    import g3py_amd as g3
    X, y = problem(N, dtype=np.float32)
    gap, ref = fp32_gap(orc.GP(SE_SPEC, 0.1), X, y)
    gp, p = _se_gp(g3, X, y, dtype=np.float32)
    r = gp.loo(p, var=True)
    assert r.mean.dtype == np.float32
    _check32(r.mean.astype(np.float64), r.variance.astype(np.float64), r.logpredictive, gap, ref, 'N=%d' % N)


# ---------------------------------------------------------------------------------------------- chains
def _chain(gp, rng, rows=5):
    """rows with different variance, rates and noise"""
    out = []
    for _ in range(rows):
        out.append(gp.active.dict_to_array(_params(gp, SE_var=rng.uniform(0.8, 1.8), SE_rate=RATE * rng.uniform(0.8, 1.25, 2),
                                                   Noise_var=rng.uniform(0.05, 0.2))))
    return np.stack(out)


def _row_reference(gp, row, X, y, dtype=np.float64):
    v = {k: np.exp(val) for k, val in gp.active.array_to_dict(row).items()}
    o = orc.GP(('SE', float(v['GP_SE_var_log_']), v['GP_SE_rate_log_'], None), float(v['GP_Noise_var_log_']))
    return o


@pytest.mark.parametrize('N', [64, 100, 128, 200, 256, 300])
def test_chain_fp64(N):
    """N <= 256: the one-workgroup kernel (one block below 129, V21 on the MFMA path above); 300: member by member"""
    import g3py_amd as g3
    X, y, _ = _reference(N)
    gp, _ = _se_gp(g3, X, y)
    chain = _chain(gp, np.random.default_rng(N))
    got = gp.loo_chain(chain)
    assert got.shape == (5,) and got.dtype == np.float64
    single = np.array([gp.loo(gp.active.array_to_dict(r)).logpredictive for r in chain])
    ref = np.array([closed_form(_row_reference(gp, r, X, y), X, y)[4] for r in chain])
    print('loo_chain N=%d: max rel |chain - single| %.2e, |chain - closed form| %.2e' % (
        N, np.abs(got / single - 1).max(), np.abs(got / ref - 1).max()))
    np.testing.assert_allclose(got, single, rtol=1e-10, atol=0)
    np.testing.assert_allclose(got, ref, rtol=1e-8, atol=0)
    np.testing.assert_allclose(single, ref, rtol=1e-8, atol=0)
    # blocks of 2 + 2 + 1: a member's block mates are not its business (a block of one takes the single-member factorisation,
    # so not the same bits: rounding level)
    np.testing.assert_allclose(gp.loo_chain(chain, batch=2), got, rtol=1e-12, atol=0)


@pytest.mark.parametrize('N', [128, 256])
def test_chain_fp32(N):
    """Measured on an MI355X over the 5 rows, |chain - float64 closed form| / float32 closed form's own error (the bound is
    10 x the latter): N = 128 6.4e-6 .. 1.9e-5 / 3.8e-6 .. 2.0e-5, N = 256 1.5e-5 .. 4.8e-5 / 1.5e-5 .. 2.6e-5, the tightest row
    (N = 128, row 1) 1.9e-5 against an allowance of 3.8e-5; chain against the row's single loo at most 3.1e-5
    (profiles/loo.md)."""
    import g3py_amd as g3
    X, y = problem(N, dtype=np.float32)
    gp, _ = _se_gp(g3, X, y, dtype=np.float32)
    chain = _chain(gp, np.random.default_rng(N + 1))
    got = gp.loo_chain(chain)
    assert got.dtype == np.float32
    for i, row in enumerate(chain):
        gap, (_, _, p64) = fp32_gap(_row_reference(gp, row, X, y), X, y)
        one = gp.loo(gp.active.array_to_dict(row)).logpredictive
        print('loo_chain fp32 N=%d row %d: |chain - closed form| %.3e |chain - single| %.3e (float32 closed form %.3e; bound 10 x)' % (
            N, i, abs(float(got[i]) - p64), abs(float(got[i]) - float(one)), gap['logpredictive']))
        assert abs(float(got[i]) - p64) <= 10 * gap['logpredictive']
        assert abs(float(got[i]) - float(one)) <= 10 * gap['logpredictive']


def test_chain_member_whose_first_factorisation_fails():
    """duplicated inputs with the noise at 1e-12 in one row: that member goes through the jitter schedule on its own, the
    others do not notice.  (The row's variance is 1e6: with unit variance the pivots of the duplicates, 2e-12, survive the
    1e-16 rounding of the Schur complements and nothing fails; LAPACK's dpotrf stops at pivot 2 for this matrix.)  That
    row equals its single-path result at the bar every chain row is held to, 1e-10 relative: the failed member is
    refactored by the single member's own schedule, so both invert the same factor (measured on an MI355X: the same
    value to all printed digits, relative difference 0).  Its value is not compared with NumPy: ill-conditioned by
    construction."""
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
    one = gp.loo(gp.active.array_to_dict(chain[2]))
    assert gp._cache['stats']['tries'] >= 1 and not gp._cache['stats']['fallback']
    # the batched factorisation of this block: member 2, and only member 2, failed its first attempt and was retried
    values_b, _ = gp._values_rows(chain)
    X_, y_, N_, d, Np, kstride, _, Xd, ws = gp._chain_setup(5, 5, None)
    delta, _, _ = gp._chain_delta_or_bad(values_b, X_, y_, 5)
    st = gp._chain_factor_block(gp._chain_members(gp.f_kernel_noise, values_b, d, 5), delta, Xd, N_, d, ws['K'], kstride, ws['W'], ws['a'])
    assert st[2, 5] != 0 and st[2, 3] >= 1 and st[2, 4] == 0 and np.all(np.delete(st[:, 5], 2) == 0), st[:, 3:]
    got = gp.loo_chain(chain)
    clean = gp.loo_chain(np.delete(chain, 2, axis=0))
    np.testing.assert_allclose(np.delete(got, 2), clean, rtol=1e-12, atol=0)
    bound = 1e-10
    print('loo_chain jittered member: chain %.10e single %.10e rel diff %.2e (bound %.1e)' % (
        got[2], one.logpredictive, abs(got[2] / one.logpredictive - 1), bound))
    assert np.isfinite(got[2]) and got[2] != np.float32(-1e30)
    assert abs(got[2] - one.logpredictive) <= bound * abs(one.logpredictive)


def test_chain_sentinel_rows():
    """a row logp_chain sends to -1e30 (a mean that is not finite) gets the sentinel; its neighbours are untouched"""
    import g3py_amd as g3
    X, y, _ = _reference(97)
    gp = g3.GaussianProcess(space=X[:2], location=g3.Bias(), kernel=g3.SE(X))
    gp.observed(X, y)
    rows = []
    for bias in (0.1, np.inf, -0.2):
        rows.append(gp.active.dict_to_array(_params(gp, SE_var=1.3, SE_rate=RATE, Noise_var=0.1, Bias_Bias=bias)))
    chain = np.stack(rows)
    got = gp.loo_chain(chain)
    assert got[1] == np.float32(-1e30) and gp.logp_chain(chain)[1] == np.float32(-1e30)
    assert gp.loo(gp.active.array_to_dict(chain[1])).logpredictive == np.float32(-1e30)
    for i in (0, 2):
        one = gp.loo(gp.active.array_to_dict(chain[i])).logpredictive
        assert abs(got[i] - one) <= 1e-10 * abs(one)


# ---------------------------------------------------------------------------------------------- cache and scores
def test_loo_after_logp_builds_and_factors_nothing():
    """logp(p) then loo(p): the Gram and factorisation counters stay where logp put them (g3_prof_* tags `gram` and `potrf`,
    and the Gram launch counter); loo adds its triangular sweep (`trsm`) and its reduction"""
    import g3py_amd as g3
    X, y, (_, _, loc, var, lp) = _reference(385)
    dev = g3.Device(0)
    try:
        gp, p = _se_gp(g3, X, y, device=dev)
        dev.prof_enable(True)
        dev.prof_reset()
        gp.logp(p)
        grams, prof = dev.gram_path_stats(), dev.prof_collect()
        assert prof['gram']['count'] >= 1 and prof['potrf']['count'] >= 1
        r = gp.loo(p, var=True)
        grams2, prof2 = dev.gram_path_stats(), dev.prof_collect()
        assert grams2 == grams
        assert prof2['gram']['count'] == prof['gram']['count'] and prof2['potrf']['count'] == prof['potrf']['count']
        assert prof2['trsm']['count'] == prof['trsm']['count'] + 1 and prof2['reduce']['count'] == prof['reduce']['count'] + 1
        gp.loo(p, mean=False, std=False)                       # the vectors are kept with the factor: no device work at all
        prof3 = dev.prof_collect()
        assert all(prof3[k]['count'] == prof2[k]['count'] for k in prof2)
        _check64(r, loc, var, lp, 'after logp, N=385', np.abs(y).max())
        # the other order, and a gradient in between (dlogp shares the Y workspace)
        q = _params(gp, SE_var=1.0, SE_rate=RATE, Noise_var=0.2)
        first = gp.loo(q).logpredictive
        g = gp.dlogp(q)
        assert gp.loo(q).logpredictive == first and np.all(np.isfinite(g))
    finally:
        dev.close()


def test_scores_keys():
    import g3py_amd as g3
    X, y, (_, _, loc, var, lp) = _reference(97)
    gp, p = _se_gp(g3, X, y)
    gp.hidden = np.zeros(2)
    plain = gp.scores(p)
    assert list(plain) == ['_l1', '_l2']                       # exactly today's keys
    s = gp.scores(p, loo=True)
    assert list(s) == ['_l1', '_l2', '_loo_nlpd', '_loo_l1', '_loo_l2']
    r = gp.loo(p)
    assert s['_loo_nlpd'] == -r.logpredictive / 97
    assert abs(s['_loo_nlpd'] + lp / 97) <= 1e-8 * abs(lp / 97)
    np.testing.assert_allclose(s['_loo_l1'], np.mean(np.abs(loc - y)), rtol=1e-8)
    np.testing.assert_allclose(s['_loo_l2'], np.mean((loc - y) ** 2), rtol=1e-8)
    assert plain['_l1'] == s['_l1'] and plain['_l2'] == s['_l2']


def test_argument_checks():
    """sizes are refused with the number of the argument, as the neighbouring entry points do"""
    import g3py_amd as g3
    dev = g3.Device.default()
    lib, ctx = dev.lib, dev.ctx
    buf = dev.alloc(384, 128, np.float64)
    p = buf.ptr
    assert lib.g3_gp_loo(ctx, None, 100, 128, p, p, 0, p, 128, p, p) == -2
    assert lib.g3_gp_loo(ctx, p, 0, 128, p, p, 0, p, 128, p, p) == -3
    assert lib.g3_gp_loo(ctx, p, 129, 128, p, p, 0, p, 256, p, p) == -4          # ldl below roundup(N, 128)
    assert lib.g3_gp_loo(ctx, p, 100, 128, None, p, 0, p, 128, p, p) == -5
    assert lib.g3_gp_loo(ctx, p, 100, 128, p, p, 0, None, 128, p, p) == -8
    assert lib.g3_gp_loo(ctx, p, 100, 128, p, p, 0, p, 127, p, p) == -9
    assert lib.g3_gp_loo(ctx, p, 100, 128, p, p, 0, p, 128, p, None) == -11
    assert lib.g3_gp_loo_batched(ctx, 0, p, 100, 128, 256 * 128, p, p, 0, None, p, p) == -2
    assert lib.g3_gp_loo_batched(ctx, 4097, p, 100, 128, 256 * 128, p, p, 0, None, p, p) == -2
    assert lib.g3_gp_loo_batched(ctx, 1, p, 100, 128, 127 * 128, p, p, 0, None, p, p) == -6     # members would overlap
    assert lib.g3_gp_loo_batched(ctx, 1, p, 300, 384, 512 * 384, p, p, 0, None, p, p) == -10    # N > 256 needs the Y workspace
    assert lib.g3_gp_loo_batched(ctx, 1, p, 300, 384, 512 * 384, p, p, 0, None, None, None) == -10
    assert lib.g3_gp_loo_batched(ctx, 1, p, 100, 128, 256 * 128, p, p, 0, None, None, p) == -11
    assert lib.g3_gp_loo_batched(ctx, 1, p, 100, 128, 256 * 128, p, p, 0, None, p, None) == -12
    assert lib.g3_gp_loo(ctx, p, 100, 128, p, p, 7, p, 128, p, p) == -7 and lib.g3_gp_loo_batched(ctx, 1, p, 100, 128, 256 * 128, p, p, 7, None, p, p) == -9
