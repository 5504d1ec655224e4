"""GPU tests of leave-fold-out cross-validation from the Cholesky factor: GaussianProcess.cv / scores(cv=...) and the C entry
point g3_gp_cv (K^-1, one gather launch per group of folds, the batched factorisation and leave-one-out launches on the
gathered members, one scatter launch).  References: tests/cv_reference.py -- the closed form from np.linalg.inv and per-fold
refits of the oracle's GP.

Inputs: SE + noise 0.1 on loo_reference.problem, kappa(K) in the hundreds; by Cauchy interlacing every A_II is as well
conditioned as K, so no fold needs jitter and `info` must be all zero.

fp64 bound: the one of test_gpu_loo.py, for the same reason -- rtol 1e-8 on the variances and on both scores, 1e-8 of max |z|
on the means (differences of numbers the size of z).  fp32 bound: per quantity, 10 x the measured |closed form in float32 -
closed form in float64| on the same inputs (cv_reference.fp32_gap): the project's leave-one-out policy.

The file's name puts it behind test_gpu_distributed.py in the suite's file order on purpose.  Until that file's multi-rank
tests have spawned their ranks no test opens the GPU in the pytest process itself; with this file in front of them (as
test_gpu_cv.py) the in-process one-rank RCCL start-up of test_gpu_dot_kernels.py::test_distribute_world_one_equals_one_gpu failed
later in the same run (ncclCommInitRank: unhandled cuda error), twice out of two runs of the whole suite, and passed without."""
import functools

import numpy as np
import pytest

from cv_reference import as_folds, closed_form, fp32_gap, refits
from loo_reference import problem
from oracle import g3_oracle as orc

pytestmark = pytest.mark.gpu

RATE = np.array([0.9, 1.2])
SE_SPEC = ('SE', 1.3, RATE, None)


def _blocks(*sizes):
    edges = np.concatenate([[0], np.cumsum(sizes)])
    return [np.arange(edges[i], edges[i + 1]) for i in range(len(sizes))]


def _uncovered(N):
    labels = np.arange(N) % 4
    labels[np.arange(N) % 3 == 0] = -1
    return labels


# name -> (N, folds): the shapes at which the entry point takes another path
CASES = {
    'singletons': (97, 97),                            # F = N folds of one point: leave-one-out; Sp = 128, 97 members
    'four_of_75': (300, 4),                            # Sp = 128
    'mixed_sizes': (300, _blocks(1, 50, 129, 120)),    # mixed padding, Sp = 256: the second block of the one-workgroup kernels
    'interleaved': (385, np.arange(385) % 5),          # non-contiguous gather, 77 per fold
    'two_large': (600, _blocks(257, 343)),             # Sp = 384: lock-step sweep with two members, loo one member at a time
    'one_of_all': (300, 1),                            # Sp = 384, a group of one: the single-matrix sweep; the prior
    'uncovered': (300, _uncovered(300)),               # a third of the points in no fold
}


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
def _reference(case):
    """problem and closed form of the SE + noise 0.1 process for a case, computed once for all tests"""
    N, folds = CASES[case]
    X, y = problem(N)
    ref = closed_form(orc.GP(SE_SPEC, 0.1), X, y, folds)
    for a in (X, y) + tuple(r for r in ref.values() if isinstance(r, np.ndarray)):
        a.setflags(write=False)
    return X, y, folds, ref


def _check64(r, loc, var, lp, joint, what, zmax):
    h = np.isfinite(loc)
    e = (np.abs(r.mean[h] - loc[h]).max() / zmax, np.abs(r.variance[h] / var[h] - 1).max(), abs(r.logpredictive / lp - 1),
         abs(r.logpredictive_joint / joint - 1))
    print('cv %s: max err loc %.2e of max |z|, rel err variance %.2e logpredictive %.2e joint %.2e (bound 1e-8)' % ((what,) + e))
    assert np.all(r.info == 0), r.info
    np.testing.assert_allclose(r.mean, loc, rtol=1e-8, atol=1e-8 * zmax)          # (NaN in no fold on both sides)
    np.testing.assert_allclose(r.variance, var, rtol=1e-8, atol=0)
    np.testing.assert_allclose(r.std, np.sqrt(var), rtol=1e-8, atol=0)
    assert abs(r.logpredictive - lp) <= 1e-8 * abs(lp)
    assert abs(r.logpredictive_joint - joint) <= 1e-8 * abs(joint)


@pytest.mark.parametrize('case', list(CASES))
def test_fp64_matches_the_closed_form(case):
    import g3py_amd as g3
    X, y, folds, ref = _reference(case)
    N = len(y)
    gp, p = _se_gp(g3, X, y)
    r = gp.cv(p, folds, var=True)
    assert list(r) == ['mean', 'variance', 'std', 'logpredictive', 'logpredictive_joint', 'folds', 'info']
    assert r.mean.shape == (N,) and r.mean.dtype == np.float64
    want = as_folds(folds, N)
    assert len(r.folds) == len(want) == len(r.info) and all(np.array_equal(a, b) for a, b in zip(r.folds, want))
    _check64(r, ref['loc'], ref['var'], ref['logpredictive'], ref['logpredictive_joint'], case, np.abs(y).max())
    out = np.isin(np.arange(N), ref['held'], invert=True)
    assert np.all(np.isnan(r.mean[out])) and np.all(np.isnan(r.variance[out])) and np.all(np.isfinite(r.mean[~out]))
    if case == 'uncovered':
        assert out.sum() == 100
    if case == 'singletons':                      # ... is leave-one-out, on every key
        one = gp.loo(p, var=True, median=True)
        rm = gp.cv(p, folds, var=True, median=True)
        for k in ('mean', 'median'):
            np.testing.assert_allclose(rm[k], one[k], rtol=1e-8, atol=1e-8 * np.abs(y).max())
        for k in ('variance', 'std'):
            np.testing.assert_allclose(rm[k], one[k], rtol=1e-8, atol=0)
        assert abs(rm.logpredictive - one.logpredictive) <= 1e-8 * abs(one.logpredictive)
        assert abs(rm.logpredictive_joint - one.logpredictive) <= 1e-8 * abs(one.logpredictive)
    if case == 'one_of_all':                      # ... is the prior: its joint log predictive is loglike
        ll = gp.loglike(p)
        print('cv one fold of everything: joint %.12e loglike %.12e' % (r.logpredictive_joint, ll))
        assert abs(r.logpredictive_joint - ll) <= 1e-8 * abs(ll)


def test_n97_matches_the_refits():
    import g3py_amd as g3
    X, y = problem(97)
    rf = refits(orc.GP(SE_SPEC, 0.1), X, y, 4)
    gp, p = _se_gp(g3, X, y)
    r = gp.cv(p, 4, var=True, median=True)
    assert list(r) == ['mean', 'variance', 'std', 'median', 'logpredictive', 'logpredictive_joint', 'folds', 'info']
    _check64(r, rf['loc'], rf['var'], rf['logpredictive'], rf['logpredictive_joint'], 'N=97 against 4 refits', np.abs(y).max())
    np.testing.assert_allclose(r.median, rf['median'], rtol=1e-8, atol=1e-8 * np.abs(y).max())
    np.testing.assert_allclose(r.mean, rf['mean'], rtol=1e-8, atol=1e-8 * np.abs(y).max())
    np.testing.assert_allclose(r.variance, rf['variance'], rtol=1e-8, atol=0)


# ---------------------------------------------------------------------------------------------- the entry point
SENTINEL_ROW = 7.0


def _outputs(dev, Np):
    """resid and pvar as rows 1 and 3 of a five-row buffer: NaN where the call must write, sentinel rows around them"""
    img = np.full((5, Np), SENTINEL_ROW)
    img[1] = img[3] = np.nan
    buf = dev.upload(img)
    return buf, dev.wrap(buf.offset(1), 1, Np, Np, np.float64, keep=buf), dev.wrap(buf.offset(3), 1, Np, Np, np.float64, keep=buf)


def test_entry_point_on_the_buffers_logp_left():
    """g3_gp_cv itself, N = 300 and folds 75 x 4: resid / pvar, their padding exactly 0, NaN-prefilled outputs overwritten up to
    roundup(N, 128) and nothing beyond, the same bits twice, K^-1 as g3_gp_dlogp leaves it; then three of the four folds:
    the observations in no fold exactly 0"""
    import g3py_amd as g3
    from g3py_amd import _lib
    X, y, folds, ref = _reference('four_of_75')
    N, Np = 300, _lib.roundup(300)
    gp, p = _se_gp(g3, X, y)
    gp.dlogp(p)
    kinv_dlogp = np.tril(gp.device.download(gp._workspace['Kinv'])[:N, :N])
    gp.logp(p)
    dev, ch = gp.device, gp._cache
    Y, Kinv, alpha = dev.alloc(Np, Np, np.float64), dev.upload(np.full((Np, Np), np.nan)), dev.alloc(1, Np, np.float64)
    fl = as_folds(folds, N)
    idx, ptr = np.concatenate(fl).astype(np.int32), np.concatenate([[0], np.cumsum([len(f) for f in fl])]).astype(np.int64)
    runs = []
    for _ in range(2):
        buf, resid, pvar = _outputs(dev, Np)
        fold, info = dev.gp_cv(N, ch['Kd'], ch['Wd'], ch['ad'], Y, Kinv, alpha, idx, ptr, resid, pvar)
        runs.append((dev.download(buf), fold.copy(), info.copy()))
    (img, fold, info), (img2, fold2, info2) = runs
    assert img.tobytes() == img2.tobytes() and fold.tobytes() == fold2.tobytes()
    assert np.all(img[[0, 2, 4]] == SENTINEL_ROW), 'a store outside resid / pvar'
    assert not np.isnan(img[[1, 3]]).any(), 'an entry below roundup(N, 128) that was not written'
    assert np.all(img[1, N:] == 0.0) and np.all(img[3, N:] == 0.0) and np.all(info == 0) and info.shape == (4,)
    np.testing.assert_allclose(img[1, :N], ref['resid'], rtol=1e-8, atol=1e-8 * np.abs(y).max())
    np.testing.assert_allclose(img[3, :N], ref['pvar'], rtol=1e-8, atol=0)
    np.testing.assert_allclose(fold, ref['fold'], rtol=1e-8, atol=0)
    got = np.tril(dev.download(Kinv)[:N, :N])
    np.testing.assert_allclose(got, kinv_dlogp, rtol=0, atol=1e-8 * np.abs(kinv_dlogp).max())
    # folds 0, 1 and 3 only: fold 2's observations are in no fold
    buf, resid, pvar = _outputs(dev, Np)
    keep = [fl[0], fl[1], fl[3]]
    idx3, ptr3 = np.concatenate(keep).astype(np.int32), np.array([0, 75, 150, 225], dtype=np.int64)
    fold3, info3 = dev.gp_cv(N, ch['Kd'], ch['Wd'], ch['ad'], Y, Kinv, alpha, idx3, ptr3, resid, pvar)
    img3 = dev.download(buf)
    assert np.all(img3[1, 150:225] == 0.0) and np.all(img3[3, 150:225] == 0.0) and np.all(img3[[1, 3], N:] == 0.0)
    for row in (1, 3):
        assert np.array_equal(np.delete(img3[row], np.s_[150:225]), np.delete(img[row], np.s_[150:225]))
    assert np.array_equal(fold3, fold[[0, 1, 3]]) and np.all(info3 == 0)
    assert np.all(img3[[0, 2, 4]] == SENTINEL_ROW)


def test_argument_checks():
    """bad folds are refused with the number of the argument (13 idx, 14 ptr, 15 nfold) and nothing is written"""
    import ctypes as C
    import g3py_amd as g3
    dev = g3.Device.default()
    lib, ctx = dev.lib, dev.ctx
    N, Np = 300, 384
    work = dev.alloc(Np + 128, Np, np.float64)
    p = work.ptr
    out = dev.upload(np.full((2, Np), SENTINEL_ROW))
    idx = np.arange(N, dtype=np.int32)
    ptr = np.array([0, 75, 150, 225, 300], dtype=np.int64)

    def call(idx=idx, ptr=ptr, nfold=4, **kw):
        a = dict(L=p, N=N, ldl=Np, W=p, a=p, dt=0, Y=p, ldy=Np, Kinv=p, ldc=Np, alpha=p, resid=out.ptr, pvar=out.offset(1))
        a.update(kw)
        fold, info = np.full((4100, 2), SENTINEL_ROW), np.full(4100, 7, dtype=np.int32)
        rc = lib.g3_gp_cv(ctx, a['L'], a['N'], a['ldl'], a['W'], a['a'], a['dt'], a['Y'], a['ldy'], a['Kinv'], a['ldc'], a['alpha'],
                          idx.ctypes.data_as(C.c_void_p), ptr.ctypes.data_as(C.c_void_p), nfold, a['resid'], a['pvar'],
                          fold.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p))
        assert np.all(fold == SENTINEL_ROW) and np.all(info == 7), 'a refused call wrote a host output'
        assert np.all(dev.download(out) == SENTINEL_ROW), 'a refused call wrote a device output'
        return rc

    overlap = idx.copy()
    overlap[200] = 10
    assert call(idx=overlap) == -13
    at_n = idx.copy()
    at_n[299] = N
    assert call(idx=at_n) == -13
    assert call(ptr=np.array([0, 150, 75, 225, 300], dtype=np.int64)) == -14
    assert call(nfold=0) == -15
    assert call(ptr=np.arange(4098, dtype=np.int64) % 2, nfold=4097) == -15
    # the arguments before the folds, numbered as in the signature (dt first of all, N between L and ldl)
    assert call(L=None) == -2 and call(N=0) == -3 and call(ldl=256) == -4 and call(W=None) == -5 and call(a=None) == -6
    assert call(dt=7) == -7 and call(Y=None) == -8 and call(ldy=383) == -9 and call(Kinv=None) == -10 and call(ldc=256) == -11
    assert call(alpha=None) == -12 and call(resid=None) == -16 and call(pvar=None) == -17
    assert lib.g3_gp_cv(None, p, N, Np, p, p, 0, p, Np, p, Np, p, None, None, 4, p, p, None, None) == -1


# ---------------------------------------------------------------------------------------------- other processes
def test_composite_kernel():
    """SE x COS + MAT32 at N = 385, 5 contiguous folds"""
    import g3py_amd as g3
    N = 385
    X, y = problem(N, seed=2)
    gp = g3.GaussianProcess(space=X[:2], location=g3.Zero(), kernel=g3.SE(X) * g3.COS(X) + g3.MAT32(X))
    gp.observed(X, y)
    f, r2 = np.array([0.11, 0.07]), np.array([0.7, 0.5])
    p = _params(gp, SE_var=1.1, SE_rate=RATE, COS_freq=f, MAT32_var=0.6, MAT32_rate=r2, Noise_var=0.1)    # (COS in a product: unit variance)
    spec = ('sum', ('prod', ('SE', 1.1, RATE, None), ('COS', 1.0, f, None)), ('MAT32', 0.6, r2, None))
    ref = closed_form(orc.GP(spec, 0.1), X, y, 5)
    _check64(gp.cv(p, 5, var=True), ref['loc'], ref['var'], ref['logpredictive'], ref['logpredictive_joint'], 'SE*COS+MAT32 N=385',
             np.abs(y).max())


def test_warped_gp_boxcox():
    """mean / variance by Gauss-Hermite on (loc, sd), median and both scores through the warping (its logdet_dinv of the
    held-out y is part of the joint score), N = 300, 4 folds"""
    import g3py_amd as g3
    N = 300
    X, y = problem(N, seed=3)
    y = np.abs(y) + 0.5                                        # inside BoxCox's domain
    gp = g3.WarpedGaussianProcess(space=X[:2], location=g3.Zero(), kernel=g3.SE(X), mapping=g3.BoxCoxLinear())
    gp.observed(X, y)
    p = _params(gp, SE_var=1.3, SE_rate=RATE, Noise_var=0.1, BoxCoxLinear_shift=1.0, BoxCoxLinear_scale=1.0, BoxCoxLinear_power=1.2)
    o = orc.GP(SE_SPEC, 0.1, ('Zero',), ('BoxCoxLinear', 1.0, 1.0, 1.2))
    ref = closed_form(o, X, y, 4)
    loc, sd = ref['loc'], np.sqrt(ref['var'])
    mean = o.gauss_hermite(lambda v: o.map(v), loc, sd)
    variance = o.gauss_hermite(lambda v: o.map(v) ** 2, loc, sd) - mean ** 2
    r = gp.cv(p, 4, var=True, median=True)
    assert list(r) == ['mean', 'variance', 'std', 'median', 'logpredictive', 'logpredictive_joint', 'folds', 'info']
    scale = max(1.0, np.abs(mean).max())
    lp, joint = ref['logpredictive'], ref['logpredictive_joint']
    print('cv warped: max err mean %.2e variance %.2e median %.2e logpredictive rel %.2e joint rel %.2e' % (
        np.abs(r.mean - mean).max(), np.abs(r.variance - variance).max(), np.abs(r.median - o.map(loc)).max(),
        abs(r.logpredictive / lp - 1), abs(r.logpredictive_joint / joint - 1)))
    assert np.all(r.info == 0)
    np.testing.assert_allclose(r.mean, mean, rtol=1e-8, atol=1e-8 * scale)
    np.testing.assert_allclose(r.variance, variance, rtol=1e-8, atol=1e-8 * scale ** 2)
    np.testing.assert_allclose(r.median, o.map(loc), rtol=1e-8, atol=1e-8 * scale)
    assert abs(r.logpredictive - lp) <= 1e-8 * abs(lp)
    assert abs(r.logpredictive_joint - joint) <= 1e-8 * abs(joint)


# ---------------------------------------------------------------------------------------------- fp32
@pytest.mark.parametrize('case', ['four_of_75', 'two_large'])
def test_fp32(case):
    """Per quantity within 10 x the float32 closed form's own error against the float64 closed form (printed).  Measured on
    an MI355X, device / NumPy's float32 closed form: folds 75 x 4 loc 1.6e-6 / 1.9e-6, variance 1.2e-6 / 3.7e-7, logpredictive
    4.7e-5 / 1.6e-5, joint 2.1e-5 / 3.7e-5; folds 257 + 343 loc 1.9e-6 / 2.6e-6, variance 2.7e-6 / 4.0e-7 (the tightest: 6.9 of
    the 10 x), logpredictive 3.0e-5 / 6.2e-5, joint 4.0e-5 / 2.1e-5 (profiles/cv.md)."""
    import g3py_amd as g3
    N, folds = CASES[case]
    X, y = problem(N, dtype=np.float32)
    gap, ref = fp32_gap(orc.GP(SE_SPEC, 0.1), X, y, folds)
    gp, p = _se_gp(g3, X, y, dtype=np.float32)
    r = gp.cv(p, folds, var=True)
    assert r.mean.dtype == np.float32 and np.all(r.info == 0)
    e = dict(loc=np.abs(r.mean.astype(np.float64) - ref['loc']).max(), var=np.abs(r.variance.astype(np.float64) - ref['var']).max(),
             logpredictive=abs(float(r.logpredictive) - float(ref['logpredictive'])),
             logpredictive_joint=abs(float(r.logpredictive_joint) - float(ref['logpredictive_joint'])))
    print('cv fp32 %s: ' % case + ', '.join('%s err %.3e (float32 closed form %.3e)' % (k, e[k], gap[k]) for k in e) + '; bound 10 x')
    for k in e:
        assert e[k] <= 10 * gap[k], (k, e[k], gap[k])


# ---------------------------------------------------------------------------------------------- cache and scores
def test_cv_after_logp_factors_nothing_and_is_kept_per_folds():
    """logp(p) then cv(p): no Gram launch and no second factorisation of K (the `gram` records are the gather launches, one per
    group; `potrf` records: the K^-1 sweep and the members' factorisation); the same folds again: no device work at all;
    other folds: computed again"""
    import g3py_amd as g3
    X, y, folds, ref = _reference('four_of_75')
    dev = g3.Device(0)
    try:
        gp, p = _se_gp(g3, X, y, device=dev)
        dev.prof_enable(True)
        dev.prof_reset()
        gp.logp(p)
        grams, prof = dev.gram_path_stats(), dev.prof_collect()
        r = gp.cv(p, 4, var=True)
        grams2, prof2 = dev.gram_path_stats(), dev.prof_collect()
        assert grams2 == grams                                     # no covariance was built
        assert prof2['gram']['count'] == prof['gram']['count'] + 1 and prof2['potrf']['count'] == prof['potrf']['count'] + 2
        again = gp.cv(p, 4, mean=False, std=False)
        prof3 = dev.prof_collect()
        assert all(prof3[k]['count'] == prof2[k]['count'] for k in prof2)
        assert again.logpredictive == r.logpredictive and again.logpredictive_joint == r.logpredictive_joint
        other = gp.cv(p, 5)
        assert dev.prof_collect()['gram']['count'] == prof2['gram']['count'] + 1 and len(other.folds) == 5
        _check64(r, ref['loc'], ref['var'], ref['logpredictive'], ref['logpredictive_joint'], 'after logp', np.abs(y).max())
        # a gradient in between shares the K^-1 workspaces
        g = gp.dlogp(p)
        assert gp.cv(p, 4).logpredictive == r.logpredictive and np.all(np.isfinite(g))
    finally:
        dev.close()


def test_scores_keys():
    import g3py_amd as g3
    X, y, folds, ref = _reference('four_of_75')
    gp, p = _se_gp(g3, X, y)
    gp.hidden = np.zeros(2)
    plain = gp.scores(p)
    assert list(plain) == ['_l1', '_l2']                       # exactly today's keys
    s = gp.scores(p, cv=4)
    assert list(s) == ['_l1', '_l2', '_cv_nlpd', '_cv_l1', '_cv_l2']
    lp, loc = ref['logpredictive'], ref['loc']
    assert s['_cv_nlpd'] == -gp.cv(p, 4).logpredictive / 300
    assert abs(s['_cv_nlpd'] + lp / 300) <= 1e-8 * abs(lp / 300)
    np.testing.assert_allclose(s['_cv_l1'], np.mean(np.abs(loc - y)), rtol=1e-8)
    np.testing.assert_allclose(s['_cv_l2'], np.mean((loc - y) ** 2), rtol=1e-8)
    assert plain['_l1'] == s['_l1'] and plain['_l2'] == s['_l2']
    both = gp.scores(p, loo=True, cv=_uncovered(300))
    assert list(both) == ['_l1', '_l2', '_loo_nlpd', '_loo_l1', '_loo_l2', '_cv_nlpd', '_cv_l1', '_cv_l2']
    un = _reference('uncovered')[3]
    assert abs(both['_cv_nlpd'] + un['logpredictive'] / 200) <= 1e-8 * abs(un['logpredictive'] / 200)
