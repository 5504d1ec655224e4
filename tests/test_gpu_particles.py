"""GPU tests of the chain draws: g3_potrf_robust_batched (the jitter schedule per member on the device), g3_gp_draws_batched
(_fields) and GaussianProcess.sample_chain / particles.
Tolerances: fp64 draws 1e-8 * max |draw| against the single sampler call of the same row and against the oracle (the
project's stated 1e-8 for mean and variance; eps * condition is about 6e-11 for the shapes used), fp32 a
plain 1e-4; a batched factor against the single call 1e-13 * |L| (fp64: the same wave programs) and 64 * eps32 * |L| (fp32)."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    import g3py_amd as g3
    return g3.Device.default()


def _params(gp, **nat):
    p = gp.params_test
    by = {v.name: v for v in gp.model.vars}
    for k, val in nat.items():
        v = by[gp.name + '_' + k]
        p[v.key] = (np.log(val) if v.positive else np.asarray(val, dtype=float)) * np.ones(v.shape)
    return p


# ----------------------------------------------------------------------------- 1. the batched robust factor
MEMBERS = ('spd', 'r1', 'r4', 'r6', 'r7', 'neg', 'nan')
EXPECT = dict(spd=(0, 0), r1=(1, 0), r4=(4, 0), r6=(6, 0), r7=(7, 0), neg=(20, 1))      # tries, fallback (the issue's table)


@functools.lru_cache(maxsize=None)
def _crafted(n):
    rng = np.random.default_rng(2024)
    B = rng.standard_normal((n, 6))
    R = B @ B.T
    m = np.diag(R).mean()
    A = rng.standard_normal((n, n))
    eye = np.eye(n)
    r7 = R.copy()
    r7[3, 3] = -0.5 * m
    bad = R + eye
    bad[2, 5] = bad[5, 2] = np.nan
    return dict(spd=A @ A.T / n + eye, r1=R - 1e-8 * m * eye, r4=R - 3e-4 * m * eye, r6=R - 3e-2 * m * eye, r7=r7, neg=-eye, nan=bad)


@functools.lru_cache(maxsize=None)
def _oracle_info(n):
    from oracle import g3_oracle as orc
    return {k: orc.cholesky_robust(v, return_info=True)[1:] for k, v in _crafted(n).items() if k != 'nan'}


_SINGLE = {}


def _single_factor(dev, n, name, dtype):
    """g3_potrf_robust on one crafted matrix: (L in its zeroed padded slot, tries, fallback, jitter), computed once"""
    key = (n, name, np.dtype(dtype).str)
    if key not in _SINGLE:
        from g3py_amd import _lib
        Np = _lib.roundup(n)
        Kd = dev.upload(_crafted(n)[name].astype(dtype))
        Ld = dev.alloc(Np, Np, dtype, zero=True)
        tr, fb, jt = dev.potrf_robust(Kd, Ld, n)
        _SINGLE[key] = (dev.download(Ld), tr, fb, jt)
        Kd.free()
        Ld.free()
    return _SINGLE[key]


def _run_batched(dev, n, names, dtype):
    from g3py_amd import _lib
    Np = _lib.roundup(n)
    Ks = np.concatenate([_crafted(n)[k].astype(dtype) for k in names])
    Kd = dev.upload(Ks)
    Ld = dev.alloc(len(names) * Np, Np, dtype)
    dev.copy_in(Ld, np.full((len(names) * Np, Np), 7.0, dtype=dtype))      # stale contents must not survive
    tries, fb, jit = dev.potrf_robust_batched(Kd, n * n, Ld, Np * Np, len(names), n)
    L = dev.download(Ld).reshape(len(names), Np, Np)
    np.testing.assert_array_equal(dev.download(Kd), Ks)                    # non-destructive
    Kd.free()
    Ld.free()
    return L, tries, fb, jit


def _check_members(dev, n, names, dtype, oracle=True):
    L, tries, fb, jit = _run_batched(dev, n, names, dtype)
    ltol = 1e-13 if np.dtype(dtype) == np.float64 else 64 * np.finfo(np.float32).eps
    for b, name in enumerate(names):
        Ls, tr, f, jt = _single_factor(dev, n, name, dtype)
        what = 'n=%d member %d (%s)' % (n, b, name)
        if oracle and name != 'nan':
            assert (tries[b], int(fb[b])) == tuple(int(v) for v in _oracle_info(n)[name]) == EXPECT[name], what
        assert (tries[b], bool(fb[b])) == (tr, f), (what, tries[b], fb[b], tr, f)
        assert jit[b] == jt, (what, jit[b], jt)
        assert np.linalg.norm(L[b] - Ls) <= ltol * np.linalg.norm(Ls), (what, np.linalg.norm(L[b] - Ls))
        assert not np.triu(L[b], 1).any() and not L[b][n:].any() and not L[b][:, n:].any(), what


@pytest.mark.parametrize('n', [7, 100, 128, 129, 200, 256])
def test_batched_robust_factor_on_crafted_matrices(dev, n):
    """every outcome of the schedule side by side in one call; batches of 1, 9 and 300 members (more members than CUs)"""
    _check_members(dev, n, MEMBERS, np.float64)
    rng = np.random.default_rng(n)
    for batch in (1, 9, 300):
        names = tuple(np.array(MEMBERS)[rng.permutation(np.arange(batch) % len(MEMBERS))])
        _check_members(dev, n, names, np.float64)


def test_batched_robust_factor_fp32(dev):
    """fp32: against the single call (the try counts of the table are the fp64 oracle's)"""
    names = tuple(np.array(MEMBERS)[np.random.default_rng(3).permutation(np.arange(20) % len(MEMBERS))])
    _check_members(dev, 200, names, np.float32, oracle=False)
    L, tries, fb, jit = _run_batched(dev, 200, ('spd', 'neg'), np.float32)
    assert (tries[0], fb[0], tries[1], fb[1]) == (0, False, 20, True)


def test_batched_robust_factor_loop_path(dev):
    """n = 300: beyond the one-workgroup kernel, the members take the single call inside the library"""
    _check_members(dev, 300, ('r4', 'spd', 'neg', 'r1', 'nan'), np.float64)


# ----------------------------------------------------------------------------- 2. rows against the loop and the oracle
def _mat52_problem(N, M, d, dtype=np.float64, rows=5, seed=0):
    import g3py_amd as g3
    rng = np.random.default_rng(1000 * N + M + seed)
    # points in [0, 3]^d: at rate 6 the oracle's posterior (and prior) covariance of the noise-free query points then has
    # min / max eigenvalue >= 8e-6 for every shape and row below (checked on the CPU), so the plain attempt passes everywhere
    X = rng.uniform(0, 3, (N, d)).astype(dtype)
    S = rng.uniform(0, 3, (M, d)).astype(dtype)
    y = (np.sin(2 * X.sum(1)) + 0.1 * rng.standard_normal(N)).astype(dtype)
    gp = g3.GaussianProcess(space=S, location=g3.Bias(), kernel=g3.MAT52(X), dtype=dtype)
    gp.observed(X, y)
    nat = [dict(MAT52_var=1.2 * (1 + 0.2 * u[0]), MAT52_rate=6.0 * (1 + 0.3 * u[1]) * np.ones(d), Noise_var=0.05 * (1 + 0.5 * u[2]),
                Bias_Bias=0.3 + 0.1 * u[3]) for u in rng.uniform(-1, 1, (rows, 4))]
    chain = np.stack([gp.active.dict_to_array(_params(gp, **p)) for p in nat])
    return rng, gp, X, y, S, nat, chain


def _loop(gp, chain, rand, **kw):
    return np.stack([gp.sampler(gp.active.array_to_dict(r), rand=rand[i], samples=rand.shape[2], **kw) for i, r in enumerate(chain)])


def _oracle_rows(nat, X, y, S, rand, prior, noise):
    from oracle import g3_oracle as orc
    out = []
    for i, p in enumerate(nat):
        o = orc.GP(('MAT52', p['MAT52_var'], p['MAT52_rate'], None), p['Noise_var'], mean=('Bias', p['Bias_Bias']))
        out.append(o.sampler(S, X, y, rand[i], prior=prior, noise=noise))
    return np.stack(out)


@pytest.mark.parametrize('N,M,d', [(40, 24, 2), (40, 150, 2), (200, 150, 3), (300, 24, 2)])
def test_rows_equal_the_loop_and_the_oracle(N, M, d):
    """Np = 128, 256 and 384 (the solve that spills V), Mp = 128 and 256; blocks of 2 + 2 + 1 rows and one block"""
    rng, gp, X, y, S, nat, chain = _mat52_problem(N, M, d)
    for samples in (1, 3):
        rand = rng.standard_normal((len(chain), M, samples))
        for noise in (False, True):
            for prior in (False, True):
                got, info = gp.sample_chain(chain, samples=samples, noise=noise, prior=prior, rand=rand, batch=2, return_info=True)
                want = _loop(gp, chain, rand, noise=noise, prior=prior)
                ref = _oracle_rows(nat, X, y, S, rand, prior, noise)
                tol = 1e-8 * np.abs(ref).max()
                print('sample_chain N=%d M=%d S=%d noise=%d prior=%d: |batched - loop| %.2e |batched - oracle| %.2e (bound %.1e) '
                      'tries %s' % (N, M, samples, noise, prior, np.abs(got - want).max(), np.abs(got - ref).max(), tol, info['tries']))
                assert got.shape == (len(chain), M, samples) and got.dtype == np.float64
                assert not info['tries'].any() and not info['fallback'].any()
                np.testing.assert_allclose(got, want, rtol=0, atol=tol)
                np.testing.assert_allclose(got, ref, rtol=0, atol=tol)
    one = gp.sample_chain(chain, samples=3, noise=True, rand=rand)                            # one block, default batch
    np.testing.assert_allclose(one, _loop(gp, chain, rand, noise=True), rtol=0, atol=tol)


def test_fp32_rows_with_noise():
    rng, gp, X, y, S, nat, chain = _mat52_problem(200, 150, 3, dtype=np.float32)
    rand = rng.standard_normal((len(chain), 150, 2)).astype(np.float32)
    got = gp.sample_chain(chain, samples=2, noise=True, rand=rand, batch=3)
    want = _loop(gp, chain, rand, noise=True)
    print('sample_chain fp32: |batched - loop| %.2e' % np.abs(got - want).max())
    assert got.dtype == np.float32
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-4)


# ----------------------------------------------------------------------------- 3. a posterior covariance singular to rounding
def test_near_singular_posterior_through_the_device_call(dev):
    """SE, rate 2, dense noise-free query points: min / max eigenvalue about -1.6e-15.  Whether the plain attempt passes is
    luck, so the try counts are not compared between paths: the schedule's own invariants are checked per row"""
    import g3py_amd as g3
    from g3py_amd import _lib
    rng = np.random.default_rng(11)
    N, M, d, B = 40, 150, 2, 4
    X, S = rng.uniform(0, 1, (N, d)), rng.uniform(0, 1, (M, d))
    y = np.sin(4 * X.sum(1)) + 0.1 * rng.standard_normal(N)
    gp = g3.GaussianProcess(space=S, location=g3.Bias(), kernel=g3.SE(X), device=dev)
    gp.observed(X, y)
    chain = np.stack([gp.active.dict_to_array(_params(gp, SE_var=1.0 + 0.1 * i, SE_rate=2.0 * np.ones(d), Noise_var=0.05,
                                                      Bias_Bias=0.1)) for i in range(B)])
    Np, Mp = _lib.roundup(N), _lib.roundup(M)
    kstride = (Np + _lib.G3_RHS_PAD) * Np
    _, (tmpl, offs, fields), loc, obs, delta = gp._chain_block_members(chain, gp.f_kernel, gp._x(S), gp._x(X), y, False)
    ws = gp._chain_workspace(B, Np, False)
    Sd, Xd = dev.upload(gp._x(S)), dev.upload(gp._x(X))
    gp._chain_factor_block(obs, delta, Xd, N, d, ws['K'], kstride, ws['W'], ws['a'])
    Cd, Ld = dev.alloc(B * Mp, Mp, np.float64), dev.alloc(B * Mp, Mp, np.float64)
    Z = rng.standard_normal((B, M, 2))
    out, tries, fb, jit = dev.gp_draws_batched_fields(tmpl, offs, fields, Sd, M, Xd, N, d, ws['K'], kstride, ws['W'], ws['a'], False,
                                                     loc, Z, Cm=Cd, Lp=Ld)
    Cs, Ls = dev.download(Cd).reshape(B, Mp, Mp), dev.download(Ld).reshape(B, Mp, Mp)
    print('near-singular posterior: tries %s jitter %s' % (tries, jit))
    assert np.isfinite(out).all() and not fb.any()
    for b in range(B):
        Cl = np.tril(Cs[b][:M, :M])
        Cm = Cl + np.tril(Cl, -1).T
        dg = np.diag(Cm)
        if tries[b] == 0:
            assert jit[b] == 0.0
        else:
            lift = dg.mean() * float(np.float32(1e-6)) - dg.min() if dg.min() <= 0 else 0.0
            dK = dg.mean() * float(np.float32(1e-6))
            for _ in range(int(tries[b]) - 1):
                dK *= float(np.float32(10))
            assert abs(jit[b] - (lift + dK)) <= 1e-12 * (lift + dK), (b, jit[b], lift + dK)
        Lp = Ls[b][:M, :M]
        assert not np.triu(Ls[b], 1).any() and not Ls[b][M:].any() and not Ls[b][:, M:].any()
        err = np.linalg.norm(Lp @ Lp.T - (Cm + jit[b] * np.eye(M)))
        assert err <= 1e-12 * np.linalg.norm(Cm), (b, err, np.linalg.norm(Cm))
    # the public method on the same chain: finite draws, no fallback
    got, info = gp.sample_chain(chain, samples=2, rand=Z, return_info=True)
    assert np.isfinite(got).all() and not info['fallback'].any()


# ----------------------------------------------------------------------------- 4. particles
def test_particles_equals_the_concatenated_loop_of_samples():
    rng, gp, X, y, S, nat, chain = _mat52_problem(40, 24, 2, seed=4)
    R, M = len(chain), 24
    for samples in (1, 2):
        np.random.seed(17)
        got = gp.particles(chain, samples=samples)
        np.random.seed(17)
        want = np.concatenate([gp.sample(gp.active.array_to_dict(r), samples=samples) for r in chain], axis=1)
        assert got.shape == (M, R * samples)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-8 * np.abs(want).max())
    np.random.seed(18)
    got = gp.particles(chain, R + 2, noise=True)                                       # cycles over the rows
    np.random.seed(18)
    want = np.concatenate([gp.sample(gp.active.array_to_dict(chain[i % R]), noise=True) for i in range(R + 2)], axis=1)
    assert got.shape == (M, R + 2)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-8 * np.abs(want).max())


# ----------------------------------------------------------------------------- 5. edge members
def test_edge_members():
    import g3py_amd as g3
    from g3py_amd import _lib
    rng = np.random.default_rng(21)
    N = 60
    X = np.repeat(rng.uniform(0, 6, (N // 2, 1)), 2, axis=0)          # every input twice: singular without noise
    y = np.sin(X[:, 0]) + 0.5
    S = np.linspace(-1, 7, 7)[:, None]
    M = len(S)
    gp = g3.GaussianProcess(space=S, location=g3.Bias(), kernel=g3.SE(X))
    gp.observed(X, y)
    rows = []
    for noise in (0.1, 0.0, 0.05):
        p = _params(gp, SE_var=1.0, SE_rate=[1.0], Noise_var=max(noise, 1e-300), Bias_Bias=0.2)
        if noise == 0.0:
            p['GP_Noise_var_log_'] = np.asarray(-800.0)                # exp underflows: no noise, the first factorisation fails
        rows.append(gp.active.dict_to_array(p))
    chain = np.stack(rows)
    # the middle row's observation covariance needs the jitter schedule, its neighbours do not
    Np = _lib.roundup(N)
    kstride = (Np + _lib.G3_RHS_PAD) * Np
    _, _, _, obs, delta = gp._chain_block_members(chain, gp.f_kernel, gp._x(S), gp._x(X), y, False)
    ws = gp._chain_workspace(3, Np, False)
    Xd = gp.device.upload(gp._x(X))
    st = gp._chain_factor_block(obs, delta, Xd, N, 1, ws['K'], kstride, ws['W'], ws['a'])
    assert st[1, 3] > 0 and st[0, 3] == 0 and st[2, 3] == 0, st[:, 3:]
    rand = rng.standard_normal((3, M, 2))
    got = gp.sample_chain(chain, samples=2, noise=True, rand=rand)
    want = _loop(gp, chain, rand, noise=True)
    for i in range(3):
        print('edge members: row %d |batched - single| %.2e' % (i, np.abs(got[i] - want[i]).max()))
        np.testing.assert_allclose(got[i], want[i], rtol=0, atol=1e-8 * np.abs(want[i]).max(), err_msg='row %d' % i)
    # the neighbours are what they are without the jittered row between them
    alone = gp.sample_chain(chain[[0, 2]], samples=2, noise=True, rand=rand[[0, 2]])
    np.testing.assert_allclose(got[[0, 2]], alone, rtol=0, atol=1e-8 * np.abs(alone).max())
    # a chain of one row; M = 1; M = 129 (two row blocks of the padded factor)
    rng, gp, X, y, S, nat, chain = _mat52_problem(40, 129, 2, seed=5)
    for M in (1, 24, 129):
        rand = rng.standard_normal((1, M, 3))
        got = gp.sample_chain(chain[:1], space=S[:M], samples=3, noise=True, rand=rand)
        want = gp.sampler(gp.active.array_to_dict(chain[0]), space=S[:M], samples=3, noise=True, rand=rand[0])
        assert got.shape == (1, M, 3)
        np.testing.assert_allclose(got[0], want, rtol=0, atol=1e-8 * np.abs(want).max(), err_msg='M=%d' % M)
    rand = rng.standard_normal((3, 129, 1))
    got = gp.sample_chain(chain[:3], noise=True, rand=rand)
    want = _loop(gp, chain[:3], rand, noise=True)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-8 * np.abs(want).max())


@pytest.mark.parametrize('N,M', [(40, 300), (1100, 24)])
def test_members_beyond_the_one_launch_kernels(N, M):
    """M = 300: more than 256 query points, the robust factor of every member is the single call inside the library, working
    in the head of the workspace that also holds V, C and Lp; N = 1100: beyond the one-launch solve, V comes from the
    single-member cross path per member.  2 rows (and a block of 1) against the loop of sampler calls"""
    rng, gp, X, y, S, nat, chain = _mat52_problem(N, M, 2, rows=2)
    rand = rng.standard_normal((2, M, 2))
    for batch in (None, 1):
        got, info = gp.sample_chain(chain, samples=2, noise=True, rand=rand, batch=batch, return_info=True)
        want = _loop(gp, chain, rand, noise=True)
        print('sample_chain N=%d M=%d batch=%s: |batched - loop| %.2e tries %s' % (N, M, batch, np.abs(got - want).max(), info['tries']))
        assert not info['tries'].any() and not info['fallback'].any()
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-8 * np.abs(want).max())
    got = gp.sample_chain(chain, samples=2, noise=True, prior=True, rand=rand)
    np.testing.assert_allclose(got, _loop(gp, chain, rand, noise=True, prior=True), rtol=0, atol=1e-8 * np.abs(want).max())


# ----------------------------------------------------------------------------- 6. repeatability
def test_two_calls_give_the_same_bits():
    import g3py_amd as g3
    rng = np.random.default_rng(31)
    N = M = 128
    X, S = rng.uniform(0, 3, (N, 2)), rng.uniform(0, 3, (M, 2))
    y = np.sin(X.sum(1)) + 0.1 * rng.standard_normal(N)
    gp = g3.GaussianProcess(space=S, location=g3.Bias(), kernel=g3.SE(X))
    gp.observed(X, y)
    a0 = gp.active.dict_to_array(_params(gp, SE_var=1.2, SE_rate=[0.8, 1.1], Noise_var=0.1, Bias_Bias=0.1))
    chain = a0 + 0.1 * rng.standard_normal((300, len(a0)))
    rand = rng.standard_normal((300, M, 1))
    first, i1 = gp.sample_chain(chain, rand=rand, return_info=True)
    second, i2 = gp.sample_chain(chain, rand=rand, return_info=True)
    np.testing.assert_array_equal(first, second)
    for k in ('tries', 'fallback', 'jitter'):
        np.testing.assert_array_equal(i1[k], i2[k])
    assert np.isfinite(first).all()


# ----------------------------------------------------------------------------- 7. the ABI's return codes
def test_bad_arguments_return_the_documented_codes(dev):
    import g3py_amd as g3
    from g3py_amd import _lib
    from g3py_amd.device import compile_spec
    rng = np.random.default_rng(41)
    N, M, d, B = 100, 30, 2, 3

    def setup(kernel):
        X, S = rng.uniform(0, 1, (N, d)), rng.uniform(0, 1, (M, d))
        y = np.sin(4 * X.sum(1)) + 0.1 * rng.standard_normal(N)
        gp = g3.GaussianProcess(space=S, location=g3.Bias(), kernel=kernel(g3, X), device=dev)
        gp.observed(X, y)
        a0 = gp.active.dict_to_array(gp.params_default)
        chain = a0 + 0.05 * rng.standard_normal((B, len(a0)))
        Np = _lib.roundup(N)
        kstride = (Np + _lib.G3_RHS_PAD) * Np
        vb, members, loc, obs, delta = gp._chain_block_members(chain, gp.f_kernel_noise, gp._x(S), gp._x(X), y, False)
        ws = gp._chain_workspace(B, Np, False)
        Sd, Xd = dev.upload(gp._x(S)), dev.upload(gp._x(X))
        gp._chain_factor_block(obs, delta, Xd, N, d, ws['K'], kstride, ws['W'], ws['a'])
        progs = [compile_spec(gp.f_kernel_noise.spec(gp._values_row(vb, j), d), d) for j in range(B)]
        return gp, ws, Sd, Xd, Np, kstride, members, loc, progs
    gp, ws, Sd, Xd, Np, kstride, (tmpl, offs, fields), loc, progs = setup(lambda g3, X: g3.SE(X))
    lib, ctx = dev.lib, dev.ctx
    arr = (_lib.KernelProg * B)(*progs)
    loc = np.ascontiguousarray(loc)
    Z = rng.standard_normal((B, M, 1))
    out = np.empty((B, M, 1))
    good = dict(progs=arr, batch=B, Xs=Sd.ptr, M=M, ldxs=d, X=Xd.ptr, N=N, ldx=d, d=d, L=ws['K'].ptr, ldl=Np, kstride=kstride,
                invd=ws['W'].ptr, a=ws['a'].ptr, dt=0, lift=1, loc=loc.ctypes.data, Z=Z.ctypes.data, S=1, out=out.ctypes.data,
                C=None, Lp=None, maxtries=20, tries=None, fallback=None, jitter=None)
    order = list(good)

    def call(**over):
        v = dict(good, **over)
        return lib.g3_gp_draws_batched(ctx, *[v[k] for k in order])
    assert call() == 0 and np.isfinite(out).all()
    other = (_lib.KernelProg * B)(*progs)
    other[2].leaf[0].kind = _lib.KINDS['OU']                 # another structure
    for over, code in [(dict(progs=None), -2), (dict(progs=other), -2), (dict(batch=0), -3), (dict(batch=_lib.G3_MAX_BATCH + 1), -3),
                       (dict(Xs=None), -4), (dict(M=0), -5), (dict(ldxs=1), -6), (dict(X=None), -7), (dict(N=0), -8),
                       (dict(ldx=1), -9), (dict(d=0), -10), (dict(ldl=Np - 2), -12), (dict(ldl=Np + 1), -12),
                       (dict(kstride=Np * Np - 2), -13), (dict(invd=None), -14), (dict(a=None), -15), (dict(dt=7), -16),
                       (dict(loc=None), -18), (dict(Z=None), -19), (dict(S=0), -20), (dict(out=None), -21), (dict(maxtries=-1), -24)]:
        assert call(**over) == code, (over, call(**over), code)
    assert call(L=None, X=None, N=0, invd=None, a=None) == 0             # the prior needs no factorisation
    assert lib.g3_gp_draws_batched(None, *[good[k] for k in order]) == -1
    # the template form: its own first six arguments, then the same list three places further
    f = np.ascontiguousarray(fields)
    o = np.ascontiguousarray(offs, dtype=np.int32)
    tail = [good[k] for k in order[2:]]

    def callf(tm=C.byref(tmpl), batch=B, fields=f.ctypes.data, offs=o.ctypes.data, nf=len(o), tail=tail):
        return lib.g3_gp_draws_batched_fields(ctx, tm, batch, fields, offs, nf, *tail)
    assert call() == 0
    first = out.copy()
    out[:] = 0
    assert callf() == 0
    np.testing.assert_array_equal(out, first)                # the two forms hand the launches the same programs
    assert callf(tm=None) == -2 and callf(batch=_lib.G3_MAX_BATCH + 1) == -3 and callf(fields=None) == -4 and callf(nf=10 ** 6) == -6
    v = dict(good, ldl=Np + 1)
    assert callf(tail=[v[k] for k in order[2:]]) == -15
    # the exponent of a POL leaf is structure: its offset is refused, as in the cross call
    gp2, ws2, Sd2, Xd2, _, _, (tm2, offs2, fields2), loc2, _ = setup(lambda g3, X: g3.POL(X, 3) + g3.SE(X))
    pol = [i for i in range(tm2.nleaf) if tm2.leaf[i].kind == _lib.KINDS['DOT']][0]
    o3 = np.ascontiguousarray(offs2, dtype=np.int32).copy()
    o3[0] = _lib.KernelProg.leaf.offset + pol * C.sizeof(_lib.Leaf) + _lib.Leaf.freq.offset
    with pytest.raises(g3.G3Error, match='status -5'):
        dev.gp_draws_batched_fields(tm2, o3, fields2, Sd2, M, Xd2, N, d, ws2['K'], kstride, ws2['W'], ws2['a'], True, loc2, Z)
    # the batched robust factor
    Kd, Ld = dev.upload(np.eye(8)), dev.alloc(128, 128, np.float64)
    rb = lambda **kw: lib.g3_potrf_robust_batched(*[dict(dict(ctx=ctx, K=Kd.ptr, ldk=8, kstride=64, L=Ld.ptr, ldl=128, lstride=128 * 128,
                                                              batch=1, n=8, dt=0, maxtries=20, t=None, f=None, j=None), **kw)[k]
                                                    for k in ('ctx', 'K', 'ldk', 'kstride', 'L', 'ldl', 'lstride', 'batch', 'n', 'dt',
                                                              'maxtries', 't', 'f', 'j')])
    assert rb() == 0
    for over, code in [(dict(ctx=None), -1), (dict(K=None), -2), (dict(ldk=7), -3), (dict(kstride=63), -4), (dict(L=None), -5),
                       (dict(ldl=127), -6), (dict(lstride=128 * 127), -7), (dict(batch=0), -8), (dict(batch=_lib.G3_MAX_BATCH + 1), -8),
                       (dict(n=-1), -9), (dict(dt=5), -10), (dict(maxtries=-1), -11)]:
        assert rb(**over) == code, (over, rb(**over), code)
