"""Dot-product kernel family on the device (LIN, POL, NN, BW, VAR, NIL -- g3py/processes/hypers/kernels.py:82-94,
293-357): Gram parity, generated = interpreted, the varying diagonal, gradient sums, the process API, chains, Student-t and
the multi-GPU driver at world 1.  The reference arithmetic is tests/dot_reference.py (the oracle does not know these
leaves); mixed trees go through the oracle with its `kernel_cov` / `kernel_cov_grads` globals patched."""
import ctypes as C

import numpy as np
import pytest

from dot_reference import dot_zoo, kernel_cov_ext, kernel_cov_grads_ext, zoo_inputs

pytestmark = pytest.mark.gpu

# the tolerances of tests/test_gpu_gram.py for the same comparison
F64 = dict(rtol=1e-12, atol=1e-13)
F32 = dict(rtol=3e-4, atol=3e-5)


def _tol(base, ref):
    return dict(rtol=base['rtol'], atol=base['atol'] * max(1.0, np.abs(ref).max()))


def _gram(dev, spec, X1, X2=None, dtype=np.float64, flags=0, pad=None):
    from g3py_amd.device import compile_spec
    X1 = np.asarray(X1, dtype=dtype)
    d = X1.shape[1]
    prog = compile_spec(spec, d)
    A = dev.upload(X1)
    B = dev.upload(np.asarray(X2, dtype=dtype)) if X2 is not None else None
    n1 = X1.shape[0]
    n2 = n1 if X2 is None else len(X2)
    p1, p2 = (pad or n1), (pad or n2) if X2 is None else n2
    out = dev.alloc(p1, p2, dtype, zero=True)
    dev.gram(prog, A, B, d, out, p1, p2, flags)
    return dev.download(out)


def _params(gp, **nat):
    p = gp.params_test
    by = {v.name: v for v in gp.model.vars}
    for k, val in nat.items():
        v = by[gp.name + '_' + k]
        p[v.key] = (np.log(val) if v.positive else np.asarray(val, dtype=float)) * np.ones(v.shape)
    return p


@pytest.fixture(scope='module')
def dev():
    import g3py_amd as g3
    return g3.Device.default()


@pytest.fixture
def patched_oracle(monkeypatch):
    from oracle import g3_oracle as orc
    monkeypatch.setattr(orc, 'kernel_cov', kernel_cov_ext)
    monkeypatch.setattr(orc, 'kernel_cov_grads', kernel_cov_grads_ext)
    return orc


# ------------------------------------------------------------------ 1. Gram parity
@pytest.mark.parametrize('d', [1, 3, 8])
def test_gram_matches_reference_square_and_cross(dev, d):
    for name, spec in dot_zoo(d).items():
        X, Xs = zoo_inputs(spec, 129, d, 10 + d), zoo_inputs(spec, 70, d, 20 + d)
        ref = kernel_cov_ext(spec, X)
        np.testing.assert_allclose(_gram(dev, spec, X), ref, err_msg=name, **_tol(F64, ref))
        ref = kernel_cov_ext(spec, Xs, X)
        np.testing.assert_allclose(_gram(dev, spec, Xs, X), ref, err_msg=name + ' cross', **_tol(F64, ref))


@pytest.mark.parametrize('name', ['LIN', 'POL4', 'POL*SE', 'NN', 'BW[dims]+VAR'])
def test_gram_fp32(dev, name):
    """fp32 at the tolerances of the stationary kernels: p <= 4 multiplications cost p eps relative; the cancellation in
    bias + sum for inputs of both signs is an absolute error of eps * sum|terms| <= eps * d * max|term|, covered by the atol
    term scaled with |ref|max"""
    d = 3
    spec = dot_zoo(d)[name]
    X = zoo_inputs(spec, 150, d, 31)
    ref = kernel_cov_ext(spec, X)
    np.testing.assert_allclose(_gram(dev, spec, X, dtype=np.float32), ref, **_tol(F32, ref))


@pytest.mark.parametrize('n', [1, 63, 64, 65, 129, 300])
def test_gram_ragged_sizes_lower_and_padding(dev, n):
    """padding rows / columns are exactly 0 / the identity even with a VAR term, a bias and a shift: the store loop never
    evaluates the program outside n x n"""
    import g3py_amd._lib as lib
    d = 3
    zoo = dot_zoo(d)
    for name in ('LIN+SE', '2*NN+0.1', 'BW[dims]+VAR', 'POL*SE', 'LIN[dims]+SE+noise'):
        spec = zoo[name]
        X = zoo_inputs(spec, n, d, n)
        ref = kernel_cov_ext(spec, X)
        pad = lib.roundup(n)
        K = _gram(dev, spec, X, flags=lib.G3_GRAM_PAD_EYE | lib.G3_GRAM_SCRUB, pad=pad)
        np.testing.assert_allclose(K[:n, :n], ref, err_msg=name, **_tol(F64, ref))
        np.testing.assert_array_equal(K[n:, n:], np.eye(pad - n))
        assert not K[:n, n:].any() and not K[n:, :n].any(), name
        K0 = _gram(dev, spec, X, flags=0, pad=pad)
        assert not K0[n:, :].any() and not K0[:, n:].any(), name
        Kl = _gram(dev, spec, X, flags=lib.G3_GRAM_LOWER, pad=pad)
        np.testing.assert_allclose(np.tril(Kl[:n, :n]), np.tril(ref), err_msg=name, **_tol(F64, ref))
        assert not Kl[n:, :].any() and not Kl[:, n:].any(), name


def test_batched_gram_pads_every_member_with_the_identity(dev):
    """the chain path's Gram launch (member in grid.z) through g3_gp_factor_batched: each member's padded covariance is
    factored, so a non-zero padding entry would show as a wrong log-determinant"""
    import g3py_amd._lib as lib
    from g3py_amd.device import compile_spec
    from oracle import g3_oracle as orc
    N, d, B = 200, 3, 3
    zoo = dot_zoo(d)
    X = zoo_inputs(zoo['LIN'], N, d, 5)
    progs, want = [], []
    for b in range(B):
        spec = ('sum', ('sum', ('DOT', 1.0, np.array([0.5, 0.8, 1.1]) + 0.1 * b, 0.3 + b, 1, None), ('VAR', 0.2 * (b + 1))),
                ('NOISE', 0.1))
        progs.append(compile_spec(spec, d))
        want.append(np.sum(np.log(np.diag(orc.cholesky_robust(kernel_cov_ext(spec, X))))))
    Np = lib.roundup(N)
    K = dev.alloc(B * (Np + 128), Np, np.float64)
    st = dev.gp_factor_batched(progs, dev.upload(X), N, d, dev.upload(np.zeros((B, N))), K, (Np + 128) * Np,
                               dev.alloc(B * Np, 128, np.float64), dev.alloc(B, Np, np.float64), raw=True)
    np.testing.assert_allclose(st[:, 0], want, rtol=1e-10)
    assert not st[:, 3].any() and not st[:, 5].any()


# ------------------------------------------------------------------ 2. generated = interpreted
def test_generated_equals_interpreted_and_nothing_is_interpreted(monkeypatch):
    import g3py_amd as g3
    dev1 = g3.Device(0)
    monkeypatch.setenv('G3_GRAM_JIT', '0')
    monkeypatch.setenv('G3_GRAM_NOFAST', '1')
    dev0 = g3.Device(0)                      # this context interprets everything
    for d in (1, 3, 8):
        for name, spec in dot_zoo(d).items():
            X, Xs = zoo_inputs(spec, 190, d, 40 + d), zoo_inputs(spec, 66, d, 50 + d)
            a, b = _gram(dev1, spec, X), _gram(dev0, spec, X)
            np.testing.assert_allclose(a, b, rtol=1e-13, atol=1e-14 * max(1.0, np.abs(b).max()), err_msg='%s d=%d' % (name, d))
            a, b = _gram(dev1, spec, Xs, X), _gram(dev0, spec, Xs, X)
            np.testing.assert_allclose(a, b, rtol=1e-13, atol=1e-14 * max(1.0, np.abs(b).max()), err_msg='%s d=%d cross' % (name, d))
            ref = kernel_cov_ext(spec, Xs, X)
            np.testing.assert_allclose(b, ref, err_msg=name + ' interpreted', **_tol(F64, ref))
    s1, s0 = dev1.gram_path_stats(), dev0.gram_path_stats()
    assert s1['interpreted'] == 0 and s1['table'] == 0 and s1['generated'] > 0, s1      # the table never matches a dot leaf
    assert s0['generated'] == 0 and s0['table'] == 0 and s0['interpreted'] > 0, s0
    dev0.close()
    dev1.close()


# ------------------------------------------------------------------ 3. the diagonal varies; row blocks
def test_gram_diag_and_row_blocks(dev):
    import g3py_amd._lib as lib
    from g3py_amd.device import compile_spec
    N, d = 300, 3
    zoo = dot_zoo(d)
    rng = np.random.default_rng(3)
    for name in ('LIN', 'POL3', 'NN', 'BW', 'LIN[dims]+SE+noise'):
        spec = zoo[name]
        X = zoo_inputs(spec, N, d, 60) * np.exp(rng.uniform(-3, 3, (N, 1)))      # points at very different distances
        ref = kernel_cov_ext(spec, X)
        dg = np.diag(ref)
        if name != 'NN':
            assert dg.max() > 1e3 * dg.min() > 0
        prog = compile_spec(spec, d)
        Xd = dev.upload(X)
        out = dev.alloc(1, N, np.float64)
        dev.gram_diag(prog, Xd, d, out)
        np.testing.assert_allclose(dev.download(out)[0], dg, rtol=1e-12, err_msg=name)
        for row0 in (0, 128, 256):
            nrows = 128
            blk = dev.alloc(nrows, row0 + nrows, np.float64, zero=True)
            rc = dev.lib.g3_gram_rows(dev.ctx, C.byref(prog), Xd.ptr, N, Xd.ld, d, row0, nrows, lib.G3_F64, blk.ptr, blk.ld,
                                      lib.G3_GRAM_PAD_EYE)
            assert rc == 0
            got = dev.download(blk)
            r1 = min(N, row0 + nrows)
            np.testing.assert_allclose(got[:r1 - row0, :r1], ref[row0:r1, :r1], err_msg='%s row0=%d' % (name, row0), **_tol(F64, ref))
            want_pad = np.zeros((nrows, row0 + nrows))
            want_pad[np.arange(nrows), row0 + np.arange(nrows)] = 1.0
            np.testing.assert_array_equal(got[r1 - row0:, :], want_pad[r1 - row0:, :])
            np.testing.assert_array_equal(got[:r1 - row0, r1:], 0.0)


# ------------------------------------------------------------------ 4. gradient sums
def test_gram_grad_matches_reference_generated_interpreted_and_rows(monkeypatch):
    """g3_gram_grad: 1/2 sum_ij (alpha_i alpha_j - Kinv_ij) dK_ij/dtheta against the analytic dK/dtheta of the reference, at
    the tolerance of test_gram_grad_matches_oracle (1e-10 of the absolute sum), from the generated kernel and from the
    interpreter (G3_GRAD_GENERIC=1); g3_gram_grad_rows over disjoint row ranges adds up to it"""
    import g3py_amd as g3
    from g3py_amd.device import compile_spec
    dev1 = g3.Device(0)
    monkeypatch.setenv('G3_GRAD_GENERIC', '1')
    dev0 = g3.Device(0)
    N, d = 150, 3
    rng = np.random.default_rng(5)
    A = rng.standard_normal((N, N))
    G = (A + A.T) / 2
    alpha = rng.standard_normal(N)
    Gfull = np.outer(alpha, alpha) - G
    for name, spec in dot_zoo(d).items():
        X = zoo_inputs(spec, N, d, 70)
        _, grads = kernel_cov_grads_ext(spec, X)
        prog = compile_spec(spec, d)
        for dv in (dev1, dev0):
            gmap = dv.grad_layout(prog)
            Xd, Gd, ad = dv.upload(X), dv.upload(np.tril(G)), dv.upload(alpha)
            out = dv.gram_grad(prog, gmap, Xd, N, d, Gd, ad)
            assert len(out) == len(grads)
            for (leaf, pname, k, dK) in grads:
                slot = getattr(gmap, pname)[leaf] + (0 if k is None else k)
                want = 0.5 * np.sum(Gfull * dK)
                scale = 0.5 * np.sum(np.abs(Gfull * dK)) + 1e-30
                assert abs(out[slot] - want) < 1e-10 * scale, (name, dv is dev1, leaf, pname, k, out[slot], want)
            tot = np.zeros(gmap.nslots)
            for r0, nr in ((0, 64), (64, 64), (128, N - 128)):
                tot += dv.gram_grad_rows(prog, gmap, Xd, N, d, r0, nr, dv.upload(np.ascontiguousarray(np.tril(G)[r0:r0 + nr])), ad)
            np.testing.assert_allclose(tot, out, rtol=1e-12, atol=1e-12 * np.abs(out).max(), err_msg=name)
    s1, s0 = dev1.grad_path_stats(), dev0.grad_path_stats()
    assert s1['interpreted'] == 0 and s1['generated'] > 0, s1
    assert s0['generated'] == 0 and s0['table'] == 0 and s0['interpreted'] > 0, s0
    dev0.close()
    dev1.close()


def test_chain_fields_refuse_the_exponent_of_a_dot_leaf(dev):
    """p is structure: the *_fields entry points refuse an offset that names freq[0] of a DOT leaf of the template (-5, as
    for any bad offset) and still accept the same offset on a periodic leaf's freq[0]"""
    import g3py_amd._lib as lib
    from g3py_amd.device import compile_spec
    N, d, B = 64, 2, 2
    X = np.random.default_rng(0).standard_normal((N, d))
    Np = lib.roundup(N)
    K = dev.alloc(B * (Np + 128), Np, np.float64)
    W, a = dev.alloc(B * Np, 128, np.float64), dev.alloc(B, Np, np.float64)
    Xd, dl = dev.upload(X), dev.upload(np.zeros((B, N)))
    off_p = lib.KernelProg.leaf.offset + lib.Leaf.freq.offset
    tmpl = compile_spec(('sum', ('DOT', 1.0, np.ones(d), 0.5, 2, None), ('NOISE', 0.1)), d)
    with pytest.raises(lib.G3Error, match='status -5'):
        dev.gp_factor_batched_fields(tmpl, [off_p], np.full((B, 1), 3.0), Xd, N, d, dl, K, (Np + 128) * Np, W, a)
    ok = dev.gp_factor_batched_fields(tmpl, [lib.KernelProg.leaf.offset + lib.Leaf.alpha.offset], np.array([[0.5], [0.7]]),
                                      Xd, N, d, dl, K, (Np + 128) * Np, W, a)
    assert ok.shape == (B, 6) and ok[0, 0] != ok[1, 0]
    tmpl = compile_spec(('sum', ('COS', 1.0, np.full(d, 0.2), None), ('NOISE', 0.1)), d)
    ok = dev.gp_factor_batched_fields(tmpl, [off_p], np.array([[0.2], [0.3]]), Xd, N, d, dl, K, (Np + 128) * Np, W, a)
    assert ok.shape == (B, 6)
    # the gradient's entry point applies the same rule before any device work
    tmpl = compile_spec(('sum', ('DOT', 1.0, np.ones(d), 0.5, 2, None), ('NOISE', 0.1)), d)
    Y, Ki, al = dev.alloc(B * (Np + 128), Np, np.float64), dev.alloc(B * (Np + 128), Np, np.float64), dev.alloc(B, Np, np.float64)
    with pytest.raises(lib.G3Error, match='status -5'):
        dev.gp_dlogp_batched_fields(tmpl, [off_p], np.full((B, 1), 3.0), dev.grad_layout(tmpl), Xd, N, d, K, (Np + 128) * Np, W, a,
                                    Y, Ki, al)


def test_batch_members_with_different_exponents_do_not_share_a_kernel(dev):
    """p is structure on the programs route too: g3_gp_factor_batched refuses members that differ in the exponent of a dot
    leaf (-2, as for any other structure mismatch -- one generated Gram kernel serves the whole batch), and
    g3_gp_dlogp_batched gives every such member its own exponent (no generated kernel is shared: the sums are interpreted
    per member) -- equal to the one-at-a-time gradient sums"""
    import g3py_amd._lib as lib
    from g3py_amd.device import compile_spec
    N, d, B = 100, 2, 2
    rng = np.random.default_rng(1)
    X = rng.standard_normal((N, d))
    delta = rng.standard_normal((B, N))
    progs = [compile_spec(('sum', ('DOT', 1.0, np.array([0.7, 1.1]), 0.5, p, None), ('NOISE', 0.5)), d) for p in (2, 3)]
    Np = lib.roundup(N)
    rows, ks = Np + 128, (Np + 128) * Np
    K, Y, Ki = (dev.alloc(B * rows, Np, np.float64, zero=True) for _ in range(3))
    W, a, al = dev.alloc(B * Np, 128, np.float64), dev.alloc(B, Np, np.float64), dev.alloc(B, Np, np.float64)
    Xd, dd = dev.upload(X), dev.upload(delta)
    with pytest.raises(lib.G3Error, match='status -2'):
        dev.gp_factor_batched(progs, Xd, N, d, dd, K, ks, W, a)
    st = dev.gp_factor_batched([progs[0], progs[0]], Xd, N, d, dd, K, ks, W, a, raw=True)       # same exponent: accepted
    assert st.shape == (B, 6)
    # factor the two members one at a time into the batch layout, then the batched gradient against the single ones
    gmap = dev.grad_layout(progs[0])
    single = []
    Y1, Ki1, al1 = dev.alloc(Np, Np, np.float64), dev.alloc(Np, Np, np.float64), dev.alloc(1, Np, np.float64)
    for b in range(B):
        Kb = dev.wrap(K.offset(b * rows), rows, Np, Np, np.float64)
        Wb = dev.wrap(W.offset(b * Np), Np, 128, 128, np.float64)
        ab = dev.wrap(a.offset(b), 1, Np, Np, np.float64)
        st1 = dev.gp_factor(progs[b], Xd, N, d, dev.wrap(dd.offset(b), 1, N, N, np.float64), Kb, Wb, ab)
        assert st1['tries'] == 0 and st1['info'] == 0
        single.append(dev.gp_dlogp(progs[b], gmap, Xd, N, d, Kb, Wb, ab, Y1, Ki1, al1))
    before = dev.grad_path_stats()
    got = dev.gp_dlogp_batched(progs, gmap, Xd, N, d, K, ks, W, a, Y, Ki, al)
    after = dev.grad_path_stats()
    assert after['generated'] == before['generated'] and after['interpreted'] == before['interpreted'] + 1, (before, after)
    assert not np.allclose(single[0], single[1], rtol=1e-3)
    for b in range(B):
        np.testing.assert_allclose(got[b], single[b], rtol=1e-9, atol=1e-11 * np.abs(single[b]).max())


# ------------------------------------------------------------------ 5. process level
R2 = np.array([0.7, 1.3])
CASES = {
    'LIN+SE': dict(
        kernel=lambda g3, X: g3.LIN(X) + g3.SE(X),
        nat=dict(LIN_rate=R2, LIN_bias=0.5, SE_var=1.1, SE_rate=np.array([0.9, 1.2]), Noise_var=0.1, Bias_Bias=0.3),
        spec=('sum', ('DOT', 1.0, R2, 0.5, 1, None), ('SE', 1.1, np.array([0.9, 1.2]), None)),
        route={(0, 'rate'): 'LIN_rate', (0, 'alpha'): 'LIN_bias', (1, 'var'): 'SE_var', (1, 'rate'): 'SE_rate', (2, 'var'): 'Noise_var'},
        far=12.0),
    'POL*OU+VAR': dict(
        kernel=lambda g3, X: g3.POL(X, 2) * g3.OU(X) + g3.VAR(X),
        nat=dict(POL_rate=R2, POL_bias=0.5, OU_var=0.8, OU_rate=np.array([0.6, 0.9]), VAR_var=0.4, Noise_var=0.1, Bias_Bias=0.3),
        spec=('sum', ('prod', ('DOT', 1.0, R2, 0.5, 2, None), ('OU', 0.8, np.array([0.6, 0.9]), None)), ('VAR', 0.4)),
        route={(0, 'rate'): 'POL_rate', (0, 'alpha'): 'POL_bias', (1, 'var'): 'OU_var', (1, 'rate'): 'OU_rate', (2, 'var'): 'VAR_var',
               (3, 'var'): 'Noise_var'},
        far=4.0),
}


@pytest.mark.parametrize('N', [200, 1500])
@pytest.mark.parametrize('case', sorted(CASES))
def test_process_logp_predict_dlogp_match_the_oracle(patched_oracle, case, N):
    """GaussianProcess with a dot leaf in a sum / product, d = 2, noise 0.1, against the oracle at the tolerances
    tests/test_gpu_process.py uses for SE (test_process_matches_oracle_fixture, test_dlogp_matches_oracle_fixture): logp 1e-8
    relative, means atol 1e-8 * scale, variances 1e-7 * scale^2 with scale = max(1, |mean|max), covariance atol 1e-8, dlogp
    rtol 1e-8 + 1e-8 |want|max.  Half of the query points lie far from the origin, where the prior variance is >= 100x the
    one near it: the case a constant-diagonal shortcut gets wrong.  The oracle takes no jitter step on these inputs
    (asserted), so agreement is never an accident of two jitter paths."""
    import g3py_amd as g3
    orc = patched_oracle
    c = CASES[case]
    rng = np.random.default_rng(N)
    X = 2.0 * rng.standard_normal((N, 2))
    y = 0.4 * X[:, 0] - 0.2 * X[:, 1] + np.sin(X.sum(1)) + 0.3 * rng.standard_normal(N)
    M = 40
    Xs = np.concatenate([0.1 * rng.standard_normal((M // 2, 2)),
                         c['far'] * np.sign(rng.standard_normal((M // 2, 2))) * rng.uniform(0.9, 1.1, (M // 2, 2))])
    gp = g3.GaussianProcess(space=Xs, location=g3.Bias(), kernel=c['kernel'](g3, X))
    gp.observed(X, y)
    p = _params(gp, **c['nat'])
    ref = orc.GP(c['spec'], 0.1, ('Bias', 0.3))
    _, tries, fallback = orc.cholesky_robust(ref.prior_kernel(X, True), return_info=True)
    assert tries == 0 and not fallback
    prior_var = ref.kernel_diag(Xs, prior=True)
    assert prior_var[M // 2:].min() >= 100 * prior_var[:M // 2].max()
    lp = ref.logp(X, y)
    assert abs(gp.logp(p) - lp) <= 1e-8 * abs(lp)
    pred = gp.predict(p, var=True, cov=True)
    want_mean = ref.mean(Xs, X, y)
    scale = max(1.0, np.abs(want_mean).max())
    want_var, want_cov = ref.variance(Xs, X, y), ref.covariance(Xs, X)
    print('%s N=%d: |mean err| %.3g (tol %.3g), |var err| %.3g (tol %.3g), |cov err| %.3g (tol 1e-8), prior var max %.4g'
          % (case, N, np.abs(pred.mean - want_mean).max(), 1e-8 * scale, np.abs(pred.variance - want_var).max(), 1e-7 * scale ** 2,
             np.abs(pred.covariance - want_cov).max(), prior_var.max()))
    np.testing.assert_allclose(pred.mean, want_mean, atol=1e-8 * scale)
    np.testing.assert_allclose(pred.variance, want_var, atol=1e-7 * scale ** 2)
    np.testing.assert_allclose(pred.covariance, want_cov, atol=1e-8)
    # gradient: every hyper incl. the bias of the dot leaf
    g = ref.dlogp_natural(X, y)
    by = {}
    for leaf, pname, k, val in g['kernel']:
        name = c['route'].get((leaf, pname))
        if name is not None:
            by.setdefault(name, []).append(val)
    by['Bias_Bias'] = [g['mean'][0][2]]
    want = []
    for v in gp.model.vars:
        k = v.name[len(gp.name) + 1:]
        val = np.atleast_1d(np.asarray(c['nat'][k], dtype=float)) * np.ones(max(v.size, 1))
        want.append(np.asarray(by[k]) * (val if v.positive else 1.0))
    want = np.concatenate(want)
    got = gp.dlogp(p)
    assert len(got) == len(want) and any('_bias' in v.name for v in gp.model.vars)
    np.testing.assert_allclose(got, want, rtol=1e-8, atol=1e-8 * max(1.0, np.abs(want).max()))


def test_public_api_walkthrough_lin_plus_se():
    import g3py_amd as g3
    rng = np.random.default_rng(2)
    x = 2.0 * rng.standard_normal((150, 2))
    yv = 0.5 * x[:, 0] + np.sin(x[:, 1]) + 0.2 * rng.standard_normal(150)
    gp = g3.GaussianProcess(space=x, location=g3.Bias(), kernel=g3.LIN(x) + g3.SE(x))
    gp.observed(x, yv)
    p = gp.params_default
    assert np.isfinite(gp.logp(p)) and np.all(np.isfinite(gp.dlogp(p)))
    pred = gp.predict(p, var=True, quantiles=True, samples=5)
    assert np.all(np.isfinite(pred.mean)) and np.all(pred.variance >= 0) and np.all(np.isfinite(np.asarray(pred.samples)))
    a = gp.active.dict_to_array(p)
    chain = a + 0.05 * rng.standard_normal((8, len(a)))
    np.testing.assert_allclose(gp.logp_chain(chain), [gp.logp(r, array=True) for r in chain], rtol=1e-10)


# ------------------------------------------------------------------ 6. chains
@pytest.mark.parametrize('N', [128, 640])
def test_chains_equal_one_at_a_time(N):
    """logp_chain / dlogp_chain over 64 rows varying bias, rate, var: N = 128 one workgroup per member, N = 640 the batched
    sweep; tolerances of the existing chain tests (logp 1e-12 / 1e-10 relative, dlogp rtol 1e-8 + atol 1e-9)"""
    import g3py_amd as g3
    rng = np.random.default_rng(N)
    X = 2.0 * rng.standard_normal((N, 2))
    y = 0.4 * X[:, 0] + np.sin(X.sum(1)) + 0.3 * rng.standard_normal(N)
    gp = g3.GaussianProcess(space=X, location=g3.Bias(), kernel=g3.POL(X, 2) * g3.OU(X) + g3.NN(X))
    gp.observed(X, y)
    base = _params(gp, POL_rate=R2, POL_bias=0.5, OU_var=0.8, OU_rate=[0.6, 0.9], NN_var=0.7, NN_rate=[0.8, 1.1], NN_bias=0.4,
                   Noise_var=0.1, Bias_Bias=0.1)
    a0 = gp.active.dict_to_array(base)
    chain = a0 + 0.15 * rng.standard_normal((64, len(a0)))
    chain[0] = a0
    want = np.array([gp.logp(r, array=True) for r in chain], dtype=np.float64)
    got = np.asarray(gp.logp_chain(chain), dtype=np.float64)
    np.testing.assert_allclose(got, want, rtol=1e-12 if N == 128 else 1e-10)
    g1 = np.array([gp.dlogp(r, array=True) for r in chain])
    np.testing.assert_allclose(gp.dlogp_chain(chain), g1, rtol=1e-8, atol=1e-9)
    s = gp.device.gram_path_stats()
    assert s['interpreted'] == 0, s


# ------------------------------------------------------------------ 7. Student-t, multi-GPU driver at world 1
def test_student_t_logp_matches_oracle(patched_oracle):
    import g3py_amd as g3
    orc = patched_oracle
    c = CASES['LIN+SE']
    rng = np.random.default_rng(9)
    X = 2.0 * rng.standard_normal((200, 2))
    y = 0.4 * X[:, 0] + np.sin(X.sum(1)) + 0.3 * rng.standard_normal(200)
    tp = g3.TP(space=X[:20], location=g3.Bias(), kernel=c['kernel'](g3, X))
    tp.observed(X, y)
    p = _params(tp, Freedom_degree=3.5, **c['nat'])
    ref = orc.TP(c['spec'], 3.5, 0.1, ('Bias', 0.3))
    lp = ref.logp(X, y)
    assert abs(tp.logp(p) - lp) <= 1e-8 * abs(lp)
    assert np.all(np.isfinite(tp.dlogp(p)))


def test_distribute_world_one_equals_one_gpu(monkeypatch):
    """the multi-GPU driver with ONE rank through RCCL (what G3_FORCE_DIST=1 selects in bench.py): same logp / predict /
    dlogp as the in-library path for LIN + SE"""
    import g3py_amd as g3
    monkeypatch.setenv('G3_FORCE_DIST', '1')
    c = CASES['LIN+SE']
    rng = np.random.default_rng(4)
    X = 2.0 * rng.standard_normal((700, 2))
    y = 0.4 * X[:, 0] + np.sin(X.sum(1)) + 0.3 * rng.standard_normal(700)
    Xs = np.concatenate([0.1 * rng.standard_normal((30, 2)), 12.0 * np.sign(rng.standard_normal((30, 2)))])
    gp = g3.GaussianProcess(space=Xs, location=g3.Bias(), kernel=c['kernel'](g3, X))
    gp.observed(X, y)
    p = _params(gp, **c['nat'])
    lp1, pr1, g1 = gp.logp(p), gp.predict(p, var=True, cov=True), gp.dlogp(p)
    gp.distribute(None, 0, 1, nb=128)
    try:
        lp, pr, g = gp.logp(p), gp.predict(p, var=True, cov=True), gp.dlogp(p)
    finally:
        gp.undistribute()
    assert abs(lp - lp1) <= 1e-10 * abs(lp1)
    vs = max(1.0, np.abs(pr1.variance).max())
    np.testing.assert_allclose(pr.mean, pr1.mean, atol=1e-8 * max(1.0, np.abs(pr1.mean).max()))
    np.testing.assert_allclose(pr.variance, pr1.variance, atol=1e-8 * vs)
    np.testing.assert_allclose(pr.covariance, pr1.covariance, atol=1e-8 * vs)
    np.testing.assert_allclose(g, g1, rtol=1e-7, atol=1e-8 * np.abs(g1).max())
