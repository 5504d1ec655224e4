"""The Gram paths on inputs far from the origin.

Every covariance of the library depends on its inputs through differences alone (or is evaluated on them), so a
translation of the inputs must not change K.  tests/input_domain.py puts the same seeded grid points U at the origin
and at offsets c that are exact in the working type -- fp32: (2048, -2048, 1958); fp64: (2^30, -2^30, 2^20); a time
series in calendar years with a yearly period -- and holds every entry point against

  truth = the oracle on U in extended precision,    tol = 4 max|yard - truth| + 8 eps max|truth|,
  yard  = the oracle's direct formula in the working type on X = U + c

(tests/test_input_domain_host.py checks those conditions on the host).  Each case runs on the compile-time table or a
generated kernel (default context; the table carries `stationary (+|x) periodic` at d in {1, 2, 4, 8} only, hence the
d = 4 cases) and on the interpreter (a context created under G3_GRAM_JIT=0 G3_GRAM_NOFAST=1), and the path counters
are asserted.

What this guards: the periodic leaves (COS, SIN, SM) are evaluated from per-tile [cos, sin] tables of theta = 2 pi f x.
Formed as a plain product, theta is rounded by eps |theta|, which grows with |x| (and, measured from a point of the
tile, still with the tile's extent: the time series at c = 0 below); the kernels take it modulo 2 pi off the exact
product (g3_kernel_eval.h::trig_theta).  One MI355X run of each, max error over the symmetric, cross and row-block
Gram; `plain` is the library before trig_theta, `yard` is max|yard - truth|; tol is about 4 yard + 1e-6 (fp32), 2e-15 (fp64):

  case          kernel           path         plain     trig_theta  yard
  f32-far       COS              generated    1.8e-04   3.6e-07     3.4e-07
  f32-far       SIN              interpreted  1.4e-04   3.9e-07     4.9e-07
  f32-far       SM               generated    7.4e-05   2.2e-07     1.8e-07
  f32-far       T:SE*COS         interpreted  7.8e-04   3.7e-07     2.8e-07
  f32-far-d4    T:SE+SIN         table        1.2e-03   1.2e-06     1.2e-06
  f32-far-d4    T:SE*COS         table        5.5e-04   2.8e-07     2.8e-07
  f32-years     COS              generated    7.7e-04   2.4e-07     1.9e-05
  f32-years     T:SE*COS         table        9.3e-04   2.2e-07     3.8e-07
  f32-years-c0  SM               generated    2.4e-05   2.5e-07     1.5e-06
  f32-years-c0  T:SE*COS         table        2.6e-05   2.2e-07     3.8e-07
  f64-far       COS              generated    1.7e-07   4.8e-16     5.3e-16
  f64-far       T:SE*COS         interpreted  7.4e-07   5.0e-16     4.7e-16
  f64-far-d4    T:SE+SIN         table        6.6e-07   1.8e-15     2.1e-15
  f64-far-d4    T:MAT52+SM       table        2.3e-07   3.8e-16     4.2e-16

Every kernel without a periodic leaf, and every kernel at c = 0 but the time series' SM, MAT52+SM and SE*COS, passed
before as after.  Process figures (SE * COS + NOISE on the table, fp64, d = 4, c = 2^30; tolerance 1e-9 / 1e-8):
logdet 3.3e-08 -> 1.6e-15, a = L^-1 delta 7.9e-07 -> 2.6e-15; fp32, d = 3, c = 2048: a 2.5e-03 -> 6.9e-06 (tolerance 2e-3).
Gradient sums, fp64, fast path, d = 4, c = 2^30, the SE variance slot of SE * COS: 2.5e-07 -> about 1e-14 (tol 1.1e-12).
"""
import ctypes as C

import numpy as np
import pytest

import hostile_memory as hm
import input_domain as idm

pytestmark = pytest.mark.gpu

ROW0 = 128              # g3_gram_rows: rows [128, N) of the square covariance


@pytest.fixture(scope='module')
def devs():
    """name -> context: 'default', 'interp' (every Gram launch interpreted), 'generic' (every gradient sum interpreted);
    contexts read their knobs when they are created"""
    import g3py_amd as g3
    made = {'default': g3.Device.default()}
    with hm.environment(G3_GRAM_JIT=0, G3_GRAM_NOFAST=1):
        made['interp'] = g3.Device(0)
    with hm.environment(G3_GRAD_GENERIC=1):
        made['generic'] = g3.Device(0)
    yield made
    made['interp'].close()
    made['generic'].close()


def _moved(dev, before, grad=False):
    after = dev.grad_path_stats() if grad else dev.gram_path_stats()
    return {k: after[k] - before[k] for k in after}


def _gram(dev, prog, A, B, d, n1, n2, dtype, flags=0):
    out = dev.alloc(n1, n2, dtype, zero=True)
    dev.gram(prog, A, B, d, out, n1, n2, flags)
    return dev.download(out)


CASE_KERNELS = [(c, k) for c in idm.CASES for k in idm.kernels(c)]


@pytest.mark.parametrize('case,name', CASE_KERNELS, ids=['%s-%s' % ck for ck in CASE_KERNELS])
def test_gram_is_translation_invariant(devs, case, name):
    """g3_gram (symmetric and cross), g3_gram_rows and g3_gram_diag on the table / generated path and on the interpreter"""
    import g3py_amd._lib as lib
    from g3py_amd.device import compile_spec
    assert idm.offsets_exact(case)
    T, d = idm.case_dtype(case), idm.case_d(case)
    _, _, X, Xs = idm.inputs(case)
    spec = idm.kernels(case)[name]
    prog = compile_spec(spec, d)
    bad = []
    for path in ('default', 'interp'):
        dev = devs[path]
        want = 'interpreted' if path == 'interp' else 'table' if idm.on_table(case, name) else 'generated'
        A, B = dev.upload(X), dev.upload(Xs)
        before = dev.gram_path_stats()
        got = {'sym': (_gram(dev, prog, A, None, d, idm.N, idm.N, T), False, slice(None)),
               'cross': (_gram(dev, prog, B, A, d, idm.M, idm.N, T), True, slice(None))}
        rows = dev.alloc(idm.N - ROW0, idm.N, T, zero=True)
        assert dev.lib.g3_gram_rows(dev.ctx, C.byref(prog), A.ptr, idm.N, A.ld, d, ROW0, idm.N - ROW0, lib.dtype_code(T),
                                    rows.ptr, rows.ld, 0) == 0
        got['rows'] = (dev.download(rows), False, slice(ROW0, idm.N))
        moved = _moved(dev, before)
        assert moved[want] == 3 and sum(moved.values()) == 3, (case, name, path, want, moved)
        diag = dev.alloc(1, idm.N, T)
        dev.gram_diag(prog, A, d, diag)
        got['diag'] = (dev.download(diag)[0], False, None)
        for what, (K, cross, sel) in got.items():
            tr = idm.truth(case, name, cross)
            tr = np.diag(tr) if sel is None else tr[sel]
            assert K.dtype == T and K.shape == tr.shape
            e = float(np.abs(K.astype(np.longdouble) - tr).max())
            ye, tol = idm.yard_err(case, name, cross), idm.tol(case, name, cross)
            print('%-13s %-20s %-11s %-5s err %.3e  |yard - truth| %.3e  tol %.3e%s' %
                  (case, name, want, what, e, ye, tol, '' if e <= tol else '   <-- FAIL'))
            if not e <= tol:
                bad.append((path, want, what, e, tol))
    assert not bad, (case, name, bad)


@pytest.mark.parametrize('case,name', [('f64-c0', 'MAT52+COS'), ('f32-far', 'SM'), ('f64-far-d4', 'T:SE+COS+NOISE'),
                                       ('f32-years', 'T:SE+SIN')])
def test_a_non_finite_point_costs_its_own_row_and_column(devs, case, name):
    """NaN coordinates at the first column point of each tile (points 0 and 128), where a table measured from a point of the
    tile would take its origin: they must cost their own rows and columns of K and nothing else, as tt_to_num
    (tensors.py:90-92) on the reference's K prescribes"""
    import g3py_amd._lib as lib
    from g3py_amd.device import compile_spec
    T, d = idm.case_dtype(case), idm.case_d(case)
    _, _, X, _ = idm.inputs(case)
    Xn = X.copy()
    Xn[0, 0] = Xn[idm.GTN, d - 1] = np.nan
    prog = compile_spec(idm.kernels(case)[name], d)
    hit = np.zeros(idm.N, bool)
    hit[[0, idm.GTN]] = True
    for path in ('default', 'interp'):
        dev = devs[path]
        K = _gram(dev, prog, dev.upload(Xn), None, d, idm.N, idm.N, T, flags=lib.G3_GRAM_SCRUB)
        assert not K[hit].any() and not K[:, hit].any(), (case, name, path)
        keep = np.ix_(~hit, ~hit)
        e = float(np.abs(K[keep].astype(np.longdouble) - idm.truth(case, name)[keep]).max())
        print('%-13s %-20s %-8s err off the NaN rows %.3e  tol %.3e' % (case, name, path, e, idm.tol(case, name)))
        assert e <= idm.tol(case, name), (case, name, path, e)


# ------------------------------------------------------------------------------------------------ the process entry points
def _process_spec(case, var=1.0):
    d = idm.case_d(case)
    r = np.linspace(0.6, 1.4, d)
    f = np.ones(1) if d == 1 else np.full(d, 0.7)
    spec_f = ('prod', ('SE', var, r, None), ('COS', 1.0, f, None))
    return spec_f, ('sum', spec_f, ('NOISE', 0.1))


def _targets(case):
    U = idm.inputs(case)[0]
    rng = np.random.default_rng(77)
    return np.sin(U.sum(1) / np.sqrt(U.shape[1])) + 0.1 * rng.standard_normal(len(U))


def _process_oracle(case, var=1.0):
    """logdet, quad, a, mu, ss of the fp64 oracle on the UN-offset points"""
    import scipy.linalg as sl
    from oracle import g3_oracle as orc
    U, Us, _, _ = idm.inputs(case)
    spec_f, spec = _process_spec(case, var)
    L = np.linalg.cholesky(orc.kernel_cov(spec, U))
    a = sl.solve_triangular(L, _targets(case), lower=True)
    V = sl.solve_triangular(L, orc.kernel_cov(spec_f, Us, U).T, lower=True).T
    return float(np.log(np.diag(L)).sum()), float(a @ a), a, V @ a, (V * V).sum(1)


def _close(what, got, ref, T, note, bad):
    """the suite's figures against the oracle: fp64 scalars 1e-9 (relative), vectors 1e-8 (absolute); fp32 as
    test_fp32_process_close_to_fp64: scalars 1e-4 (relative), vectors 2e-3 (absolute)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if ref.ndim == 0:
        e, tol = abs(got - ref) / abs(ref), (1e-9 if T == np.float64 else 1e-4)
    else:
        e, tol = np.abs(got - ref).max(), (1e-8 if T == np.float64 else 2e-3)
    print('%-40s %-7s err %.3e  tol %.1e%s' % (note, what, e, tol, '' if e <= tol else '   <-- FAIL'))
    if not e <= tol:
        bad.append((note, what, float(e), tol))


PROCESS_CASES = [c for c in idm.CASES if idm.case_d(c) > 1]


@pytest.mark.parametrize('case', PROCESS_CASES)
def test_factor_and_cross_are_translation_invariant(devs, case):
    """g3_gp_factor and g3_gp_cross with SE * COS + NOISE(0.1), N = 200, M = 70: the oracle's figures on U, and a clean
    factorisation (info == 0, tries == 0) at every offset as at c = 0"""
    from g3py_amd import _lib
    from g3py_amd.device import compile_spec
    T, d = idm.case_dtype(case), idm.case_d(case)
    _, _, X, Xs = idm.inputs(case)
    spec_f, spec = _process_spec(case)
    logdet, quad, a_ref, mu_ref, ss_ref = _process_oracle(case)
    Np, Mp = _lib.roundup(idm.N), _lib.roundup(idm.M, 128)
    bad = []
    for path in ('default', 'interp'):
        dev = devs[path]
        Xd = dev.upload(X)
        K, a, W = dev.alloc(Np + 128, Np, T), dev.alloc(1, Np, T), dev.alloc_inverses(Np, T)
        before = dev.gram_path_stats()
        st = dev.gp_factor(compile_spec(spec, d), Xd, idm.N, d, dev.upload(_targets(case).astype(T)), K, W, a)
        V, mu, ss = dev.alloc(Mp, Np, T), dev.alloc(1, Mp, T), dev.alloc(1, Mp, T)
        dev.gp_cross(compile_spec(spec_f, d), dev.upload(Xs), idm.M, Xd, idm.N, d, K, W, a, V, mu, ss)
        want = 'interpreted' if path == 'interp' else 'table' if d == 4 else 'generated'
        moved = _moved(dev, before)
        assert moved[want] >= 2 and sum(moved.values()) == moved[want], (case, path, moved)
        assert st['info'] == 0 and st['tries'] == 0 and not st['fallback'] and st['nonfinite'] == 0, (case, path, st)
        note = '%s %s' % (case, want)
        _close('logdet', st['logdet'], logdet, T, note, bad)
        _close('quad', st['quad'], quad, T, note, bad)
        _close('a', dev.download(a, 1, idm.N)[0], a_ref, T, note, bad)
        _close('mu', dev.download(mu, 1, idm.M)[0], mu_ref, T, note, bad)
        _close('ss', dev.download(ss, 1, idm.M)[0], ss_ref, T, note, bad)
    assert not bad, bad


@pytest.mark.parametrize('case', PROCESS_CASES)
def test_chain_gram_is_translation_invariant(devs, case):
    """the batched Gram launch (member in grid.z) through g3_gp_factor_batched, B = 3 members at N = 200.  The members'
    covariances are factored in place, so each member's logdet, quad and a = L^-1 delta are held against the oracle on U"""
    from g3py_amd import _lib
    from g3py_amd.device import compile_spec
    T, d = idm.case_dtype(case), idm.case_d(case)
    _, _, X, _ = idm.inputs(case)
    Bn, Np = 3, _lib.roundup(idm.N)
    variances = [1.0, 1.3, 0.7]
    progs = [compile_spec(_process_spec(case, v)[1], d) for v in variances]
    y = _targets(case)
    bad = []
    for path in ('default', 'interp'):
        dev = devs[path]
        K, W, a = dev.alloc(Bn * (Np + 128), Np, T), dev.alloc(Bn * Np, 128, T), dev.alloc(Bn, Np, T)
        before = dev.gram_path_stats()
        st = dev.gp_factor_batched(progs, dev.upload(X), idm.N, d, dev.upload(np.tile(y, (Bn, 1)).astype(T)), K,
                                   (Np + 128) * Np, W, a, raw=True)
        want = 'interpreted' if path == 'interp' else 'generated'      # the table serves one member per launch: not used here
        moved = _moved(dev, before)
        assert moved[want] >= 1 and sum(moved.values()) == moved[want], (case, path, moved)
        assert not st[:, 2].any() and not st[:, 3].any() and not st[:, 4].any() and not st[:, 5].any(), (case, path, st)
        got_a = dev.download(a, Bn, idm.N)
        for b, v in enumerate(variances):
            logdet, quad, a_ref, _, _ = _process_oracle(case, v)
            note = '%s %s member %d' % (case, want, b)
            _close('logdet', st[b, 0], logdet, T, note, bad)
            _close('quad', st[b, 1], quad, T, note, bad)
            _close('a', got_a[b], a_ref, T, note, bad)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the gradient sums
GRAD_KERNELS = list(idm.TABLE_SHAPES)


@pytest.mark.parametrize('name', GRAD_KERNELS)
@pytest.mark.parametrize('case', ['f64-c0-d4', 'f64-far-d4', 'f64-far'])
def test_gram_grad_is_translation_invariant(devs, case, name):
    """g3_gram_grad in fp64 at c = 2^30 (and at the origin): the register fast path (d = 4: its trig tables), a generated
    kernel (d = 3) and the generic kernel (G3_GRAD_GENERIC=1).  Truth: the oracle's dK/dparam on U in extended precision,
    contracted with the same K^-1 stand-in and alpha; yard: the same contraction of the fp64 dK/dparam on X;
    tol = 4 |yard - truth| + 8 eps * 1/2 sum |G_ij dK_ij| (the magnitude of the sum's terms)"""
    from g3py_amd.device import compile_spec
    from oracle import g3_oracle as orc
    d = idm.case_d(case)
    U, _, X, _ = idm.inputs(case)
    spec = idm.kernels(case)[name]
    rng = np.random.default_rng(5)
    A = rng.standard_normal((idm.N, idm.N))
    G = (A + A.T) / 2
    alpha = rng.standard_normal(idm.N)
    Gfull = (np.outer(alpha, alpha) - G).astype(np.longdouble)
    _, g_true = orc.kernel_cov_grads(spec, U, dtype=np.longdouble)
    _, g_yard = orc.kernel_cov_grads(spec, X, dtype=np.float64)
    prog = compile_spec(spec, d)
    bad = []
    for path in ('default', 'generic'):
        dev = devs[path]
        gmap = dev.grad_layout(prog)
        assert gmap.nslots == len(g_true)
        before = dev.grad_path_stats()
        out = dev.gram_grad(prog, gmap, dev.upload(X), idm.N, d, dev.upload(np.tril(G)), dev.upload(alpha))
        want = 'interpreted' if path == 'generic' else 'table' if d == 4 else 'generated'
        moved = _moved(dev, before, grad=True)
        assert moved[want] == 1 and sum(moved.values()) == 1, (case, name, path, moved)
        for (leaf, pname, k, dK), (_, _, _, dKy) in zip(g_true, g_yard):
            slot = getattr(gmap, pname)[leaf] + (0 if k is None else k)
            truth = 0.5 * np.sum(Gfull * dK)
            yard = 0.5 * np.sum(Gfull * dKy.astype(np.longdouble))
            scale = 0.5 * np.sum(np.abs(Gfull * dK))
            tol = float(4 * abs(yard - truth) + 8 * np.finfo(np.float64).eps * scale)
            e = float(abs(np.longdouble(out[slot]) - truth))
            print('%-11s %-13s %-11s leaf %d %-5s %-4s err %.3e  |yard - truth| %.3e  tol %.3e%s' %
                  (case, name, want, leaf, pname, '' if k is None else k, e, float(abs(yard - truth)), tol,
                   '' if e <= tol else '   <-- FAIL'))
            if not e <= tol:
                bad.append((path, want, leaf, pname, k, e, tol))
    assert not bad, (case, name, bad)
