"""Wide inputs on the GPU: the Gram, gradient and chain kernels at 5 ... 40 input columns (G3_MAXCOLS = 40, leaves on up to
G3_MAXD = 32 of them), element by element against the fp64 oracle (tests/wide_reference.py): the d = 16 compile-time kernels of
BASELINE config 5, every width between the table's entries on generated kernels and on the interpreter, a leading dimension
larger than d (the extra columns NaN), and both sides of the size rules that depend on d -- the interpreter's trig tables
(16 pairs), the generated kernel's limits (24 pairs, 96 KiB of LDS), the gradient's 40 register accumulators and its 32-slot
LDS window.  Tolerances are the project's derived ones (tests/test_gpu_gram.py, tests/test_gpu_fuzz.py): see wide_reference."""
import ctypes as C
import functools

import numpy as np
import pytest

import wide_reference as wr

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
DTYPES = [pytest.param(F64, id='f64'), pytest.param(F32, id='f32')]


@pytest.fixture(scope='module')
def dev():
    import g3py_amd as g3
    return g3.Device.default()


def _interpreting_device(monkeypatch):
    """a second context that interprets everything (the knobs are read when a context is created)"""
    import g3py_amd as g3
    monkeypatch.setenv('G3_GRAM_JIT', '0')
    monkeypatch.setenv('G3_GRAM_NOFAST', '1')
    monkeypatch.setenv('G3_GRAD_GENERIC', '1')
    return g3.Device(0)


@functools.lru_cache(maxsize=None)
def _ref(key, n, m, d, f32):
    """the oracle's square covariance of inputs(n, d) and its cross block K(inputs(m, d, 1), inputs(n, d)) for the spec
    registered under `key`, on the inputs as the kernel's type sees them; computed once, read-only"""
    from oracle import g3_oracle as orc
    spec = _SPECS[key]
    dtype = F32 if f32 else F64
    X, Xs = wr.as_seen(wr.inputs(n, d), dtype), wr.as_seen(wr.inputs(m, d, 1), dtype)
    sq, cr = orc.kernel_cov(spec, X), orc.kernel_cov(spec, Xs, X)
    wr.assert_condition(sq)
    wr.assert_condition(cr, square=False)
    sq.setflags(write=False)
    cr.setflags(write=False)
    return sq, cr


_SPECS = {}


def _register(key, spec):
    _SPECS[key] = spec
    return key


def _close(got, ref, dtype, what=''):
    np.testing.assert_allclose(got, ref, err_msg=what, **wr.gram_tol(dtype, ref))


# ----------------------------------------------------------------------------- A.1 the compile-time table at d = 16
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', wr.STATIONARY)
@pytest.mark.parametrize('layout', ['d16', 'd16_ldx19', 'd3'])
def test_table_kernels_at_16_columns_match_the_oracle(dev, layout, kind, dtype):
    """gram_kernel<T, 16, kind> (config 5's kernel in fp32) element by element: N = 300 (ragged edge tiles), the lower-padded
    form and the 70 x 300 cross block; N = 391 with an odd leading dimension (general loop everywhere) against the same matrix
    padded to 512 (interior loop): equal to 1e-14 (fp64; the same bound in units of the type's rounding for fp32), the guard
    region exactly identity / zero; g3_gram_rows puts the noise on the true diagonal; g3_gram_diag; every launch is counted
    on the table.  The same at d = 3 and with ldx = 19 (three NaN columns behind the 16)"""
    import g3py_amd._lib as lib
    from g3py_amd.device import compile_spec
    from oracle import g3_oracle as orc
    d = 3 if layout == 'd3' else 16
    extra = 3 if layout == 'd16_ldx19' else 0
    f32 = dtype == F32
    same = dict(rtol=1e-14 * (np.finfo(dtype).eps / np.finfo(F64).eps), atol=0)
    for noise in ((0.1,) if layout == 'd3' else (None, 0.1)):
        base = wr.leaf(kind, np.arange(d))
        spec = base if noise is None else orc.with_noise(base, noise)
        before = dev.gram_path_stats()
        launches = 0
        # N = 300: square, lower + identity padding + scrub, cross
        k300 = _register(('table', kind, noise, d), spec)
        sq, cr = _ref(k300, 300, 70, d, f32)
        A, S = wr.upload(dev, wr.inputs(300, d), dtype, extra), wr.upload(dev, wr.inputs(70, d, 1), dtype, extra)
        assert A.ld == d + extra
        got = wr.gram(dev, spec, d, A, dtype=dtype)
        _close(got, sq, dtype, 'square')
        pad = lib.roundup(300)
        full = wr.gram(dev, spec, d, A, dtype=dtype, flags=lib.G3_GRAM_PAD_EYE | lib.G3_GRAM_SCRUB, pad=pad)
        _close(full[:300, :300], sq, dtype, 'padded')
        np.testing.assert_array_equal(full[300:, 300:], np.eye(pad - 300))
        assert not full[:300, 300:].any() and not full[300:, :300].any()
        low = wr.gram(dev, spec, d, A, dtype=dtype, flags=lib.G3_GRAM_LOWER | lib.G3_GRAM_PAD_EYE | lib.G3_GRAM_SCRUB, pad=pad)
        np.testing.assert_array_equal(np.tril(low[:300, :300]), np.tril(full[:300, :300]))
        np.testing.assert_array_equal(low[300:, 300:], np.eye(pad - 300))
        assert not low[300:, :300].any()
        _close(wr.gram(dev, spec, d, S, A, dtype=dtype), cr, dtype, 'cross')
        launches += 4
        # N = 391: general loop (ld = 391) against interior loop (ld = 512)
        sq391, _ = _ref(k300, 391, 70, d, f32)
        A391 = wr.upload(dev, wr.inputs(391, d), dtype, extra)
        edge = wr.gram(dev, spec, d, A391, dtype=dtype)
        even = wr.gram(dev, spec, d, A391, dtype=dtype, flags=lib.G3_GRAM_PAD_EYE, pad=512)
        _close(edge, sq391, dtype, 'N=391 general loop')
        _close(even[:391, :391], sq391, dtype, 'N=391 interior loop')
        np.testing.assert_allclose(even[:391, :391], edge, **same)
        np.testing.assert_array_equal(even[391:, 391:], np.eye(512 - 391))
        assert not even[:391, 391:].any() and not even[391:, :391].any()
        launches += 2
        # rows [128, 256) of the square covariance: the noise sits where i + 128 == j
        prog = compile_spec(spec, d)
        out = dev.alloc(128, 256, dtype, zero=True)
        assert dev.lib.g3_gram_rows(dev.ctx, C.byref(prog), A391.ptr, 391, A391.ld, d, 128, 128, lib.dtype_code(dtype), out.ptr, out.ld,
                                    lib.G3_GRAM_PAD_EYE) == 0
        rows = dev.download(out)
        np.testing.assert_array_equal(rows, even[128:256, :256])
        _close(rows, sq391[128:256, :256], dtype, 'rows')
        launches += 1
        stats = dev.gram_path_stats()
        assert stats['table'] == before['table'] + launches and stats['generated'] == before['generated'] \
            and stats['interpreted'] == before['interpreted'], (before, stats, launches)
        dg = dev.alloc(1, 391, dtype)
        dev.gram_diag(prog, A391, d, dg)
        _close(dev.download(dg)[0], np.diag(sq391), dtype, 'diag')
        for b in (A, S, A391, out, dg):
            b.free()


# ----------------------------------------------------------------------------- A.2 leaving the table
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('d', [16, 3])
def test_stationary_plus_periodic_off_the_table_runs_a_generated_kernel(dev, d, dtype):
    """the periodic second term is instantiated for D in {1, 2, 4, 8} only: MAT52 + COS on all columns at d = 16 and d = 3
    leaves the table for a kernel generated for the expression (COS at 0.2: at 0.4 and d = 3 the sum comes within 0.03 of zero
    and the reference's condition refuses it)"""
    from oracle import g3_oracle as orc
    spec = orc.with_noise(wr.se_plus_cos(d, d, kind='MAT52', cvar=0.2), 0.1)
    sq, cr = _ref(_register(('mat52+cos', d), spec), 300, 70, d, dtype == F32)
    A, S = wr.upload(dev, wr.inputs(300, d), dtype), wr.upload(dev, wr.inputs(70, d, 1), dtype)
    before = dev.gram_path_stats()
    _close(wr.gram(dev, spec, d, A, dtype=dtype), sq, dtype, 'square')
    _close(wr.gram(dev, spec, d, S, A, dtype=dtype), cr, dtype, 'cross')
    after = dev.gram_path_stats()
    assert after['generated'] == before['generated'] + 2 and after['table'] == before['table'] \
        and after['interpreted'] == before['interpreted'], (before, after)


# ----------------------------------------------------------------------------- A.3 every width in between
SWAP_D = 17


@pytest.mark.parametrize('d', wr.GRAM_WIDTHS)
def test_every_width_generated_and_interpreted_match_the_oracle(monkeypatch, d):
    """d = 5 ... 40 (none on the table): SE on all (at d > 32: the top 32) columns, MAT52[even columns] * RQ[odd columns] +
    WN[last column], SE with dims in descending order; fp64 square and cross on a default context (generated kernels) and
    on one that interprets, each against the oracle and against each other at 1e-13; fp32 on the default context; the same
    with ldx = d + 3 and NaN behind the columns: bit-identical.  At d = 17 two input columns are swapped on the device side
    only: the result moves by more than 100 x the tolerance (the test would see a kernel that permutes columns)"""
    import g3py_amd as g3
    dev1 = g3.Device(0)
    dev0 = _interpreting_device(monkeypatch)
    try:
        X, Xs = wr.inputs(300, d), wr.inputs(70, d, 1)
        specs = wr.width_specs(d)
        if d not in (9, 32, 40):
            del specs['SE[descending]']
        for name, spec in specs.items():
            sq, cr = _ref(_register(('width', name, d), spec), 300, 70, d, False)
            got = {}
            for dv in (dev1, dev0):
                A, S = wr.upload(dv, X, F64), wr.upload(dv, Xs, F64)
                got[dv] = (wr.gram(dv, spec, d, A), wr.gram(dv, spec, d, S, A))
                _close(got[dv][0], sq, F64, '%s d=%d square' % (name, d))
                _close(got[dv][1], cr, F64, '%s d=%d cross' % (name, d))
                Ap, Sp = wr.upload(dv, X, F64, 3), wr.upload(dv, Xs, F64, 3)          # ldx = d + 3, NaN behind the columns
                np.testing.assert_array_equal(wr.gram(dv, spec, d, Ap), got[dv][0])
                np.testing.assert_array_equal(wr.gram(dv, spec, d, Sp, Ap), got[dv][1])
                np.testing.assert_array_equal(wr.gram(dv, spec, d, Sp, A), got[dv][1])  # two leading dimensions in one call
            for a, b in zip(got[dev1], got[dev0]):
                np.testing.assert_allclose(a, b, rtol=1e-13, atol=1e-14 * max(1.0, np.abs(b).max()), err_msg='%s d=%d' % (name, d))
            if name == 'MAT52*RQ+WN' or (name == 'SE' and d in (17, 40)):
                sq32, cr32 = _ref(('width', name, d), 300, 70, d, True)
                A, S = wr.upload(dev1, X, F32, 3), wr.upload(dev1, Xs, F32)
                _close(wr.gram(dev1, spec, d, A, dtype=F32), sq32, F32, '%s d=%d fp32 square' % (name, d))
                _close(wr.gram(dev1, spec, d, S, A, dtype=F32), cr32, F32, '%s d=%d fp32 cross' % (name, d))
            if name == 'SE' and d == SWAP_D:
                Xw = X.copy()
                Xw[:, [0, d - 1]] = X[:, [d - 1, 0]]
                tol = wr.gram_tol(F64, sq)
                moved = np.abs(wr.gram(dev1, spec, d, wr.upload(dev1, Xw, F64)) - sq) / (tol['atol'] + tol['rtol'] * np.abs(sq))
                assert moved.max() > 100, moved.max()
        s1, s0 = dev1.gram_path_stats(), dev0.gram_path_stats()
        assert s1['interpreted'] == 0 and s1['table'] == 0 and s1['generated'] > 0, s1
        assert s0['generated'] == 0 and s0['table'] == 0 and s0['interpreted'] > 0, s0
    finally:
        dev0.close()
        dev1.close()


# ----------------------------------------------------------------------------- A.4 LDS and table-size boundaries
@pytest.mark.parametrize('case', sorted(wr.boundary_cases()))
def test_lds_and_trig_table_boundaries(monkeypatch, case):
    """1.3 SE(top 32 columns) + 0.4 COS / SM(first columns) + noise 0.1 on both sides of the size rules of g3_gram.hip and
    g3_gram_jit.hip: every case returns 0 from g3_gram and the oracle's values, fp64 and fp32, square and cross, on a default
    context and with the interpreter forced.  Dynamic LDS asked for, from the two files' formulas
    (generated: 192 ((d|1) + ((2 pairs)|1)) size, declined above 24 pairs or 96 KiB = 98304 B; interpreted: 192 ((d|1) + 2 pairs + 1) size
    with tables for <= 16 pairs, 192 (d|1) size without), and the path that serves the default context:

        case         pairs   generated fp64 / fp32       interpreted fp64 / fp32    default context fp64 / fp32
        d16_cos16     16      76800 /  38400               76800 / 38400            generated   / generated
        d32_cos16     16     101376 /  50688 (fp64 > 96K) 101376 / 50688            interpreted / generated
        d32_cos17     17     104448 /  52224 (fp64 > 96K)  50688 / 25344 (no table) interpreted / generated
        d32_cos24     24     125952 /  62976 (fp64 > 96K)  50688 / 25344 (no table) interpreted / generated
        d32_cos25     25     declined: > 24 pairs          50688 / 25344 (no table) interpreted / interpreted
        d40_cos12     12     101376 /  50688 (fp64 > 96K) 101376 / 50688            interpreted / generated
        d40_sm8        8      89088 /  44544               89088 / 44544            generated   / generated

    The last column is what an MI355X run of this test printed (the forced context: `interpreted` everywhere).  Four
    interpreter launches ask for more than 64 KiB (76800, 89088, 101376, 101376 B) of a kernel that nothing opts in above
    64 KiB: on gfx950 (160 KiB of LDS per workgroup) the runtime grants them and the values are the oracle's, so the library
    needed no change.  The counters are asserted only where the rule in the code is unambiguous: above 24 pairs or 96 KiB
    `generated` does not rise; the forced context only interprets."""
    import g3py_amd as g3
    from oracle import g3_oracle as orc
    d, core, pairs = wr.boundary_cases()[case]
    spec = orc.with_noise(core, 0.1)
    key = _register(('boundary', case), spec)
    dev1 = g3.Device(0)
    dev0 = _interpreting_device(monkeypatch)
    try:
        for dtype in (F64, F32):
            size = np.dtype(dtype).itemsize
            sq, cr = _ref(key, 300, 70, d, dtype == F32)
            for dv in (dev1, dev0):
                A, S = wr.upload(dv, wr.inputs(300, d), dtype), wr.upload(dv, wr.inputs(70, d, 1), dtype)
                before = dv.gram_path_stats()
                got_sq = wr.gram(dv, spec, d, A, dtype=dtype)               # Device.gram raises unless g3_gram returns 0
                got_cr = wr.gram(dv, spec, d, S, A, dtype=dtype)
                after = dv.gram_path_stats()
                rose = {k: after[k] - before[k] for k in after}
                print('%s %s %s: generated asks %d B%s, interpreted asks %d B; served by %s' % (
                    case, np.dtype(dtype).name, 'default' if dv is dev1 else 'forced interpreter', wr.lds_generated(d, pairs, size),
                    ' (declined)' if wr.generated_declines(d, pairs, size) else '', wr.lds_interpreted(d, pairs, size), rose))
                _close(got_sq, sq, dtype, '%s square' % case)
                _close(got_cr, cr, dtype, '%s cross' % case)
                assert sum(rose.values()) == 2 and rose['table'] == 0, rose
                if dv is dev0:
                    assert rose['interpreted'] == 2, rose
                elif wr.generated_declines(d, pairs, size):
                    assert rose['generated'] == 0 and rose['interpreted'] == 2, rose
    finally:
        dev0.close()
        dev1.close()


# ----------------------------------------------------------------------------- B. gradient sums
N_GRAD = 203


@functools.lru_cache(maxsize=None)
def _grad_ref(name, f32):
    d, spec, slots = wr.gradient_specs()[name]
    G, alpha = wr.grad_problem(N_GRAD, 5)
    dtype = F32 if f32 else F64
    K, ref = wr.grad_reference(spec, wr.as_seen(wr.inputs(N_GRAD, d), dtype), wr.as_seen(G, dtype), wr.as_seen(alpha, dtype))
    if name != 'd40_se_times_cos':
        wr.assert_condition(K)
    else:       # a product with COS crosses zero wherever the cosine does: the factor that can underflow is the SE leaf
        from oracle import g3_oracle as orc
        wr.assert_condition(orc.kernel_cov(wr.leaf('SE', wr.top(40)), wr.inputs(N_GRAD, d)))
    assert len(ref) == slots
    return ref


def _run_grad(dv, name, dtype, extra=0, rows=False):
    """g3_gram_grad of the named structure on `dv`: every slot against the oracle, a bit-identical repeat; rows=True: three
    disjoint row ranges (the last ragged) add up to the full call"""
    from g3py_amd.device import compile_spec
    d, spec, slots = wr.gradient_specs()[name]
    G, alpha = wr.grad_problem(N_GRAD, 5)
    prog = compile_spec(spec, d)
    gmap = dv.grad_layout(prog)
    assert gmap.nslots == slots
    Xd = wr.upload(dv, wr.inputs(N_GRAD, d), dtype, extra)
    Gd, ad = dv.upload(np.tril(G).astype(dtype)), dv.upload(alpha.astype(dtype))
    out = dv.gram_grad(prog, gmap, Xd, N_GRAD, d, Gd, ad)
    wr.assert_slots(out, gmap, _grad_ref(name, dtype == F32), 1e-10 if dtype == F64 else 2e-4, '%s %s' % (name, np.dtype(dtype).name))
    np.testing.assert_array_equal(dv.gram_grad(prog, gmap, Xd, N_GRAD, d, Gd, ad), out)
    if rows:
        tot = np.zeros(gmap.nslots)
        for r0, nr in ((0, 64), (64, 64), (128, N_GRAD - 128)):
            tot += dv.gram_grad_rows(prog, gmap, Xd, N_GRAD, d, r0, nr, dv.upload(np.ascontiguousarray(np.tril(G)[r0:r0 + nr]).astype(dtype)), ad)
        np.testing.assert_allclose(tot, out, rtol=1e-12, atol=1e-12 * np.abs(out).max())
    return out


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('kind', wr.STATIONARY)
def test_gradient_table_at_16_columns(dev, kind, dtype):
    """gram_grad_se<16> (config 5's gradient kernel): every slot of the five stationary kinds, with and without noise"""
    for name in ('d16_%s' % kind, 'd16_%s_noise' % kind):
        before = dev.grad_path_stats()
        _run_grad(dev, name, dtype, rows=(kind == 'SE' and name.endswith('noise')))
        after = dev.grad_path_stats()
        assert after['table'] > before['table'] and after['generated'] == before['generated'] \
            and after['interpreted'] == before['interpreted'], (before, after)


@pytest.mark.parametrize('dtype', DTYPES)
def test_gradient_slot_limits_on_wide_inputs(monkeypatch, dtype):
    """d = 38, SE on 32 columns + OU on the other 6: 40 slots, the last size with register accumulators
    (G3_GRAD_JIT_MAXSLOTS); with noise 41, the first interpreted one.  d = 31 / 32, SE on all columns, interpreter forced: 32
    slots are one LDS window, 33 are two.  d = 40, SE[top 32] * COS[12 columns] + noise (47 slots) with ldx = 43, both
    contexts, and its row ranges"""
    import g3py_amd as g3
    dev1 = g3.Device(0)
    dev0 = _interpreting_device(monkeypatch)
    try:
        for name, dv, path in (('d38_40slots', dev1, 'generated'), ('d38_41slots', dev1, 'interpreted'),
                               ('d38_40slots', dev0, 'interpreted'), ('d31_32slots', dev0, 'interpreted'),
                               ('d32_33slots', dev0, 'interpreted'), ('d31_32slots', dev1, 'generated'),
                               ('d32_33slots', dev1, 'generated'), ('d40_se_times_cos', dev1, 'interpreted'),
                               ('d40_se_times_cos', dev0, 'interpreted')):
            before = dv.grad_path_stats()
            wide = name == 'd40_se_times_cos'
            _run_grad(dv, name, dtype, extra=3 if wide else 0, rows=wide)
            after = dv.grad_path_stats()
            rose = {k: after[k] - before[k] for k in after}
            print('%s %s %s: %d slots served by %s' % (name, np.dtype(dtype).name, 'default' if dv is dev1 else 'forced interpreter',
                                                      wr.gradient_specs()[name][2], rose))
            others = [k for k in rose if k != path]
            assert rose[path] > 0 and not any(rose[k] for k in others), (name, path, rose)
    finally:
        dev0.close()
        dev1.close()


# ----------------------------------------------------------------------------- C. whole evaluations and chains
def _eval_problem(d, N, M):
    """inputs, observations and the expression of the whole-evaluation tests: config 5's ARD SE + noise at d = 16; SE on the top
    32 columns + COS on 12 + noise at d = 40 (fp64: the interpreter with its trig tables)"""
    X, Xs = wr.inputs(N, d), wr.inputs(M, d, 1)
    rng = np.random.default_rng(d + N)
    y = np.sin(X.sum(1) / np.sqrt(d)) + 0.1 * rng.standard_normal(N)
    spec = wr.leaf('SE', np.arange(16)) if d == 16 else wr.se_plus_cos(40, 12)
    return X, Xs, y, spec


@pytest.mark.parametrize('d', [16, 40])
def test_factor_predict_and_dlogp_on_wide_inputs(dev, d):
    """g3_gp_factor_predict (N = 300, M = 70) and g3_gp_factor + g3_gp_dlogp (N = 257) against the oracle: logp, mean,
    variance, alpha and every gradient slot"""
    from g3py_amd import _lib
    from g3py_amd.device import compile_spec
    from oracle import g3_oracle as orc
    noise = 0.1
    N, M = 300, 70
    X, Xs, y, spec = _eval_problem(d, N, M)
    ref = wr.posterior(spec, noise, X, y, Xs)
    wr.assert_condition(ref['K'])
    Np, Mp = _lib.roundup(N), _lib.roundup(M, 128)
    K = dev.alloc(Np + 128 + Mp, Np, F64)
    W, a = dev.alloc_inverses(Np, F64), dev.alloc(1, Np, F64)
    mu, ss = dev.alloc(1, Mp, F64), dev.alloc(1, Mp, F64)
    st = dev.gp_factor_predict(compile_spec(orc.with_noise(spec, noise), d), compile_spec(spec, d), wr.upload(dev, X, F64, 3), N, d,
                               dev.upload(y), wr.upload(dev, Xs, F64, 3), M, K, W, a, mu, ss)
    assert st['info'] == 0 and st['tries'] == 0
    lp = -0.5 * N * np.log(2 * np.pi) - 0.5 * st['quad'] - st['logdet']
    assert abs(lp - ref['logp']) <= 1e-8 * max(1.0, abs(ref['logp'])), (lp, ref['logp'])
    np.testing.assert_allclose(dev.download(mu, 1, M)[0], ref['mean'], atol=1e-8, rtol=1e-8)
    np.testing.assert_allclose(np.maximum(ref['prior'] - dev.download(ss, 1, M)[0], 0), ref['variance'], atol=1e-8, rtol=1e-8)
    # factor + gradient at N = 257 (one row beyond two 128-blocks)
    N = 257
    X, _, y, spec = _eval_problem(d, N, M)
    spec_n = orc.with_noise(spec, noise)
    ref = wr.posterior(spec, noise, X, y)
    Kinv = np.linalg.inv(ref['K'])
    _, slots_ref = wr.grad_reference(spec_n, X, Kinv, ref['alpha'])
    prog = compile_spec(spec_n, d)
    gmap = dev.grad_layout(prog)
    Np = _lib.roundup(N)
    Kd = dev.alloc(Np + 128, Np, F64)
    W, a = dev.alloc_inverses(Np, F64), dev.alloc(1, Np, F64)
    Xd = wr.upload(dev, X, F64, 3)
    st = dev.gp_factor(prog, Xd, N, d, dev.upload(y), Kd, W, a)
    assert st['info'] == 0 and st['tries'] == 0
    lp = -0.5 * N * np.log(2 * np.pi) - 0.5 * st['quad'] - st['logdet']
    assert abs(lp - ref['logp']) <= 1e-8 * max(1.0, abs(ref['logp'])), (lp, ref['logp'])
    Y, Ki, al = dev.alloc(Np, Np, F64), dev.alloc(Np, Np, F64), dev.alloc(1, Np, F64)
    slots = dev.gp_dlogp(prog, gmap, Xd, N, d, Kd, W, a, Y, Ki, al)
    np.testing.assert_allclose(dev.download(al, 1, N)[0], ref['alpha'], rtol=1e-8, atol=1e-8)
    wr.assert_slots(slots, gmap, slots_ref, 1e-8, 'gp_dlogp d=%d' % d)


def test_factor_predict_fp32_at_16_columns(dev):
    """the config-5 kernels (fp32, d = 16) at N = 300 against the fp64 oracle on the fp32-rounded inputs: logp to 1e-4
    relative, the project's stated fp32 tolerance; mean as test_fp32_process_close_to_fp64 (2e-3)"""
    from g3py_amd import _lib
    from g3py_amd.device import compile_spec
    from oracle import g3_oracle as orc
    d, N, M, noise = 16, 300, 70, 0.1
    X, Xs, y, spec = _eval_problem(d, N, M)
    ref = wr.posterior(spec, noise, wr.as_seen(X, F32), wr.as_seen(y, F32), wr.as_seen(Xs, F32))
    Np, Mp = _lib.roundup(N), _lib.roundup(M, 128)
    K = dev.alloc(Np + 128 + Mp, Np, F32)
    W, a = dev.alloc_inverses(Np, F32), dev.alloc(1, Np, F32)
    mu, ss = dev.alloc(1, Mp, F32), dev.alloc(1, Mp, F32)
    before = dev.gram_path_stats()
    st = dev.gp_factor_predict(compile_spec(orc.with_noise(spec, noise), d), compile_spec(spec, d), wr.upload(dev, X, F32), N, d,
                               dev.upload(y.astype(F32)), wr.upload(dev, Xs, F32), M, K, W, a, mu, ss)
    after = dev.gram_path_stats()
    assert after['table'] > before['table'] and after['generated'] == before['generated'] and after['interpreted'] == before['interpreted']
    assert st['info'] == 0 and st['tries'] == 0
    lp = -0.5 * N * np.log(2 * np.pi) - 0.5 * st['quad'] - st['logdet']
    print('fp32 d=16 N=300: logp %.6f oracle %.6f' % (lp, ref['logp']))
    assert abs(lp - ref['logp']) <= 1e-4 * abs(ref['logp']), (lp, ref['logp'])
    np.testing.assert_allclose(dev.download(mu, 1, M)[0], ref['mean'], atol=2e-3)


def _members(d, B=4):
    """B members of 1.3 SE(top 32 columns) + noise that differ in var, rate[0], the last rate of the leaf and the noise:
    their (var, rate, noise), their programs with and without noise, and the same as template + fields"""
    from g3py_amd.device import compile_spec
    from oracle import g3_oracle as orc
    cols = wr.top(d)
    nd = len(cols)
    var = 1.3 * (1 + 0.1 * np.arange(B))
    rates = np.tile(wr.rate(nd), (B, 1))
    rates[:, 0] *= 1 + 0.15 * np.arange(B)
    rates[:, nd - 1] *= 1 - 0.1 * np.arange(B)
    noise = 0.1 * (1 + 0.2 * np.arange(B))
    specs = [('SE', var[b], rates[b], cols) for b in range(B)]
    progs_n = [compile_spec(orc.with_noise(s, noise[b]), d) for b, s in enumerate(specs)]
    progs = [compile_spec(s, d) for s in specs]
    # template = member 0; the fields are exactly the members the programs differ in: var, rate[0], the last rate of the leaf
    # (rate[15] / rate[31]) and the noise
    from g3py_amd import _lib
    leaf0 = _lib.KernelProg.leaf.offset
    offs = [leaf0 + _lib.Leaf.var.offset, leaf0 + _lib.Leaf.rate.offset, leaf0 + _lib.Leaf.rate.offset + 8 * (nd - 1),
            leaf0 + C.sizeof(_lib.Leaf) + _lib.Leaf.var.offset]
    assert nd - 1 == (15 if d == 16 else 31) and progs_n[0].leaf[1].kind == _lib.KINDS['NOISE']
    fields = np.stack([var, rates[:, 0], rates[:, nd - 1], noise], axis=1)
    f_n = (progs_n[0], np.asarray(offs, dtype=np.int32), np.ascontiguousarray(fields))
    f = (progs[0], np.asarray(offs[:3], dtype=np.int32), np.ascontiguousarray(fields[:, :3]))
    return specs, noise, progs_n, progs, f_n, f


def _chain_buffers(dv, B, N, M):
    from g3py_amd import _lib
    Np, Mp = _lib.roundup(N), _lib.roundup(M, 128)
    kstride = (Np + _lib.G3_RHS_PAD) * Np
    mats = [dv.alloc(B * (Np + _lib.G3_RHS_PAD), Np, F64) for _ in range(3)]
    return dict(Np=Np, Mp=Mp, kstride=kstride, K=mats[0], Y=mats[1], Ki=mats[2], W=dv.alloc(B * Np, _lib.G3_PAD, F64),
                a=dv.alloc(B, Np, F64), al=dv.alloc(B, Np, F64))


def _chain_factor_and_cross(dv, d, N, M, form, refs=None):
    """g3_gp_factor_batched + g3_gp_cross_batched (form 'progs') or their _fields forms for the B = 4 members; returns the
    raw results and checks each member against the oracle"""
    B = 4
    specs, noise, progs_n, progs, f_n, f = _members(d, B)
    X, Xs = wr.inputs(N, d), wr.inputs(M, d, 1)
    y = np.sin(X.sum(1) / np.sqrt(d)) + 0.1 * np.random.default_rng(N).standard_normal(N)
    buf = _chain_buffers(dv, B, N, M)
    Xd, Sd, dd = wr.upload(dv, X, F64, 3), wr.upload(dv, Xs, F64, 3), dv.upload(np.tile(y, (B, 1)))
    mu, ss, kd = (dv.alloc(B, buf['Mp'], F64, zero=True) for _ in range(3))
    if form == 'progs':
        st = dv.gp_factor_batched(progs_n, Xd, N, d, dd, buf['K'], buf['kstride'], buf['W'], buf['a'], raw=True)
        dv.gp_cross_batched(progs, Sd, M, Xd, N, d, buf['K'], buf['kstride'], buf['W'], buf['a'], mu, ss, kd)
    else:
        st = dv.gp_factor_batched_fields(*f_n, Xd, N, d, dd, buf['K'], buf['kstride'], buf['W'], buf['a'])
        dv.gp_cross_batched_fields(*f, Sd, M, Xd, N, d, buf['K'], buf['kstride'], buf['W'], buf['a'], mu, ss, kd)
    res = dict(st=st.copy(), mu=dv.download(mu, B, M), ss=dv.download(ss, B, M), kd=dv.download(kd, B, M))
    if refs is None:
        refs = [wr.posterior(specs[b], noise[b], X, y, Xs) for b in range(B)]
    for b, ref in enumerate(refs):
        wr.assert_condition(ref['K'])
        assert st[b, 5] == 0 and st[b, 3] == 0, st[b]
        lp = -0.5 * N * np.log(2 * np.pi) - 0.5 * st[b, 1] - st[b, 0]
        assert abs(lp - ref['logp']) <= 1e-8 * max(1.0, abs(ref['logp'])), (b, lp, ref['logp'])
        np.testing.assert_allclose(res['mu'][b], ref['mean'], atol=1e-8, rtol=1e-8)
        np.testing.assert_allclose(np.maximum(res['kd'][b] - res['ss'][b], 0), ref['variance'], atol=1e-8, rtol=1e-8)
        np.testing.assert_allclose(res['kd'][b], ref['prior'], atol=1e-8, rtol=1e-8)
    return res, refs, (specs, noise, progs_n, progs, f_n, f), buf, (X, Xs, y, Xd, Sd)


@pytest.mark.parametrize('d', [16, 40])
def test_chain_entry_points_on_wide_inputs(dev, d):
    """g3_gp_factor_batched, g3_gp_cross_batched, g3_gp_dlogp_batched and g3_gp_draws_batched with B = 4 members at N = 128,
    M = 40 (ldx = d + 3): every member against the oracle -- logp, mean, variance, prior diagonal, alpha, every gradient slot,
    the draws with supplied Z against loc + mu + Lp Z from the oracle's robust Cholesky -- and the _fields forms of the four
    calls, their offsets pointing at var, rate[0], rate[15] / rate[31] and the noise of the template: bit-identical"""
    from oracle import g3_oracle as orc
    N, M, B, S = 128, 40, 4, 3
    out = {}
    refs = None
    for form in ('progs', 'fields'):
        res, refs, (specs, noise, progs_n, progs, f_n, f), buf, (X, Xs, y, Xd, Sd) = _chain_factor_and_cross(dev, d, N, M, form, refs)
        gmap = dev.grad_layout(progs_n[0])
        rng = np.random.default_rng(d)
        loc, Z = 0.3 * rng.standard_normal((B, M)), rng.standard_normal((B, M, S))
        # (the gradient call overwrites nothing the draws need; the draws come first as in GaussianProcess.particles)
        if form == 'progs':
            draws, tries, fb, jit = dev.gp_draws_batched(progs, Sd, M, Xd, N, d, buf['K'], buf['kstride'], buf['W'], buf['a'], False, loc, Z)
            slots = dev.gp_dlogp_batched(progs_n, gmap, Xd, N, d, buf['K'], buf['kstride'], buf['W'], buf['a'], buf['Y'], buf['Ki'], buf['al'])
        else:
            draws, tries, fb, jit = dev.gp_draws_batched_fields(*f, Sd, M, Xd, N, d, buf['K'], buf['kstride'], buf['W'], buf['a'], False, loc, Z)
            slots = dev.gp_dlogp_batched_fields(*f_n, gmap, Xd, N, d, buf['K'], buf['kstride'], buf['W'], buf['a'], buf['Y'], buf['Ki'], buf['al'])
        res.update(draws=draws, slots=slots.copy(), alpha=dev.download(buf['al'], B, N))
        assert not tries.any() and not fb.any()
        for b, ref in enumerate(refs):
            Lp, tr, fell = orc.cholesky_robust(ref['cov'], return_info=True)
            assert tr == 0 and not fell
            want = loc[b][:, None] + ref['mean'][:, None] + Lp @ Z[b]
            np.testing.assert_allclose(draws[b], want, rtol=0, atol=1e-8 * np.abs(want).max())
            np.testing.assert_allclose(res['alpha'][b], ref['alpha'], rtol=1e-8, atol=1e-8)
            _, sref = wr.grad_reference(orc.with_noise(specs[b], noise[b]), X, np.linalg.inv(ref['K']), ref['alpha'])
            wr.assert_slots(slots[b], gmap, sref, 1e-8, 'member %d d=%d %s' % (b, d, form))
        out[form] = res
    for k in out['progs']:
        np.testing.assert_array_equal(out['progs'][k], out['fields'][k], err_msg=k)


@pytest.mark.parametrize('mode', ['coop', 'sweep'])
@pytest.mark.parametrize('d', [16, 40])
def test_chain_factor_and_cross_beyond_one_workgroup(monkeypatch, d, mode):
    """N = 300: the cooperative kernel and the lock-step sweep (the knobs of tests/test_gpu_predict_chain.py), both forms"""
    import g3py_amd as g3
    monkeypatch.setenv('G3_COOP_MIN_BATCH', '2')
    monkeypatch.setenv('G3_COOP_MAX_N', '0' if mode == 'sweep' else '1024')
    dv = g3.Device(0)
    try:
        a, refs = _chain_factor_and_cross(dv, d, 300, 40, 'progs')[:2]
        b = _chain_factor_and_cross(dv, d, 300, 40, 'fields', refs)[0]
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    finally:
        dv.close()


# ----------------------------------------------------------------------------- C. the process API at d = 16
def _params(gp, **nat):
    p = gp.params_test
    by = {v.name: v for v in gp.model.vars}
    for k, val in nat.items():
        v = by[gp.name + '_' + k]
        p[v.key] = (np.log(val) if v.positive else np.asarray(val, dtype=float)) * np.ones(v.shape)
    return p


@pytest.mark.parametrize('dtype', DTYPES)
def test_gaussian_process_at_16_columns_matches_the_oracle(dtype):
    """config 5's expression at test size: GaussianProcess with ARD SE + noise on 200 points of 16 columns.  fp64: logp,
    predict, dlogp (in the transformed space: theta * 1/2 sum G dK/dtheta), logp_chain, dlogp_chain, predict_chain and
    particles over a 5-row chain, row by row against the oracle; fp32: logp and the mean, single and chain forms, against the
    fp64 oracle on the fp32-rounded data at the tolerance of test_fp32_process_close_to_fp64 (1e-4 relative, 2e-3)"""
    import g3py_amd as g3
    from oracle import g3_oracle as orc
    N, d, M, R = 200, 16, 40, 5
    f32 = dtype == F32
    X, Xs = wr.inputs(N, d).astype(dtype), wr.inputs(M, d, 1).astype(dtype)
    y = (np.sin(wr.inputs(N, d).sum(1) / 4) + 0.1 * np.random.default_rng(16).standard_normal(N)).astype(dtype)
    gp = g3.GaussianProcess(space=Xs, location=g3.Zero(), kernel=g3.SE(X), dtype=dtype)
    gp.observed(X, y)
    assert [v.key for v in gp.model.vars] == ['GP_SE_var_log_', 'GP_SE_rate_log_', 'GP_Noise_var_log_']
    u = np.random.default_rng(5).uniform(-1, 1, (R, 3 + d))
    nat = [dict(SE_var=1.3 * (1 + 0.2 * u[r, 0]), SE_rate=wr.rate(d) * (1 + 0.2 * u[r, 3:]), Noise_var=0.1 * (1 + 0.3 * u[r, 1]))
           for r in range(R)]
    rows = [_params(gp, **p) for p in nat]
    chain = np.stack([gp.active.dict_to_array(p) for p in rows])
    X64, Xs64, y64 = X.astype(F64), Xs.astype(F64), y.astype(F64)
    refs, grads = [], []
    for p in nat:
        spec = ('SE', p['SE_var'], p['SE_rate'], None)
        ref = wr.posterior(spec, p['Noise_var'], X64, y64, Xs64)
        wr.assert_condition(ref['K'])
        refs.append(ref)
        if not f32:
            spec_n = orc.with_noise(spec, p['Noise_var'])
            _, sl = wr.grad_reference(spec_n, X64, np.linalg.inv(ref['K']), ref['alpha'])
            theta = np.concatenate([[p['SE_var']], p['SE_rate'], [p['Noise_var']]])
            # the oracle lists the slots leaf by leaf (var, rate_k of the SE leaf, then the noise variance): the model's order
            assert [(s[0], s[1]) for s in sl] == [(0, 'var')] + [(0, 'rate')] * d + [(1, 'var')]
            grads.append((theta * np.array([s[3] for s in sl]), theta * np.array([s[4] for s in sl])))
    lp_chain = np.asarray(gp.logp_chain(chain, batch=3), dtype=F64)
    pc = gp.predict_chain(chain, var=True, noise=False, batch=3)
    for r in range(R):
        ref = refs[r]
        lp, pred = float(gp.logp(rows[r])), gp.predict(rows[r], var=True, noise=False)
        if f32:
            for v in (lp, lp_chain[r]):
                assert abs(v - ref['logp']) <= 1e-4 * abs(ref['logp']), (r, v, ref['logp'])
            np.testing.assert_allclose(pred.mean, ref['mean'], atol=2e-3)
            np.testing.assert_allclose(pc['mean'][r], ref['mean'], atol=2e-3)
            continue
        for v in (lp, lp_chain[r]):
            assert abs(v - ref['logp']) <= 1e-8 * max(1.0, abs(ref['logp'])), (r, v, ref['logp'])
        for mean, var in ((pred.mean, pred.variance), (pc['mean'][r], pc['variance'][r])):
            np.testing.assert_allclose(mean, ref['mean'], rtol=1e-8, atol=1e-8)
            np.testing.assert_allclose(var, ref['variance'], rtol=1e-8, atol=1e-8)
    if f32:
        return
    dl_chain = gp.dlogp_chain(chain, batch=3)
    for r in range(R):
        want, scale = grads[r]
        for got in (gp.dlogp(chain[r], array=True), dl_chain[r]):
            assert np.all(np.abs(got - want) < 1e-8 * scale), (r, np.abs(got - want) / scale)
    Z = np.random.default_rng(6).standard_normal((R, M, 2))
    got = gp.particles(chain, samples=2, rand=Z, batch=3)
    want = np.concatenate([refs[r]['mean'][:, None] + orc.cholesky_robust(refs[r]['cov']) @ Z[r] for r in range(R)], axis=1)
    assert got.shape == (M, 2 * R)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-8 * np.abs(want).max())
