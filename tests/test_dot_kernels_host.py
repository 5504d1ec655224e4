"""Dot-product kernel family (LIN, POL, NN, BW, VAR, NIL -- g3py/processes/hypers/kernels.py:82-94, 293-357;
metrics.py:25-27, 54-56, 111-136) without a GPU: classes, names, defaults, lowering to g3_kernel_prog, chain-row packing,
gradient slot layout, cross-compilation of the generated kernels for gfx950, program validation, and the NumPy reference
of the GPU tests checked against finite differences."""
import ctypes as C
import inspect

import numpy as np
import pytest

import g3py_amd as g3
from g3py_amd import _lib
from g3py_amd.device import compile_spec, compile_spec_rows

from dot_reference import dot_zoo, kernel_cov_ext, kernel_cov_grads_ext, nn_argument, zoo_inputs

K_DOT, K_NN, K_BW, K_VAR = 11, 12, 13, 14


def _xy(n=40, d=3, seed=0):
    rng = np.random.default_rng(seed)
    X = 1.5 * rng.standard_normal((n, d))
    y = np.sin(X.sum(1)) + 0.3 * rng.standard_normal(n) + 0.7
    return X, y


# ------------------------------------------------------------------ 1. classes, signatures, names, defaults
def test_classes_signatures_names_and_defaults():
    def sig(cls):
        return [(p.name, p.default) for p in list(inspect.signature(cls.__init__).parameters.values())[1:]]
    assert sig(g3.KernelDot) == [('x', None), ('name', None), ('metric', g3.ARD_Dot), ('var', None)]
    assert sig(g3.LIN) == [('x', None), ('name', None), ('metric', g3.ARD_DotBias), ('var', 1)]
    assert sig(g3.POL) == [('x', None), ('p', 2), ('name', None), ('metric', g3.ARD_DotBias), ('var', 1)]
    assert sig(g3.NN) == [('x', None), ('name', None), ('metric', g3.ARD_DotBias), ('var', None)]
    assert sig(g3.BW) == [('x', None), ('name', None), ('metric', g3.Minimum), ('var', None)]
    assert sig(g3.VAR) == [('x', None), ('name', None), ('metric', g3.One), ('var', None)]
    assert sig(g3.NIL) == [('x', None), ('name', None), ('metric', g3.One), ('var', 1)]
    import g3py_amd.processes.hypers.kernels as hk
    import g3py_amd.processes.hypers.metrics as hm
    for n in ('KernelDot', 'LIN', 'POL', 'NN', 'BW', 'VAR', 'NIL'):
        assert getattr(hk, n) is getattr(g3, n)
    for n in ('One', 'Minimum', 'ARD_Dot', 'ARD_DotBias'):
        assert getattr(hm, n) is getattr(g3, n)
    assert g3.POL(None, 3).p == 3 and g3.POL().p == 2
    for bad in (2.5, 0, -1, 9, '2', None, True):
        with pytest.raises(g3.G3Error, match='integer'):
            g3.POL(None, bad)

    X, y = _xy()
    free = {}
    for cls in (g3.KernelDot, g3.LIN, g3.POL, g3.NN, g3.BW, g3.VAR, g3.NIL):
        gp = g3.GP(space=X, location=g3.Zero(), kernel=cls(X))
        free[cls.__name__] = [v.key for v in gp.model.vars]
    assert free['KernelDot'] == ['GP_KernelDot_var_log_', 'GP_KernelDot_rate_log_', 'GP_Noise_var_log_']
    assert free['LIN'] == ['GP_LIN_rate_log_', 'GP_LIN_bias_log_', 'GP_Noise_var_log_']          # var = 1 is a constant
    assert free['POL'] == ['GP_POL_rate_log_', 'GP_POL_bias_log_', 'GP_Noise_var_log_']
    assert free['NN'] == ['GP_NN_var_log_', 'GP_NN_rate_log_', 'GP_NN_bias_log_', 'GP_Noise_var_log_']
    assert free['BW'] == ['GP_BW_var_log_', 'GP_Noise_var_log_']
    assert free['VAR'] == ['GP_VAR_var_log_', 'GP_Noise_var_log_']
    assert free['NIL'] == ['GP_Noise_var_log_']

    # defaults: metrics.py:115-116 and :134-136, a free var gets y.var()
    gp = g3.GP(space=X, location=g3.Zero(), kernel=g3.KernelDot(X, name='D') + g3.NN(X))
    gp.observed(X, y)
    dflt = gp.params_default
    ax, ay = np.abs(X), np.abs(y)
    np.testing.assert_allclose(np.exp(dflt['GP_D_rate_log_']), 1 / (np.sqrt(ax).mean(axis=0) / ay.mean(axis=0)), rtol=1e-14)
    np.testing.assert_allclose(np.exp(dflt['GP_NN_bias_log_']), ay.mean() / ax.mean(), rtol=1e-14)
    np.testing.assert_allclose(np.exp(dflt['GP_NN_rate_log_']), np.sqrt(ay).mean(axis=0) / ax.mean(axis=0), rtol=1e-14)
    np.testing.assert_allclose(np.exp(dflt['GP_NN_var_log_']), y.var(), rtol=1e-14)
    np.testing.assert_allclose(np.exp(dflt['GP_D_var_log_']), y.var(), rtol=1e-14)
    # column subsets: the defaults see the selected columns only
    gp = g3.GP(space=X, location=g3.Zero(), kernel=g3.LIN([0, 2]))
    gp.observed(X, y)
    np.testing.assert_allclose(np.exp(gp.params_default['GP_LIN_rate_log_']),
                               np.sqrt(ay).mean() / ax[:, [0, 2]].mean(axis=0), rtol=1e-14)


# ------------------------------------------------------------------ 2. lowering
def _leaf(prog, i):
    L = prog.leaf[i]
    nd = L.ndims
    return dict(kind=L.kind, nd=nd, dims=list(L.dims[:nd]), var=L.var, alpha=L.alpha, rate=list(L.rate[:nd]), p=L.freq[0])


def test_compile_spec_lowers_every_class_and_the_mixed_trees():
    X, _ = _xy(d=3)
    r = np.array([0.7, 1.1, 1.3])
    v = {'LIN_rate': r, 'LIN_bias': 0.5, 'POL_rate': r, 'POL_bias': 0.4, 'NN_var': 1.4, 'NN_rate': r, 'NN_bias': 0.6,
         'BW_var': 0.8, 'VAR_var': 0.3, 'KernelDot_var': 1.2, 'KernelDot_rate': r, 'SE_var': 1.0, 'SE_rate': r,
         'OU_var': 1.0, 'OU_rate': r}

    def low(k):
        k.check_hypers('')
        return compile_spec(k.spec(v, 3), 3)
    with g3.Model('m'):
        p = low(g3.KernelDot(X))
        assert p.nleaf == 1 and _leaf(p, 0) == dict(kind=K_DOT, nd=3, dims=[0, 1, 2], var=1.2, alpha=0.0, rate=list(r), p=1.0)
    with g3.Model('m'):
        assert _leaf(low(g3.LIN(X)), 0) == dict(kind=K_DOT, nd=3, dims=[0, 1, 2], var=1.0, alpha=0.5, rate=list(r), p=1.0)
    with g3.Model('m'):
        assert _leaf(low(g3.POL(X, 3)), 0) == dict(kind=K_DOT, nd=3, dims=[0, 1, 2], var=1.0, alpha=0.4, rate=list(r), p=3.0)
    with g3.Model('m'):
        lf = _leaf(low(g3.NN(X)), 0)
        assert (lf['kind'], lf['var'], lf['alpha'], lf['rate']) == (K_NN, 1.4, 0.6, list(r))
    with g3.Model('m'):
        lf = _leaf(low(g3.BW(X)), 0)
        assert (lf['kind'], lf['var'], lf['dims']) == (K_BW, 0.8, [0, 1, 2])
    with g3.Model('m'):
        lf = _leaf(low(g3.VAR(X)), 0)
        assert (lf['kind'], lf['var']) == (K_VAR, 0.3)
    with g3.Model('m'):
        lf = _leaf(low(g3.NIL(X)), 0)
        assert (lf['kind'], lf['var']) == (K_VAR, 0.0)           # NIL: a VAR leaf with var = 0
    # mixed trees
    with g3.Model('m'):
        p = low(g3.LIN(X) + g3.SE(X))
        assert (p.nleaf, p.nprod, p.shift) == (2, 2, 0.0) and [p.leaf[i].kind for i in range(2)] == [K_DOT, 0]
    with g3.Model('m'):
        p = low(g3.POL(X) * g3.SE(X))
        assert (p.nleaf, p.nprod) == (2, 1) and p.prod[0].nfac == 2 and p.leaf[0].freq[0] == 2.0
    with g3.Model('m'):
        p = low(2 * g3.NN(X) + 0.1)
        assert (p.nleaf, p.nprod, p.shift, p.prod[0].coef) == (1, 1, 0.1, 2.0) and p.leaf[0].kind == K_NN
    with g3.Model('m'):
        p = low(g3.BW([0, 2]) + g3.VAR(X))
        assert [p.leaf[i].kind for i in range(2)] == [K_BW, K_VAR] and _leaf(p, 0)['dims'] == [0, 2]
    with g3.Model('m'):
        p = low(g3.NIL(X) + g3.OU(X))
        assert [p.leaf[i].kind for i in range(2)] == [K_VAR, 1] and p.leaf[0].var == 0.0
    # the exponent is checked where programs are built, too
    for bad in (2.5, 0, 9):
        with pytest.raises(g3.G3Error, match='exponent'):
            compile_spec(('DOT', 1.0, r, 0.5, bad, None), 3)
    # a dot kernel on a metric it has no formula for
    with g3.Model('m'):
        k = g3.POL(X, 2, metric=g3.Minimum)
        k.check_hypers('')
        with pytest.raises(g3.G3Error, match='ARD_Dot'):
            k.spec(v, 3)


def test_chain_rows_pack_bias_rate_var_and_reexpand_to_row_by_row_programs():
    """compile_spec_rows on a chain with varying bias / rate / var: exactly those fields (never the exponent), and the
    template with the fields written back equals the row-by-row program byte for byte"""
    rng = np.random.default_rng(3)
    X, y = _xy(25, 3, 3)
    for kernel in (g3.LIN(X) + g3.SE(X), g3.POL(X, 3) * g3.OU(X) + g3.VAR(X), 2 * g3.NN(X) + 0.1, g3.BW(np.abs(X)) + g3.NIL(X)):
        gp = g3.GP(space=X, location=g3.Bias(), kernel=kernel)
        gp.observed(X, y)
        B, d = 6, 3
        base = gp.active.dict_to_array(gp.params_default)
        chain = base[None, :] + 0.3 * rng.standard_normal((B, gp.active.ndim))
        values_b, _ = gp._values_rows(chain)
        tmpl, offs, fields = compile_spec_rows(gp.f_kernel_noise.spec(values_b, d),
                                               gp.f_kernel_noise.spec(gp._values_row(values_b, 0), d), d, B)
        nkern = sum(v.size for v in gp.model.vars if 'Bias_' not in v.name)
        assert fields.shape == (B, len(offs)) and len(set(offs.tolist())) == len(offs) == nkern
        leaf0, lsz = _lib.KernelProg.leaf.offset, C.sizeof(_lib.Leaf)
        for o in offs:                         # no field names the exponent of a DOT leaf
            l, inner = divmod(int(o) - leaf0, lsz)
            assert not (tmpl.leaf[l].kind == K_DOT and inner == _lib.Leaf.freq.offset)
        for j in range(B):
            gp._values_memo = None
            values, _ = gp._values(gp.active.array_to_dict(chain[j]))
            want = compile_spec(gp.f_kernel_noise.spec(values, d), d)
            got = _lib.KernelProg.from_buffer_copy(bytes(tmpl))
            raw = (C.c_char * C.sizeof(got)).from_buffer(got)
            for o, val in zip(offs, fields[j]):
                raw[o:o + 8] = np.float64(val).tobytes()
            assert bytes(got) == bytes(want), j


# ------------------------------------------------------------------ 3. gradient slots
def test_grad_layout_slots_of_the_new_kinds():
    lib = _lib.load()
    d = 3
    r = np.ones(d)
    spec = ('sum', ('sum', ('sum', ('DOT', 1.0, r, 0.5, 2, None), ('NN', 1.0, r[:2], 0.5, np.array([0, 2]))),
                    ('sum', ('BW', 1.0, None), ('VAR', 1.0))), ('SE', 1.0, r, None))
    prog = compile_spec(spec, d)
    m = _lib.GradMap()
    assert lib.g3_grad_layout(C.byref(prog), C.byref(m)) == 0
    # per leaf: var, [alpha = bias], [rate...]; the exponent has no slot
    assert list(m.var[:5]) == [0, 5, 9, 10, 11]
    assert list(m.alpha[:5]) == [1, 6, -1, -1, -1]
    assert list(m.rate[:5]) == [2, 7, -1, -1, 12]
    assert list(m.freq[:5]) == [-1] * 5
    assert m.nslots == 15


# ------------------------------------------------------------------ 4. generated kernels cross-compile for gfx950
def _jit(fn, spec, d, dt):
    prog = compile_spec(spec, d)
    cb, log = C.c_int64(0), C.create_string_buffer(8000)
    rc = fn(C.byref(prog), d, dt, C.byref(cb), log, 8000)
    if rc == -1:
        pytest.skip('libhiprtc is not available on this host')
    return rc, cb.value, log.value.decode()[:3000]


@pytest.mark.parametrize('which', ['gram', 'grad'])
def test_generated_kernels_compile_for_every_dot_expression(which):
    lib = _lib.load()
    fn = lib.g3_gram_jit_check if which == 'gram' else lib.g3_grad_jit_check
    n = 0
    for d in (1, 3, 8):
        for name, spec in dot_zoo(d).items():
            for dt in ((0, 1) if name in ('POL*SE', 'NN') else (0,)):
                rc, nbytes, log = _jit(fn, spec, d, dt)
                assert rc == 0 and nbytes > 1000, (which, d, name, dt, rc, log)
                n += 1
    assert n == 3 * (len(dot_zoo(3)) + 2)


# ------------------------------------------------------------------ 5. the reference checks itself
@pytest.mark.parametrize('name', sorted(dot_zoo(3)))
def test_reference_gradients_match_finite_differences(name):
    """kernel_cov_grads_ext against central differences of kernel_cov_ext, fp64: step h = 1e-6 max(1, |theta|), agreement
    1e-7 of max|dK| (truncation O(h^2) and rounding eps / h are both ~1e-10 at that step)"""
    d, n = 3, 30
    spec = dot_zoo(d)[name]
    X = zoo_inputs(spec, n, d, 7)
    K, grads = kernel_cov_grads_ext(spec, X)
    np.testing.assert_allclose(K, kernel_cov_ext(spec, X), rtol=1e-14, atol=1e-15)

    # every leaf parameter, addressed by (leaf, pname, k): rebuild the tree with one value moved
    field = {'DOT': dict(var=1, rate=2, alpha=3), 'NN': dict(var=1, rate=2, alpha=3), 'BW': dict(var=1), 'VAR': dict(var=1),
             'SE': dict(var=1, rate=2), 'OU': dict(var=1, rate=2), 'NOISE': dict(var=1)}

    def moved(s, target, delta, counter):
        if s[0] in ('sum', 'prod'):
            a = moved(s[1], target, delta, counter)
            return (s[0], a, moved(s[2], target, delta, counter))
        if s[0] in ('scale', 'shift'):
            return (s[0], s[1], moved(s[2], target, delta, counter))
        me = counter[0]
        counter[0] += 1
        if me != target[0]:
            return s
        idx = field[s[0]][target[1]]
        val = np.array(s[idx], dtype=float)
        if target[2] is None:
            val = float(val) + delta
        else:
            val = val.copy()
            val[target[2]] += delta
        return s[:idx] + (val,) + s[idx + 1:]

    def value(s, target, counter):
        if s[0] in ('sum', 'prod', 'scale', 'shift'):
            out = None
            for c in s[1:]:
                if isinstance(c, tuple):
                    got = value(c, target, counter)
                    out = got if got is not None else out
            return out
        me = counter[0]
        counter[0] += 1
        if me != target[0]:
            return None
        val = np.asarray(s[field[s[0]][target[1]]], dtype=float)
        return float(val if target[2] is None else val[target[2]])

    for leaf, pname, k, dK in grads:
        theta = value(spec, (leaf, pname, k), [0])
        h = 1e-6 * max(1.0, abs(theta))
        up = kernel_cov_ext(moved(spec, (leaf, pname, k), +h, [0]), X)
        dn = kernel_cov_ext(moved(spec, (leaf, pname, k), -h, [0]), X)
        fd = (up - dn) / (2 * h)
        assert np.abs(fd - dK).max() <= 1e-7 * max(np.abs(dK).max(), 1e-300), (name, leaf, pname, k)


def test_nn_argument_stays_within_a_quarter():
    for d in (1, 3, 8):
        spec = dot_zoo(d)['NN']
        s = nn_argument(spec, zoo_inputs(spec, 200, d, d))
        assert np.abs(s).max() <= 0.25 + 1e-15


# ------------------------------------------------------------------ 6. validation
def test_program_validation_accepts_the_new_kinds_and_checks_the_exponent():
    lib = _lib.load()
    d = 2
    r = np.ones(d)

    def check(prog):
        cb, log = C.c_int64(0), C.create_string_buffer(4000)
        rc = lib.g3_gram_jit_check(C.byref(prog), d, 0, C.byref(cb), log, 4000)
        if rc == -1:
            pytest.skip('libhiprtc is not available on this host')
        return rc
    for spec in (('DOT', 1.0, r, 0.5, 8, None), ('NN', 1.0, r, 0.5, None), ('BW', 1.0, None), ('VAR', 1.0)):
        assert check(compile_spec(spec, d)) == 0
    prog = compile_spec(('VAR', 1.0), d)
    prog.leaf[0].kind = K_VAR + 1                      # the first kind number past the last one
    assert check(prog) == -2
    for bad in (0.0, 2.5, 9.0, -1.0, float('nan'), 1e30):
        prog = compile_spec(('DOT', 1.0, r, 0.5, 2, None), d)
        prog.leaf[0].freq[0] = bad
        assert check(prog) == -2, bad
    assert lib.g3_version() >= 101
