"""CPU tests of the reverse mode through the Cholesky factor: the two new symbols and their bindings, the signatures of
CholeskyRobust.grad / factor_vjp / Device.potrf_vjp / Device.gram_vjp, the routing of the device's parameter sums to the
model's variables, and -- in NumPy, on the padded operands the device uses -- the formulation g3_potrf_vjp implements against
oracle.cholesky_grad (tests/vjp_reference.py).  No device call is made here."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import vjp_reference as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    from g3py_amd import _lib
    return _lib.load()


def _prototype(name):
    """the parameter list of `name` in include/g3hip.h (comments removed), as a list of declarations"""
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'g3hip.h')).read(), flags=re.S)
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, header)
    assert m, '%s is not declared in include/g3hip.h' % name
    return [' '.join(a.split()) for a in m.group(1).split(',')]


def test_symbols_in_library_header_and_signature_table(lib):
    from g3py_amd import _lib
    for name in ('g3_potrf_vjp', 'g3_gram_vjp'):
        assert hasattr(lib, name)
        assert name in _lib.EXPORTS
        _prototype(name)
    assert lib.g3_version() >= 103


def test_argument_types_follow_the_header(lib):
    """every parameter of the two prototypes against the ctypes table: pointers to the two structs by their type, other
    pointers as void*, int64_t / int / g3_dtype by width"""
    from g3py_amd import _lib

    def ctype(decl):
        if 'g3_kernel_prog*' in decl:
            return C.POINTER(_lib.KernelProg)
        if 'g3_grad_map*' in decl:
            return C.POINTER(_lib.GradMap)
        if 'double*' in decl:
            return C.POINTER(C.c_double)
        if '*' in decl:
            return C.c_void_p
        if decl.startswith('int64_t'):
            return C.c_int64
        assert decl.startswith('int ') or decl.startswith('g3_dtype '), decl
        return C.c_int
    for name in ('g3_potrf_vjp', 'g3_gram_vjp'):
        f = getattr(lib, name)
        assert list(f.argtypes) == [ctype(d) for d in _prototype(name)], name
        assert f.restype is C.c_int
    assert len(lib.g3_potrf_vjp.argtypes) == 9 and len(lib.g3_gram_vjp.argtypes) == 11


def test_null_context(lib):
    assert lib.g3_potrf_vjp(None, None, 0, None, 0, 0, 0, None, 0) == -1
    assert lib.g3_gram_vjp(None, None, None, None, 0, 0, 0, 0, None, 0, None) == -1


def test_signatures():
    import g3py_amd as g3
    from g3py_amd.libs.tensors import CholeskyRobust
    assert list(inspect.signature(CholeskyRobust.grad).parameters) == ['self', 'inputs', 'gradients']
    sig = inspect.signature(g3.GaussianProcess.factor_vjp)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ('params', inspect.Parameter.empty), ('Lbar', inspect.Parameter.empty), ('inputs', None), ('outputs', None)]
    # GP and TP (and their warped forms) share the one definition
    for cls in (g3.WarpedGaussianProcess, g3.StudentTProcess, g3.WarpedStudentTProcess):
        assert cls.factor_vjp is g3.GaussianProcess.factor_vjp
    assert list(inspect.signature(g3.Device.potrf_vjp).parameters) == ['self', 'L', 'Lbar', 'n', 'Kbar']
    assert list(inspect.signature(g3.Device.gram_vjp).parameters) == ['self', 'prog', 'gmap', 'X', 'N', 'd', 'Kbar']


def test_factor_vjp_is_refused_on_a_distributed_process_and_without_observations():
    import g3py_amd as g3
    p = vr.problem(16)
    gp = g3.GaussianProcess(space=p['X'], location=g3.Zero(), kernel=g3.SE(p['X']))
    with pytest.raises(g3.G3Error, match='factor_vjp needs observations'):
        gp.factor_vjp(None, np.zeros((16, 16)))
    gp.observed(p['X'], p['y'])
    gp.distribute(None, 0, 1)
    with pytest.raises(g3.G3Error, match='factor_vjp runs on one GPU'):
        gp.factor_vjp(None, np.zeros((16, 16)))


def test_kernel_slots_route_the_sums_to_the_variables(lib):
    """the kernel-hyper part of the chain rule on its own: slot k of the standard layout lands on the variable that fed it,
    for one row of sums and for a chain block, and nothing else moves"""
    import g3py_amd as g3
    from g3py_amd import _lib
    p = vr.problem(16)
    gp = g3.GaussianProcess(space=p['X'], location=g3.Bias(), kernel=g3.SE(p['X']) + g3.RQ(p['X']))
    values = {v.name: np.ones(v.shape) for v in gp.model.vars}
    prog = gp._prog(gp.f_kernel_noise, values, 2)
    gmap = _lib.GradMap()
    assert lib.g3_grad_layout(C.byref(prog), C.byref(gmap)) == 0
    # standard layout: SE var, rate x 2 | RQ var, alpha, rate x 2 | NOISE var
    assert gmap.nslots == 8
    want = {'GP_SE_var': [0], 'GP_SE_rate': [1, 2], 'GP_RQ_var': [3], 'GP_RQ_alpha': [4], 'GP_RQ_rate': [5, 6],
            'GP_Noise_var': [7], 'GP_Bias_Bias': []}
    assert set(want) == set(values)
    for lead in ((), (3,)):
        slots = 1.0 + np.arange(8.0) + (10.0 * np.arange(3.0)[:, None] if lead else 0.0)
        nat = {v.name: np.zeros(lead + tuple(v.shape)) for v in gp.model.vars}
        gp._kernel_slots(nat, prog, gmap, slots, 2)
        for name, idx in want.items():
            expect = slots[..., idx].reshape(nat[name].shape) if idx else np.zeros(nat[name].shape)
            assert np.array_equal(nat[name], expect), name


def _device_formulation(L, Lbar, dtype=np.float64):
    """g3_potrf_vjp's five steps restated with NumPy products on the padded row-major operands (include/g3hip.h):
    Lt / Lbt transposed lower triangles with identity / zero padding, Y = L^-T, P = Lt Lbt^T lower -> Phi + scrub,
    Tt = Y P^T, C = Y Tt^T + Tt Y^T lower, Kbar = Phi(C)"""
    n = len(L)
    npad = (n + 127) // 128 * 128
    Lp = np.eye(npad, dtype=dtype)
    Lp[:n, :n] = np.tril(L)
    Bp = np.zeros((npad, npad), dtype=dtype)
    Bp[:n, :n] = np.where(np.tril(np.ones((n, n), bool)), Lbar, 0.0)           # nothing above the diagonal is read
    Lt, Lbt = Lp.T.copy(), Bp.T.copy()
    Y = np.linalg.inv(Lp).T.astype(dtype)
    P = np.tril(Lt.dot(Lbt.T))
    P = np.where(np.isnan(P), 0.0, np.where(np.isinf(P), 1e10, P)).astype(dtype)
    P = vr.phi(P)
    Tt = Y.dot(P.T)
    Cm = np.tril(Y.dot(Tt.T) + Tt.dot(Y.T))
    return vr.phi(Cm)[:n, :n]


@pytest.mark.parametrize('n', [1, 97, 200])
def test_formulation_matches_the_oracle(n):
    p = vr.problem(n)
    ref = vr.reference(p['L'], p['Lbar'])
    got = _device_formulation(p['L'], vr.with_nan_above(p['Lbar']))
    err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    print('formulation n=%d: rel Frobenius error %.2e' % (n, err))
    assert err <= 1e-12
    assert np.all(np.triu(got, 1) == 0.0)


def test_reference_satisfies_the_adjoint_identity():
    """<tril Lbar, dL> = <Kbar, tril dK> with the exact forward-mode dL: the helper's two routes agree with each other"""
    p = vr.problem(97)
    Kbar = vr.reference(p['L'], p['Lbar'])
    dL = vr.forward_mode(p['L'], p['dK'])
    assert np.all(np.triu(dL, 1) == 0.0)
    lhs, rhs = np.sum(np.tril(p['Lbar']) * dL), np.sum(Kbar * np.tril(p['dK']))
    assert abs(lhs - rhs) <= 1e-11 * abs(rhs)
    # and dL is the derivative of the factor: a central difference of np.linalg.cholesky, to what differences give
    h = 1e-6
    fd = (np.linalg.cholesky(p['K'] + h * p['dK']) - np.linalg.cholesky(p['K'] - h * p['dK'])) / (2 * h)
    assert np.linalg.norm(fd - dL) <= 1e-6 * np.linalg.norm(dL)


def test_fp32_gap_is_a_float32_quantity():
    gap, ref64, L32, B32 = vr.fp32_gap(128)
    print('fp32_gap(128) = %.2e' % gap)
    assert L32.dtype == np.float32 and B32.dtype == np.float32 and ref64.dtype == np.float64
    assert 1e-9 < gap < 1e-5           # float32 rounding, neither float64 nor a blunder
