"""CPU tests of appending observations: the block formulas of tests/append_reference.py against SciPy's factor of the whole
matrix and against the oracle's GP on the concatenated data, the new header and its signature table, the signature of
observe_more, the capacity rule, and the plan arithmetic of g3_host.h as a stand-alone program under the sanitizers.  No device
call is made here.

Bound of the formula tests: 1e-10.  The covariances have kappa ~ 1e2 (append_reference.problem), so two orders of
summation of the same factor differ by ~1e-14; nothing here is anywhere near the bound."""
import ctypes
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.linalg

import append_reference as ar
from oracle import g3_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'g3hip_online.h')
CASES = [(1, 1), (100, 20), (100, 28), (100, 29), (128, 1), (128, 128), (300, 1), (300, 300), (120, 30)]


@pytest.fixture(scope='module')
def lib():
    from g3py_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------- the block formulas
@pytest.mark.parametrize('N0,m', CASES)
def test_append_equals_the_factor_of_the_whole_matrix(N0, m):
    N1 = N0 + m
    X, y, _ = ar.problem(N1)
    K1 = ar.covariance(N1)
    L0, a0, _, _ = ar.factor(K1[:N0, :N0], y[:N0])
    n0, Np1, r = ar.plan(N0, N1)
    # what the precondition does not cover must not matter: rows from n0 on, and the strict upper triangle
    L0, a0 = L0.copy(), a0.copy()
    L0[n0:], a0[n0:] = np.nan, np.nan
    L0[np.triu_indices_from(L0, 1)] = np.nan
    L1, a1, logdet, quad = ar.append_factor(K1, L0, a0, y, N0)
    Lr, ar_, logdet_r, quad_r = ar.reference(N1)
    assert L1.shape == (Np1, Np1) and np.isfinite(np.tril(L1)).all()
    np.testing.assert_allclose(np.tril(L1), np.tril(Lr), rtol=0, atol=1e-10 * np.abs(Lr).max())
    np.testing.assert_allclose(a1, ar_, rtol=0, atol=1e-10 * np.abs(ar_).max())
    assert abs(logdet - logdet_r) <= 1e-10 * abs(logdet_r) and abs(quad - quad_r) <= 1e-10 * quad_r
    full = scipy.linalg.cholesky(K1, lower=True)
    np.testing.assert_allclose(np.tril(L1)[:N1, :N1], full, rtol=0, atol=1e-10 * np.abs(full).max())
    np.testing.assert_array_equal(np.tril(L1)[N1:, N1:], np.eye(Np1 - N1))


def test_append_equals_the_oracle_on_the_concatenated_data():
    N0, m, M = 100, 29, 17
    N1 = N0 + m
    X, y, Xs = ar.problem(N1, M)
    gp = orc.GP(ar.SE, ar.NOISE)
    K1 = ar.covariance(N1)
    L0, a0, _, _ = ar.factor(K1[:N0, :N0], y[:N0])
    L1, a1, logdet, quad = ar.append_factor(K1, L0, a0, y, N0)
    logp = -0.5 * N1 * math.log(2 * math.pi) - logdet - 0.5 * quad
    want = gp.logp(X, y)
    assert abs(logp - want) <= 1e-10 * abs(want)
    Kx = orc.tt_to_num(orc.kernel_cov(ar.SE, Xs, X))
    V0, _, _ = ar.cross(Kx[:, :N0], L0, a0, N0)
    V, mu, ss = ar.append_cross(V0, Kx, L1, a1, N0)
    Vr, mur, ssr = ar.cross(Kx, L1, a1, N1)
    np.testing.assert_allclose(V, Vr, rtol=0, atol=1e-10 * np.abs(Vr).max())
    np.testing.assert_allclose(mu, gp.mean(Xs, X, y), rtol=0, atol=1e-10 * np.abs(mur).max())
    prior = np.diag(orc.kernel_cov(ar.SE, Xs))
    np.testing.assert_allclose(prior - ss, gp.variance(Xs, X, y), rtol=1e-9, atol=0)


def test_thirty_single_appends_equal_one_append_of_thirty():
    N0, m = 120, 30
    X, y, _ = ar.problem(N0 + m)
    K = ar.covariance(N0 + m)
    L, a, _, _ = ar.factor(K[:N0, :N0], y[:N0])
    for n in range(N0, N0 + m):
        L, a, logdet, quad = ar.append_factor(K[:n + 1, :n + 1], L, a, y, n)
    L0, a0, _, _ = ar.factor(K[:N0, :N0], y[:N0])
    Lb, ab, logdet_b, quad_b = ar.append_factor(K, L0, a0, y, N0)
    np.testing.assert_allclose(np.tril(L), np.tril(Lb), rtol=0, atol=1e-10 * np.abs(Lb).max())
    np.testing.assert_allclose(a, ab, rtol=0, atol=1e-10 * np.abs(ab).max())
    assert abs(logdet - logdet_b) <= 1e-10 * abs(logdet_b) and abs(quad - quad_b) <= 1e-10 * quad_b


# ---------------------------------------------------------------------------------------------- header and table
def _declared():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(g3_[a-z0-9_]+)\s*\(', src)))


def test_header_symbols_exported_and_table_equals_header(lib):
    from g3py_amd import _lib
    names = _declared()
    assert names == ['g3_gp_append', 'g3_gp_cross_append']
    for n in names:
        assert hasattr(lib, n), 'libg3hip.so does not export ' + n
        assert getattr(lib, n).argtypes is not None and getattr(lib, n).restype is ctypes.c_int
    assert sorted(_lib.EXPORTS_ONLINE) == names, 'ctypes signature table and header disagree'
    assert not set(_lib.EXPORTS_ONLINE) & set(_lib.EXPORTS)
    assert lib.g3_version() >= 106
    # the declarations live in the new header alone
    main = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'g3hip.h')).read(), flags=re.S)
    assert 'append' not in main


def test_header_compiles_as_plain_c(tmp_path):
    src = tmp_path / 'h.c'
    src.write_text('#include "g3hip_online.h"\nint main(void){return G3_OK;}\n')
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), '-c', str(src),
                           '-o', str(tmp_path / 'h.o')])


def test_null_context_is_refused(lib):
    assert lib.g3_gp_append(None, None, None, 0, 0, 0, 0, None, 0, None, 0, None, None, None) == -1
    assert lib.g3_gp_cross_append(None, None, None, 0, 0, None, 0, 0, 0, 0, None, 0, None, None, 0, None, 0, None, None) == -1


def test_signatures():
    import g3py_amd as g3
    sig = inspect.signature(g3.GaussianProcess.observe_more)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ('inputs', inspect.Parameter.empty), ('outputs', inspect.Parameter.empty), ('params', None)]
    from g3py_amd.processes.elliptical import EllipticalProcess
    from g3py_amd.processes.transport import TransportProcess
    for cls in (g3.GaussianProcess, g3.WarpedGaussianProcess, g3.StudentTProcess):
        assert cls.observe_more is EllipticalProcess.observe_more
    assert not hasattr(TransportProcess, 'observe_more')
    assert hasattr(g3.Device, 'gp_append') and hasattr(g3.Device, 'gp_cross_append')


def test_observe_more_without_a_gpu_extends_the_data():
    """with no factor cached nothing touches the device: the observations, their mirrors and the counters are the host's"""
    import g3py_amd as g3
    x = np.linspace(0, 1, 8)
    gp = g3.GaussianProcess(space=x[:2, None], location=g3.Zero(), kernel=g3.SE(x[:, None]))
    assert gp.append_stats == dict(appended=0, cross_appended=0, refit=0)
    gp.observe_more(x[:5], np.sin(x[:5]))                 # nothing observed yet: this is observed()
    assert gp.is_observed and gp.inputs.shape == (5, 1)
    gp.observe_more(x[5:], np.sin(x[5:]))
    fresh = g3.GaussianProcess(space=x[:2, None], location=g3.Zero(), kernel=g3.SE(x[:, None]))
    fresh.observed(x, np.sin(x))
    for name in ('inputs', 'outputs', 'index', 'order'):
        np.testing.assert_array_equal(getattr(gp, name), getattr(fresh, name), err_msg=name)
    assert gp.append_stats == dict(appended=0, cross_appended=0, refit=2) and gp._cache is None
    with pytest.raises(g3.G3Error):
        gp.observe_more(x[:3], np.sin(x[:2]))
    with pytest.raises(g3.G3Error):
        gp.observe_more(np.zeros((2, 2)), np.zeros(2))


# ---------------------------------------------------------------------------------------------- capacity
def test_capacity_rule():
    from g3py_amd import _lib
    for have in range(128, 20000, 128 * 5):
        for need in range(1, have + 3000, 61):
            cap = _lib.append_capacity(have, need)
            assert cap == ar.capacity(have, need) and cap >= need and cap >= have
            if need <= have:
                assert cap == have
            else:
                assert cap % 128 == 0 and 2 * cap >= 3 * have
    cap, grown = 128, 0
    for n in range(129, 32769, 128):
        nxt = _lib.append_capacity(cap, n)
        grown += nxt != cap
        cap = nxt
    assert grown <= math.ceil(math.log(32768 / 128, 1.5)) + 1


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_plan_arithmetic_under_asan_ubsan(tmp_path):
    """g3h_append_plan, g3h_args_append and g3h_append_capacity (g3_host.h: plain C++) as a stand-alone program under
    g++ -fsanitize=address,undefined: tests/host_asan/append_plan.cpp"""
    exe = str(tmp_path / 'append_plan')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'g3py_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'host_asan', 'append_plan.cpp'), '-o', exe])
    env = dict(os.environ)
    env.pop('LD_PRELOAD', None)            # ASan must come first in the link order of the test binary
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'append_plan ok' in r.stdout
