"""The inputs of tests/golden/host_rows.npz and its reader.  TEST INFRASTRUCTURE ONLY.

The fixture records the host-side formulas of g3py_amd/processes/ as they were at commit a6ec925, the last one in which
every formula existed twice -- once for one hyper-parameter vector and once, hand-vectorised, for the B rows of a chain
block (`inv` / `inv_rows`, `_chain_rule` / `_chain_rule_rows`, `th_loglike` / `_chain_density`, ...).  The recording half
of this file called those paired names and went with them; it is not in the repository, so the fixture CANNOT be
regenerated or its origin checked from this tree: it is a record of that commit, taken on trust.  What is left builds the same inputs and objects on the
current code -- `inputs()`, `mapping_cases()`, `mean_cases()`, `freedom_case()`, `packing_cases()`, `gradient_cases()`,
`program()` -- and reads the arrays (`load()`); tests/test_host_rows.py imports both.  No device is needed:
compile_spec and g3_grad_layout are host code.

Keys, with <t> = f8 | f4 (the dtype of the observations), `_one` = the one-row form evaluated row by row and stacked,
`_rows` = the B-row form, every array with the B = 7 rows first:
  inputs/<name>                                   inputs() as recorded
  <t>/map/<Mapping>/values/<hyper>                mapping_cases(): the rows of natural-space hyper values
  <t>/map/<Mapping>/call_one                      mapping(x)
  <t>/map/<Mapping>/inv_{one,rows}, logdet_{one,rows}
  <t>/map/<Mapping>/grad_{one,rows}/<i>/{dinv,dlogdet}     entry i of grad / grad_rows
  <t>/mean/<Mean>/values/<hyper>, call_one, rows, grad_one/<i>
  <t>/freedom/{values,one,rows}
  <t>/diag/logp_cho_diag_one, loo_rows/logpredictive, loo_one/<None|10>/<key>    Box-Cox warp on inputs' alpha, kdiag;
                                                  loo_assemble per row with hermite None | 10, var and median on
  <t>/density/{gauss,student}/{one,rows}          th_loglike's arithmetic per row / _chain_density on inputs' st, det_m
  <t>/grad/{wgp,tp}/chain, slots                  gradient_cases()'s chain, the synthetic device sums (B, nslots)
  <t>/grad/{wgp,tp}/{pot,scale,rule}_{one,rows}/<variable>, s_{one,rows}, flat_{one,rows}
                                                  the natural-space gradient after _potential_gradient, _dlogp_scale (and
                                                  its s) and _chain_rule, then _flat_gradient; rows with inputs' ok False
                                                  got no likelihood term
  values/<i>/chain, logjac_{one,rows}, {one,rows}/<hyper>    packing_cases()[i]: _values / _values_rows
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'tests', 'golden', 'host_rows.npz')

N, B, D = 25, 7, 3
DTYPES = (('f8', np.float64), ('f4', np.float32))


def as_rows(a):
    from g3py_amd.device import Rows
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(Rows)


def row(values_rows, j):
    return {k: np.asarray(v)[j] for k, v in values_rows.items()}


def inputs():
    """observations, inputs and synthetic device results shared by every family (float64; cast per dtype)"""
    rng = np.random.default_rng(20261019)
    y = rng.uniform(0.5, 3.0, N)
    y[3] = 0.2                                   # with shift = -0.3 the Box-Cox `shifted` is negative here
    X = rng.uniform(0, 5, (N, D))
    x = 0.4 * rng.standard_normal(N)             # argument of the forward maps
    alpha = rng.standard_normal((B, N))
    kdiag = rng.uniform(0.5, 2.0, (B, N))
    kdiag[4, 7] = -0.1                           # sd = 1 / sqrt(kdiag) is NaN: that row takes the sentinel
    st = np.zeros((B, 6))
    st[:, 0] = rng.uniform(-5, 5, B)             # log det
    st[:, 1] = rng.uniform(5, 60, B)             # quad
    ok = np.array([True, True, False, True, True, False, True])
    return dict(y=y, X=X, x=x, alpha=alpha, kdiag=kdiag, st=st, ok=ok, det_m=rng.standard_normal(B))


def mapping_cases(special_powers=False):
    """{class name: (mapping, values_rows)} for every built-in mapping, B rows of natural-space hyper values.
    special_powers=True puts BoxCoxLinear's power at exactly 0.5 and 2.0 on two rows (NumPy's scalar fast paths)."""
    import g3py_amd as g3
    from g3py_amd.processes.hypers import Model
    rng = np.random.default_rng(7)
    y = inputs()['y']
    out = {}
    with Model('host_rows_mappings'):
        for cls in (g3.Identity, g3.LinearMapping, g3.LogShifted, g3.BoxCoxLinear, g3.ArcsinhLinear):
            m = cls(name=cls.__name__)
            m.check_hypers('P_')
            name = 'P_' + cls.__name__
            if cls is g3.Identity:
                v = {}
            elif cls is g3.LogShifted:
                shift = rng.uniform(-1.0, 0.1, B)
                shift[5] = y.min() + 0.3                                   # shift > min(y): log of a negative number
                v = {name + '_shift': shift}
            elif cls is g3.BoxCoxLinear:
                power = np.array([1e-6, 0.3, 1.0, 3e-6, 1.7, 0.8, 2.5])    # both sides of the 1e-5 switch
                if special_powers:
                    power[1], power[4] = 0.5, 2.0
                shift = np.array([0.5, -0.3, 1.0, -0.3, 0.0, 2.0, 0.7])    # -0.3: y[3] + shift < 0
                v = {name + '_shift': shift, name + '_scale': np.exp(0.3 * rng.standard_normal(B)), name + '_power': power}
            else:
                v = {name + '_shift': rng.standard_normal(B), name + '_scale': np.exp(0.3 * rng.standard_normal(B))}
            out[cls.__name__] = (m, {k: as_rows(a) for k, a in v.items()})
    return out


def mean_cases():
    """{class name: (mean, values_rows)} for every built-in mean on D = 3 columns; Linear's coeff is per column"""
    import g3py_amd as g3
    from g3py_amd.processes.hypers import Model
    rng = np.random.default_rng(8)
    X = inputs()['X']
    out = {}
    with Model('host_rows_means'):
        for cls in (g3.Zero, g3.Bias, g3.Linear):
            m = cls(X, name=cls.__name__)
            m.check_hypers('P_')
            v = {h.name: as_rows(rng.standard_normal((B,) + tuple(h.shape))) for h in m.hypers}
            out[cls.__name__] = (m, v)
    return out


def freedom_case():
    from g3py_amd.processes.hypers import Freedom, Model
    with Model('host_rows_freedom'):
        f = Freedom()
        f.check_dims(None)
        f.check_hypers('TP_')
    # nu = 2 + degree on both sides of the 1e6 switch of the Student-t density, and exactly on it
    return f, {f.degree.name: as_rows([1.5, 10.0, 1e3, 999997.9, 999998.0, 2e6, 1e7])}


def packing_cases():
    """the three processes and chains of tests/test_host.py::test_chain_rows_packing_equals_row_by_row (its row 2
    underflows the FlatExp variables; the first process carries an L2 potential)"""
    import g3py_amd as g3
    rng = np.random.default_rng(3)
    X = rng.uniform(0, 5, (25, 3))
    y = np.sin(X.sum(1)) + 3.0
    k1 = g3.SE(X)
    k1.set_potential('var', 'L2', c=0.5)
    cases = [
        g3.GP(space=X, location=g3.Bias(), kernel=2.5 * k1 * g3.SIN(X) + g3.RQ(X[:, :2], name='RQ2') + 0.25),
        g3.WGP(space=X, location=g3.Linear(), kernel=g3.MAT52(X) + g3.COS(X) * g3.OU(X), mapping=g3.BoxCoxLinear()),
        g3.WGP(space=X, location=g3.Zero(), kernel=g3.SM(X) + g3.WN(X), mapping=g3.LinearMapping()),
    ]
    out = []
    for gp in cases:
        gp.observed(X, y)
        base = gp.active.dict_to_array(gp.params_default)
        chain = base[None, :] + 0.3 * rng.standard_normal((B, gp.active.ndim))
        chain[2, :] = -40.0
        out.append((gp, chain))
    return out


def gradient_cases(dtype):
    """{'wgp' | 'tp': (process, chain, X, y)}: a WGP(BoxCoxLinear, Linear, SE + RQ with an L2 potential) and a
    StudentTProcess on N = 25 observations, B rows around the default parameters"""
    import g3py_amd as g3
    rng = np.random.default_rng(11)
    X = rng.uniform(0, 4, (N, 2))
    y = np.exp(0.3 * np.sin(X.sum(1))) + 0.02 * rng.standard_normal(N) + 1.0
    k = g3.SE(X)
    k.set_potential('var', 'L2', c=0.3)
    wgp = g3.WGP(space=X[:4], location=g3.Linear(X), kernel=k + g3.RQ(X), mapping=g3.BoxCoxLinear(y), dtype=dtype)
    tp = g3.StudentTProcess(space=X[:4], location=g3.Bias(X), kernel=g3.MAT52(X) + g3.COS(X), dtype=dtype)
    out = {}
    for name, p in (('wgp', wgp), ('tp', tp)):
        p.observed(X, y)
        base = p.active.dict_to_array(p.params)
        chain = base[None, :] + 0.1 * rng.standard_normal((B, len(base)))
        if name == 'tp':
            chain[6, -1] = np.log(3e6)           # the degree is the last variable: nu above the 1e6 switch
        out[name] = (p, chain, p._x(X), np.asarray(y, dtype=dtype))
    return out


def program(p, values0, d):
    """(template program, gradient slot map, number of slots) of the observation kernel -- host code, no device"""
    from g3py_amd import _lib
    from g3py_amd.device import compile_spec
    prog = compile_spec(p.f_kernel_noise.spec(values0, d), d)
    gmap = _lib.GradMap()
    assert _lib.load().g3_grad_layout(C.byref(prog), C.byref(gmap)) == 0
    return prog, gmap, int(gmap.nslots)


def load(path=OUT):
    """{key: array} as record() returned it"""
    import json
    with np.load(path) as z:
        index, blobs = json.loads(str(z['index'])), {'f8': z['f8'], 'f4': z['f4']}
    out, at = {}, {'f8': 0, 'f4': 0}
    for name, kind, shape, dt in index:
        n = int(np.prod(shape))
        out[name] = blobs[kind][at[kind]:at[kind] + n].reshape(shape).astype(dt)
        at[kind] += n
    return out
