"""Inputs, kernels, truth and tolerance shared by test_input_domain_host.py (CPU) and test_gpu_input_domain.py (GPU).

Every kernel of the library is stationary or evaluated on differences, so K(U + c) == K(U) for any translation c.  The
cases below put the same seeded grid points U at the origin (the control) and far from it, with c chosen so that U + c
is exact in the working type: then the covariance of X = U + c has an exact value -- the extended-precision covariance
of U -- and the reference's own formula in the working type on X says how close a correct evaluation in that type gets.

  truth = oracle kernel_cov(spec, U)  in np.longdouble          (exact: X - c == U)
  yard  = oracle kernel_cov(spec, X)  in the working type T     (the direct formula, as the reference writes it)
  tol   = 4 * max|yard - truth| + 8 * eps_T * max|truth|

The factor 4 leaves room for another order of the same roundings (per-tile trig tables and the angle-difference identity
in place of cos of the difference: emulated at the end of this file) and for the difference between the host's and the
device's math library.  Neither truth nor tolerance comes from the code under test."""
import functools

import numpy as np

N, M = 200, 70          # four 64-row tiles by two 128-column tiles, ragged edges, off-diagonal tiles; the cross block is M x N
GT, GTN = 64, 128       # the Gram kernels' tile (g3_gram.hip)

#        name          type        d  grid    span  offset c per column
CASES = {
    'f32-c0': (np.float32, 3, 2.0 ** -10, 3.0, (0.0, 0.0, 0.0)),
    'f32-far': (np.float32, 3, 2.0 ** -10, 3.0, (2048.0, -2048.0, 1958.0)),
    'f64-c0': (np.float64, 3, 2.0 ** -10, 3.0, (0.0, 0.0, 0.0)),
    'f64-far': (np.float64, 3, 2.0 ** -10, 3.0, (2.0 ** 30, -2.0 ** 30, 2.0 ** 20)),
    # d = 4: the width at which the compile-time table carries  stationary (+|x) periodic  (it has no d = 3 variants)
    'f32-c0-d4': (np.float32, 4, 2.0 ** -10, 3.0, (0.0, 0.0, 0.0, 0.0)),
    'f32-far-d4': (np.float32, 4, 2.0 ** -10, 3.0, (2048.0, -2048.0, 1958.0, -1958.0)),
    'f64-c0-d4': (np.float64, 4, 2.0 ** -10, 3.0, (0.0, 0.0, 0.0, 0.0)),
    'f64-far-d4': (np.float64, 4, 2.0 ** -10, 3.0, (2.0 ** 30, -2.0 ** 30, 2.0 ** 20, -2.0 ** 20)),
    # a time series indexed by calendar year with a yearly period
    'f32-years-c0': (np.float32, 1, 2.0 ** -6, 64.0, (0.0,)),
    'f32-years': (np.float32, 1, 2.0 ** -6, 64.0, (1958.0,)),
}
OFFSET_CASES = [c for c in CASES if any(CASES[c][4])]


def case_dtype(case):
    return CASES[case][0]


def case_d(case):
    return CASES[case][1]


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(U, Us, X, Xs): U, Us float64 grid points (N x d, M x d), X = U + c and Xs = Us + c in the case's type.  The same U
    for every case of one (d, grid): seeded by those alone."""
    T, d, grid, span, c = CASES[case]
    rng = np.random.default_rng(1000 * d + int(span))
    steps = int(round(span / grid))
    U = rng.integers(0, steps, (N, d)).astype(np.float64) * grid
    Us = rng.integers(0, steps, (M, d)).astype(np.float64) * grid
    Us[:3] = U[:3]                      # coincident pairs in the cross block (SINC's dx == 0 branch, WN)
    cT = np.asarray(c, dtype=T)
    X, Xs = U.astype(T) + cT, Us.astype(T) + cT
    for a in (U, Us, X, Xs):
        a.setflags(write=False)
    return U, Us, X, Xs


def offsets_exact(case):
    """U + c carries no rounding in the case's type"""
    c = np.asarray(CASES[case][4], dtype=np.longdouble)
    U, Us, X, Xs = inputs(case)
    return (X.dtype == CASES[case][0] and np.array_equal(X.astype(np.longdouble) - c, U.astype(np.longdouble)) and
            np.array_equal(Xs.astype(np.longdouble) - c, Us.astype(np.longdouble)))


TABLE_SHAPES = ('T:SE+SIN', 'T:MAT52+SM', 'T:SE*COS', 'T:SE+COS+NOISE')


def kernels(case):
    """name -> spec: the kernel zoo of tests/test_gpu_gram.py at d = 3; the shapes of the compile-time table's periodic
    variants ('T:...') at every width, frequency 0.7 per column; the bare periodic leaves for the time series, where every
    frequency is 1 (a yearly period)"""
    from oracle.gen_golden import kernel_zoo
    d = case_d(case)
    r = np.linspace(0.6, 1.4, d)
    f = np.ones(1) if d == 1 else np.full(d, 0.7)
    out = dict(kernel_zoo(3)) if d == 3 else {}
    if d == 1:
        out['COS'] = ('COS', 0.8, f, None)
        out['SIN'] = ('SIN', 0.5, f, 0.25 * r, None)
        out['SM'] = ('SM', 0.9, f, 0.05 * r, None)
    out['T:SE+SIN'] = ('sum', ('SE', 1.3, r, None), ('SIN', 0.5, f, 0.25 * r, None))
    out['T:MAT52+SM'] = ('sum', ('MAT52', 1.3, r, None), ('SM', 0.5, f, 0.3 * r, None))
    out['T:SE*COS'] = ('prod', ('SE', 1.0, r, None), ('COS', 1.0, f, None))
    out['T:SE+COS+NOISE'] = ('sum', ('sum', ('SE', 1.3, r, None), ('COS', 0.5, f, None)), ('NOISE', 0.1))
    return out


def on_table(case, name):
    """does the kernel match the compile-time table (g3_host.h::g3h_match_fast)?  One stationary leaf on all columns at any
    instantiated width; stationary (+|x) periodic (+ noise) only at d in {1, 2, 4, 8}.  Everything else runs a generated kernel."""
    if name in ('SE', 'OU', 'MAT32', 'MAT52', 'RQ'):
        return True
    return case_d(case) != 3 and name in TABLE_SHAPES


def eps(case):
    return float(np.finfo(case_dtype(case)).eps)


@functools.lru_cache(maxsize=None)
def truth(case, name, cross=False):
    """the covariance of the un-offset points in extended precision (every kind of the oracle accepts np.longdouble)"""
    from oracle import g3_oracle as orc
    U, Us, _, _ = inputs(case)
    spec = kernels(case)[name]
    K = orc.kernel_cov(spec, Us, U, dtype=np.longdouble) if cross else orc.kernel_cov(spec, U, dtype=np.longdouble)
    K.setflags(write=False)
    return K


@functools.lru_cache(maxsize=None)
def yard(case, name, cross=False):
    """the reference's direct formula in the working type on the offset inputs"""
    from oracle import g3_oracle as orc
    _, _, X, Xs = inputs(case)
    spec = kernels(case)[name]
    T = case_dtype(case)
    K = orc.kernel_cov(spec, Xs, X, dtype=T) if cross else orc.kernel_cov(spec, X, dtype=T)
    assert K.dtype == T
    K.setflags(write=False)
    return K


def yard_err(case, name, cross=False):
    return float(np.abs(yard(case, name, cross).astype(np.longdouble) - truth(case, name, cross)).max())


def tol(case, name, cross=False):
    return 4.0 * yard_err(case, name, cross) + 8.0 * eps(case) * float(np.abs(truth(case, name, cross)).max())


def err(got, case, name, cross=False):
    return float(np.abs(np.asarray(got).astype(np.longdouble) - truth(case, name, cross)).max())


def spec_freqs(spec):
    """the frequency vectors of the periodic leaves of a spec tree"""
    op = spec[0]
    if op in ('sum', 'prod'):
        return spec_freqs(spec[1]) + spec_freqs(spec[2])
    if op in ('scale', 'shift'):
        return spec_freqs(spec[2])
    return [np.atleast_1d(np.asarray(spec[2], dtype=np.float64))] if op in ('COS', 'SIN', 'SINC', 'SM') else []


def yard_bound(case, name, cross=False):
    """what the direct formula in the working type may miss the truth by: 64 eps (1 + 2 pi sum_k f_k span_k) max|truth|,
    the rounding of theta = 2 pi f dx over the span of the inputs (not over their distance from the origin)"""
    span = CASES[case][3]
    fs = sum(float(f.sum()) for f in spec_freqs(kernels(case)[name]))
    return 64.0 * eps(case) * (1.0 + 2.0 * np.pi * fs * span) * float(np.abs(truth(case, name, cross)).max())


# ---------------------------------------------------------------- NumPy emulation of the kernels' per-tile trig tables
def periodic_probe(case, local):
    """(spec, COS leaf, stationary factor or None) of the kernel the emulation evaluates: the bare COS leaf of the case
    (the zoo's at d = 3, frequency 0.7 at d = 4, a yearly period for the time series) or, local True, the locally
    periodic SE * COS of the case, whose entries of any size sit on close pairs"""
    if local:
        spec = kernels(case)['T:SE*COS']
        return spec, spec[2], spec[1]
    d = case_d(case)
    f = np.linspace(0.11, 0.23, 3) if d == 3 else np.ones(1) if d == 1 else np.full(d, 0.7)
    leaf = ('COS', 0.8, f, None)
    return leaf, leaf, None


def _two_prod(a, b):
    """a * b == hi + lo exactly, both in the type of a and b (what an fma's residual gives on the device)"""
    if a.dtype == np.float32:
        p = a.astype(np.float64) * b.astype(np.float64)             # 24 + 24 bits: exact in float64
        hi = p.astype(np.float32)
        return hi, (p - hi.astype(np.float64)).astype(np.float32)
    hi = a * b                                                      # float64: Dekker's product on Veltkamp's split

    def split(v):
        c = 134217729.0 * v
        h = c - (c - v)
        return h, v - h
    a1, a2 = split(a)
    b1, b2 = split(b)
    return hi, ((a1 * b1 - hi) + a1 * b2 + a2 * b1) + a2 * b2


def table_emulation(case, mode, cross=False, local=False):
    """NumPy emulation, in the case's type, of the COS leaf as the Gram kernels evaluate it: [cos, sin] of theta per point,
    then cos(theta_i - theta_j) = c_i c_j + s_i s_j per pair and dimension (times the stationary factor by the direct
    formula).  theta = 2 pi f x is formed
      'origin'  from x itself, as a plain product;
      'tile'    from x - x0, x0 the first column point of the pair's 128-column tile, as a plain product;
      'exact'   modulo 2 pi, the whole periods taken off the exact product:  2 pi fma(f, x, -rint(f x)), which is what
                g3_kernel_eval.h::trig_theta computes."""
    from oracle import g3_oracle as orc
    T = case_dtype(case)
    _, _, X, Xs = inputs(case)
    _, leaf, stat = periodic_probe(case, local)
    var, f = T(leaf[1]), np.asarray(leaf[2], dtype=T)
    rows, cols = (Xs if cross else X), X

    def theta(x, x0):
        if mode == 'exact':             # fma(f, x, -rint(f * x)): hi - n is exact, so the sum below rounds once, as the fma
            hi, lo = _two_prod(np.broadcast_to(f, x.shape), x)
            th = T(2 * np.pi) * ((hi - np.rint(hi)) + lo)
        else:
            th = T(2 * np.pi) * f * (x - x0 if mode == 'tile' else x)
        assert th.dtype == T
        return th
    K = np.empty((len(rows), len(cols)), dtype=T)
    for j0 in range(0, len(cols), GTN):
        thi, thj = theta(rows, cols[j0]), theta(cols[j0:j0 + GTN], cols[j0])
        cd = np.cos(thi)[:, None, :] * np.cos(thj)[None, :, :] + np.sin(thi)[:, None, :] * np.sin(thj)[None, :, :]
        K[:, j0:j0 + GTN] = var * np.prod(cd, axis=2)
    if stat is not None:
        K = orc.kernel_cov(stat, Xs, X, dtype=T) * K if cross else orc.kernel_cov(stat, X, dtype=T) * K
    assert K.dtype == T
    return K


def probe_truth(case, cross=False, local=False):
    """(truth, yard error, tol) of periodic_probe(case, local): what the emulation is held against"""
    from oracle import g3_oracle as orc
    U, Us, X, Xs = inputs(case)
    T, spec = case_dtype(case), periodic_probe(case, local)[0]
    tr = orc.kernel_cov(spec, Us, U, dtype=np.longdouble) if cross else orc.kernel_cov(spec, U, dtype=np.longdouble)
    yd = orc.kernel_cov(spec, Xs, X, dtype=T) if cross else orc.kernel_cov(spec, X, dtype=T)
    ye = float(np.abs(yd.astype(np.longdouble) - tr).max())
    return tr, ye, 4.0 * ye + 8.0 * eps(case) * float(np.abs(tr).max())
