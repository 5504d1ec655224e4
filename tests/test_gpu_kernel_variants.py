"""The compile-time variants of gemm_nt_kernel and trsm_stripe_kernel that the host only picks for LARGE problems, at
SMALL shapes: element by element against an fp64 NumPy/SciPy reference of the same operation on the same inputs (fp32: on
the fp32-rounded inputs), with the launch log (G3_GEMM_LOG, format in g3_host.h) as the proof that the intended variant
is the one that ran.

  g3_gemm.hip::launch_t       64 x 64 tile by default; the eight-wave 128 x 128 tile from G3_GEMM_BIG_MIN (4096) tiles on,
                              or from G3_GEMM_BIG_MIN_K (1024) tiles on when K >= 1024; 32 x 128 for the in-place leaf
  g3_gemm.hip::g3i_trsm_stripe  16-row stripes while m x batch <= G3_TRSM_THIN_MAX (2048), 32-row stripes above,
                              64-row stripes from G3_TRSM_WIDE_MIN (12288) rows on

The knobs are read once per context (g3_host.h::g3h_tune_from_env), so every case runs in a fresh g3.Device(0) created
under the knobs it names and closed before the next one; each knob selects another schedule of the same arithmetic.  A
case whose knob did not select the variant fails on the log, it does not pass on the default kernel."""
import collections
import contextlib
import functools
import itertools
import types

import numpy as np
import pytest
import scipy.linalg

pytestmark = pytest.mark.gpu

TOL = {np.float64: 5e-13, np.float32: 2e-4}        # tests/test_gpu_kernels.py: per 64 terms of a product, relative to max|ref|
DTYPES = [np.float64, np.float32]

# every knob of G3hTune: a context of this file sees the ones its case names and the defaults for all the others,
# whatever the environment of the run holds
KNOBS = ('G3_NB', 'G3_SB', 'G3_NB_TAIL', 'G3_NB_MIN', 'G3_NB_HEAD', 'G3_SIDE_LDS', 'G3_GEMM_BIG_MIN', 'G3_GEMM_BIG_MIN_K',
         'G3_TRSM_THIN_MAX', 'G3_TRSM_WIDE_MIN', 'G3_TRSM_SPLIT_MIN', 'G3_TRSM_SPLIT_N', 'G3_STAIR_MAX', 'G3_GRAM_NOFAST',
         'G3_GRAD_GENERIC', 'G3_GRAM_JIT', 'G3_COOP_MAX_N', 'G3_COOP_MIN_BATCH', 'G3_COOP_GROUP', 'G3_PROBE')

# one launch: `op` is 'gemm' or 'trsm'; for a stripe solve bm is the stripe height and ntiles the stripe count
Launch = collections.namedtuple('Launch', 'op bm bn waves m n k kind ntiles flops bulk')
_serial = itertools.count()


def _parse_log(path):
    out = []
    with open(path) as f:
        for line in f:
            w = line.split()
            assert len(w) == 11 and w[0] in ('gemm', 'trsm'), line
            out.append(Launch(w[0], *[int(x) for x in w[1:9]], float(w[9]), int(w[10])))
    return out


@contextlib.contextmanager
def variant_context(monkeypatch, tmp_path, **knobs):
    """a fresh context under exactly these knobs, logging its launches: yields an object with `.dev`; once the block
    is left the context is closed (that flushes the log) and `.log` holds the parsed lines"""
    import g3py_amd as g3
    assert set(knobs) <= set(KNOBS), knobs
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, value in knobs.items():
        monkeypatch.setenv(name, str(value))
    path = tmp_path / ('launches%d.log' % next(_serial))
    monkeypatch.setenv('G3_GEMM_LOG', str(path))
    run = types.SimpleNamespace(dev=g3.Device(0), log=None)
    try:
        yield run
    finally:
        run.dev.close()
        monkeypatch.delenv('G3_GEMM_LOG')
        run.log = _parse_log(path)


def _tiles(log, op='gemm'):
    return [(l.bm, l.bn, l.waves) for l in log if l.op == op]


def _spd(rng, n):
    B = rng.standard_normal((n, max(8, n // 4)))
    return B @ B.T / B.shape[1] + np.eye(n)


def _cond_of_factor(K):
    """cond_2(L) for K = L L^T: the singular values of L are the square roots of the eigenvalues of K"""
    w = np.linalg.eigvalsh(K)
    return float(np.sqrt(w[-1] / w[0]))


# ------------------------------------------------------------------ 1. the 128 x 128 tile, every raster
def _gemm_case(dev, dt, m, n, k, lower, seed):
    """C <- C - 0.5 A B^T on an (m, n) block of a C with 64 guard columns; returns (C before, C after, reference)"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, k)).astype(dt)
    B = rng.standard_normal((n, k)).astype(dt)      # asymmetric operands: a transposed C would show
    C = rng.standard_normal((m, n + 64)).astype(dt)
    Ad, Bd, Cd = dev.upload(A), dev.upload(B), dev.upload(C)
    assert Cd.ld == n + 64
    dev.gemm_nt(Cd, Ad, Bd, m, n, k, alpha=-0.5, beta=1.0, lower_only=lower)
    got = dev.download(Cd)
    ref = C[:, :n].astype(np.float64) - 0.5 * A.astype(np.float64) @ B.astype(np.float64).T
    return C, got, ref


def _check_gemm(C, got, ref, dt, n, k, lower):
    m = C.shape[0]
    mask = np.tril(np.ones((m, n), bool)) if lower else np.ones((m, n), bool)
    err = np.abs(got[:, :n] - ref)[mask].max()
    tol = TOL[dt] * np.abs(ref[mask]).max() * max(1, k / 64)
    print('gemm %s m=%d n=%d k=%d lower=%d: max err %.3e (tol %.3e)' % (np.dtype(dt).name, m, n, k, lower, err, tol))
    np.testing.assert_array_equal(got[:, n:], C[:, n:])                     # the guard columns
    if lower:
        np.testing.assert_array_equal(got[:, :n][~mask], C[:, :n][~mask])   # above the diagonal: the old C, exactly
    assert err <= tol


BIG_TILE_CASES = [
    ('one_tile', 128, 128, 32, False), ('one_tile', 128, 128, 96, False),
    ('dense_6_tiles', 256, 384, 32, False), ('dense_6_tiles', 256, 384, 96, False),    # fewer tiles than the 8 XCDs
    ('dense_15_tiles', 640, 384, 96, False),       # uneven XCD remap; row groups of 4 + 1
    ('trapezoid_tall', 640, 384, 96, True),
    ('trapezoid_wide', 384, 640, 96, True),        # tiles above the diagonal are not launched
    ('square_lower', 512, 512, 256, True),
]


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('case,m,n,k,lower', BIG_TILE_CASES)
def test_big_tile_every_raster(monkeypatch, tmp_path, dt, case, m, n, k, lower):
    """gemm_nt_kernel<T, 128, 128, 64, 32> (G3_GEMM_BIG_MIN=1) on its dense and trapezoid rasters.  k = 32 is a single
    K tile in fp32; k = 96 is an odd tile count in fp32 (3 x 32) and an even one in fp64 (6 x 16): both parities of the
    double buffer"""
    with variant_context(monkeypatch, tmp_path, G3_GEMM_BIG_MIN=1) as run:
        C, got, ref = _gemm_case(run.dev, dt, m, n, k, lower, m * 7 + n * 3 + k)
    assert _tiles(run.log) == [(128, 128, 8)] and _tiles(run.log, 'trsm') == []
    l = run.log[0]
    assert (l.m, l.n, l.k, l.kind, l.bulk) == (m, n, k, 1 if lower else 0, 0)
    dense = (m // 128) * (n // 128)
    if not lower:
        assert l.ntiles == dense
    elif case == 'trapezoid_wide':
        assert l.ntiles == (m // 128) ** 2 < dense      # one group of three row tiles: columns up to its last row's diagonal
    _check_gemm(C, got, ref, dt, n, k, lower)


@pytest.mark.parametrize('dt', DTYPES)
def test_big_tile_by_the_k_clause(monkeypatch, tmp_path, dt):
    """the second selection clause of launch_t: the 128 x 128 tile from G3_GEMM_BIG_MIN_K tiles on when K >= 1024 (it only
    applies while G3_GEMM_BIG_MIN has its default 4096, so that knob stays unset); the same product just below K = 1024
    stays on the 64 x 64 tile"""
    m = n = 256
    with variant_context(monkeypatch, tmp_path, G3_GEMM_BIG_MIN_K=1) as run:
        C, got, ref = _gemm_case(run.dev, dt, m, n, 1024, False, 41)
        C2, got2, ref2 = _gemm_case(run.dev, dt, m, n, 992, False, 42)
    assert _tiles(run.log) == [(128, 128, 8), (64, 64, 4)]
    assert [(l.m, l.n, l.k, l.kind) for l in run.log] == [(m, n, 1024, 0), (m, n, 992, 0)]
    _check_gemm(C, got, ref, dt, n, 1024, False)
    _check_gemm(C2, got2, ref2, dt, n, 992, False)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('lower', [False, True])
def test_big_tile_unaligned_c_takes_the_scalar_epilogue(monkeypatch, tmp_path, dt, lower):
    """the body of test_gemm_unaligned_c_takes_the_scalar_epilogue (tests/test_gpu_kernels.py) at a shape the 128 x 128
    tile accepts: an odd leading dimension and a start one element into the row make the kernel leave the vectorised LDS
    epilogue for element-wise stores from the MFMA layout (eight waves of 64 x 32 here); beta = 0 must not read C"""
    m, n, k, ld = 256, 128, 64, 131
    es = np.dtype(dt).itemsize
    rng = np.random.default_rng(11)
    A = rng.standard_normal((m, k)).astype(dt)
    B = rng.standard_normal((n, k)).astype(dt)
    C = rng.standard_normal((m, ld)).astype(dt)
    prod = A.astype(np.float64) @ B.astype(np.float64).T
    mask = np.tril(np.ones((m, n), bool)) if lower else np.ones((m, n), bool)
    with variant_context(monkeypatch, tmp_path, G3_GEMM_BIG_MIN=1) as run:
        dev = run.dev
        Ad, Bd, Cd = dev.upload(A), dev.upload(B), dev.upload(C)
        dev.gemm_nt(Cd, Ad, Bd, m, n, k, alpha=2.0, beta=-1.0, lower_only=lower, c_off=es)      # starts at column 1
        got = dev.download(Cd)
        C0 = dev.upload(np.full((m, n), np.nan, dtype=dt))           # beta = 0 must not read C: aligned ...
        dev.gemm_nt(C0, Ad, Bd, m, n, k, alpha=1.0, beta=0.0)
        got0 = dev.download(C0)
        C1 = dev.upload(np.full((m, ld), np.nan, dtype=dt))          # ... and through the scalar epilogue
        dev.gemm_nt(C1, Ad, Bd, m, n, k, alpha=1.0, beta=0.0, lower_only=lower, c_off=es)
        got1 = dev.download(C1)
    assert _tiles(run.log) == [(128, 128, 8)] * 3
    ref = C.astype(np.float64)
    ref[:, 1:1 + n] = np.where(mask, 2.0 * prod - ref[:, 1:1 + n], ref[:, 1:1 + n])
    assert np.abs(got - ref).max() <= TOL[dt] * np.abs(ref).max() * 4
    np.testing.assert_array_equal(got[:, 0], C[:, 0])                # the columns around the block, and what is above the
    np.testing.assert_array_equal(got[:, 1 + n:], C[:, 1 + n:])      # diagonal, keep their old values exactly
    np.testing.assert_array_equal(got[:, 1:1 + n][~mask], C[:, 1:1 + n][~mask])
    assert np.abs(got0 - prod).max() <= TOL[dt] * 50
    inside = np.zeros((m, ld), bool)
    inside[:, 1:1 + n] = mask
    assert np.abs(got1[inside] - prod[mask]).max() <= TOL[dt] * 50
    assert np.isnan(got1[~inside]).all()


# ------------------------------------------------------------------ 2. k_tri (triangular B: Kt = n0 + BN) on both tiles
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('n,m', [(256, 128), (256, 384), (640, 128), (640, 384)])
def test_triangular_product_on_both_tiles(monkeypatch, tmp_path, dt, n, m):
    """g3_trsm_full, X = B V^T with V lower triangular: the column tile at n0 stops its reduction at Kt = n0 + BN.  n = 640
    is five column tiles of 128 (Kt = 128 ... 640 = K) and ten of 64; m = 384 is more than one row tile of either.  Both
    tiles against B @ V.T in fp64, and against each other."""
    from g3py_amd import _lib
    rng = np.random.default_rng(n + m)
    V = np.tril(rng.standard_normal((n, n)))
    V[np.diag_indices(n)] = 1.0 + np.abs(rng.standard_normal(n))
    V = V.astype(dt)
    B = rng.standard_normal((m, n)).astype(dt)
    ref = B.astype(np.float64) @ V.astype(np.float64).T
    tol = TOL[dt] * np.abs(ref).max() * max(1, n / 64)
    guard = np.full((m, n + 64), -7.25, dtype=dt)           # X inside a wider buffer: the columns beyond n stay as they are
    res = {}
    for name, knobs, tile in (('small', {}, (64, 64, 4)), ('big', {'G3_GEMM_BIG_MIN': 1}, (128, 128, 8))):
        with variant_context(monkeypatch, tmp_path, **knobs) as run:
            dev = run.dev
            Vd, Bd, Xd = dev.upload(V), dev.upload(B), dev.upload(guard)
            assert dev.lib.g3_trsm_full(dev.ctx, Vd.ptr, n, Vd.ld, Bd.ptr, m, Bd.ld, Xd.ptr, Xd.ld, _lib.dtype_code(dt)) == 0
            got = dev.download(Xd)
        assert _tiles(run.log) == [tile], (name, run.log)
        l = run.log[0]
        assert (l.m, l.n, l.k, l.kind, l.ntiles) == (m, n, n, 0, (m // tile[0]) * (n // tile[1]))
        np.testing.assert_array_equal(got[:, n:], guard[:, n:])
        res[name] = got[:, :n].astype(np.float64)
        err = np.abs(res[name] - ref).max()
        print('k_tri %s %s n=%d m=%d: max err %.3e (tol %.3e)' % (name, np.dtype(dt).name, n, m, err, tol))
        assert err <= tol, name
    assert np.abs(res['small'] - res['big']).max() <= tol


# ------------------------------------------------------------------ 3. the stripe solve, every height and type
STRIPES = ((16, {}), (32, {'G3_TRSM_THIN_MAX': 0}), (64, {'G3_TRSM_WIDE_MIN': 64}))


@functools.lru_cache(maxsize=None)
def _trsm_problem(n, m):
    rng = np.random.default_rng(n + m)
    L = scipy.linalg.cholesky(_spd(rng, n), lower=True)
    B = rng.standard_normal((m, n))
    for a in (L, B):
        a.setflags(write=False)
    return L, B, float(np.linalg.cond(L))


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('n,m', [(256, 128), (384, 256), (640, 128), (1024, 256), (1536, 128)])
def test_stripe_solve_every_height(monkeypatch, tmp_path, dt, n, m):
    """g3_trsm_rlt, X <- X L^-T, through trsm_stripe_kernel<T, BM> for BM = 16 (default), 32 (G3_TRSM_THIN_MAX=0) and 64
    (G3_TRSM_WIDE_MIN=64).  n = 384 and 640 are the uneven splits of trsm_ops_rec; n = 1536 goes through trsm_rec's
    launch-level split (two stripe launches of 768 columns around one GEMM); m = 128 with BM = 64 is a two-workgroup grid.
    B sits in a buffer with 128 more rows and 32 more columns (ld = n + 32) that must come back bit-identical.

    The three heights on the same input: a row's arithmetic does not depend on the height of the stripe it is solved in
    -- every output element is accumulated by the same sequence of 16 x 16 x 4 MFMAs over the same K order -- and on
    MI355X the three results came out bit-identical in both types at all five shapes (max difference 0.0 in all twenty
    comparisons), so array_equal is what is asserted."""
    from g3py_amd import _lib
    L64, B64, cond = _trsm_problem(n, m)
    L, B = L64.astype(dt), B64.astype(dt)
    ref = scipy.linalg.solve_triangular(L.astype(np.float64), B.astype(np.float64).T, lower=True).T
    tol = (1e-11 if dt == np.float64 else 3e-4 * cond) * np.abs(ref).max()
    buf = np.full((m + 128, n + 32), -7.25, dtype=dt)
    buf[:m, :n] = B
    outside = np.ones(buf.shape, bool)
    outside[:m, :n] = False
    res = {}
    for bm, knobs in STRIPES:
        with variant_context(monkeypatch, tmp_path, **knobs) as run:
            dev = run.dev
            Ld, Bd = dev.upload(L), dev.upload(buf)
            assert dev.lib.g3_trsm_rlt(dev.ctx, Ld.ptr, n, Ld.ld, Bd.ptr, m, Bd.ld, _lib.dtype_code(dt), None) == 0
            got = dev.download(Bd)
        stripes = [l for l in run.log if l.op == 'trsm']
        widths = [n] if n <= 1024 else [768, 768]
        assert [(l.bm, l.bn, l.waves, l.m, l.n, l.ntiles) for l in stripes] == [(bm, 128, 4, m, w, m // bm) for w in widths], run.log
        assert [(l.m, l.n, l.k) for l in run.log if l.op == 'gemm'] == ([] if n <= 1024 else [(m, 768, 768)])
        np.testing.assert_array_equal(got[outside], buf[outside])
        res[bm] = got[:m, :n]
        err = np.abs(res[bm].astype(np.float64) - ref).max()
        print('trsm BM=%d %s n=%d m=%d: max err %.3e (tol %.3e)' % (bm, np.dtype(dt).name, n, m, err, tol))
        assert err <= tol, bm
    for bm in (32, 64):
        print('trsm BM=%d vs 16 %s n=%d m=%d: max diff %.3e' % (bm, np.dtype(dt).name, n, m,
                                                               np.abs(res[bm].astype(np.float64) - res[16]).max()))
    np.testing.assert_array_equal(res[32], res[16])
    np.testing.assert_array_equal(res[64], res[16])


# ------------------------------------------------------------------ 4. the sweep under each variant, element by element
# name -> (knobs, the GEMM tile the knobs ask for, the stripe height they ask for).  Without G3_NB the panels of a sweep
# at n <= 4096 are 128 columns wide, and a 128-column panel is solved by the in-place 32 x 128 leaf product, not by a
# stripe launch: the first two contexts name no stripe height and none is asserted for them.
SWEEPS = {
    'default': ({}, 64, None),
    'big_tile': ({'G3_GEMM_BIG_MIN': 1}, 128, None),
    'nb512_stripe32': ({'G3_NB': 512, 'G3_TRSM_THIN_MAX': 0}, 64, 32),
    'nb512_stripe64': ({'G3_NB': 512, 'G3_TRSM_WIDE_MIN': 64}, 64, 64),
    'nb256_big_tile_stripe64': ({'G3_NB': 256, 'G3_GEMM_BIG_MIN': 1, 'G3_TRSM_WIDE_MIN': 64}, 128, 64),
}


def _sweep_knobs(name, n):
    """the knobs of a sweep over n columns.  g3h_panel_bounds halves the panel width while the remaining size is
    <= G3_NB_TAIL (10) x width, which at n = 1536 brings EVERY panel of a G3_NB = 256 or 512 sweep down to 128 columns --
    no stripe launch at all, whatever the stripe knobs say, and the log assertion below says so.  At that size the
    contexts that set G3_NB therefore also set G3_NB_TAIL=0 (the width stays G3_NB throughout, as in
    test_logp_is_invariant_to_the_panel_width), so that their stripes do run; at n = 3072 the taper leaves two
    256-column panels and the knobs are exactly the named ones."""
    knobs, tile, stripe = SWEEPS[name]
    if n <= 1536 and 'G3_NB' in knobs:
        knobs = dict(knobs, G3_NB_TAIL=0)
    return knobs, tile, stripe


def _check_sweep_log(log, tile, stripe):
    """at least one launch of the intended tile, one of the intended stripe height (every stripe launch has it), and one of
    them on the bulk stream"""
    gemms = [l for l in log if l.op == 'gemm' and (l.bm, l.bn, l.waves) == (tile, tile, 8 if tile == 128 else 4)]
    assert gemms, log
    hits = list(gemms)
    if stripe is not None:
        stripes = [l for l in log if l.op == 'trsm']
        assert stripes and all((l.bm, l.ntiles) == (stripe, l.m // stripe) for l in stripes), log
        hits += stripes
    assert any(l.bulk == 1 for l in hits), log


# max|L - L_lapack| of the fp32 sweep in the DEFAULT context, measured on MI355X (see test_sweep_under_each_variant)
FP32_SWEEP_ERR = {1536: 5.0560e-07, 3072: 7.6681e-07}


@functools.lru_cache(maxsize=None)
def _potrf_problem(n, dtname):
    K = _spd(np.random.default_rng(n), n).astype(dtname)
    Lr = scipy.linalg.cholesky(K.astype(np.float64), lower=True)
    cond = _cond_of_factor(K.astype(np.float64)) if dtname == 'float32' else None
    for a in (K, Lr):
        a.setflags(write=False)
    return K, Lr, cond


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('n', [1536, 3072])
@pytest.mark.parametrize('name', list(SWEEPS))
def test_sweep_under_each_variant(monkeypatch, tmp_path, name, n, dt):
    """g3_potrf: the whole lower triangle of L against scipy.linalg.cholesky of the (fp32: fp32-rounded) input in fp64, the
    strict upper triangle untouched, in the default context and under each variant (knobs: SWEEPS and _sweep_knobs).

    fp64: 1e-12 sqrt(n), the figure of test_potrf_matches_lapack.  fp32: the project had no element-wise figure, so one was
    measured: max|L - L_lapack| of the DEFAULT context on MI355X is 5.0560e-07 at n = 1536 and 7.6681e-07 at n = 3072
    (FP32_SWEEP_ERR); the tolerance is four times the larger of the two, 3.07e-06 (variation between boxes and between
    variants), capped at 3e-4 cond(L) max|L| (1.4e-03 here: cond(L) = 3.15), the bound the project accepts for fp32
    triangular results.  A variant that exceeds what the default context meets fails.  (The variants measured 5.06e-07 ...
    7.78e-07 in the same run; fp64: 1.1e-15 ... 1.3e-15 everywhere.)"""
    knobs, tile, stripe = _sweep_knobs(name, n)
    K, Lr, cond = _potrf_problem(n, np.dtype(dt).name)
    with variant_context(monkeypatch, tmp_path, **knobs) as run:
        Kd = run.dev.upload(K)
        info = run.dev.potrf(Kd, n)
        got = run.dev.download(Kd)
    assert info == 0
    _check_sweep_log(run.log, tile, stripe)
    np.testing.assert_array_equal(np.triu(got, 1), np.triu(K, 1))          # strict upper triangle is never touched
    err = np.abs(np.tril(got).astype(np.float64) - Lr).max()
    if dt == np.float64:
        tol = 1e-12 * n ** 0.5
    else:
        tol = min(4 * max(FP32_SWEEP_ERR.values()), 3e-4 * cond * np.abs(Lr).max())
    print('potrf %s %s n=%d: max|L - L_lapack| %.4e (tol %.3e)' % (name, np.dtype(dt).name, n, err, tol))
    assert err <= tol


def test_tall_sweep_under_each_variant(monkeypatch, tmp_path):
    """g3_gp_factor_predict, SE + noise, d = 3, N = 1500 (ragged: Np = 1536), M = 200, fp64: the 128 + 256 appended rows
    (delta and K(Xs, X)) are more rows of every panel solve, so under the G3_NB contexts they pass through the 32- and
    64-row stripes (the first panel's stripe launch covers all of them: m = Np + 384 - G3_NB).  logdet, quad, a = L^-1 delta,
    the posterior mean and ss against oracle/g3_oracle.py at the suite's tolerances (scalars 1e-9, vectors 1e-8) and
    against the default context at 1e-11 x scale (test_logp_is_invariant_to_the_panel_width's figure)."""
    from oracle import g3_oracle as orc
    from g3py_amd import _lib
    from g3py_amd.device import compile_spec
    rng = np.random.default_rng(1500)
    N, d, M, noise = 1500, 3, 200, 0.1
    X = rng.uniform(0, N ** (1.0 / d), (N, d))
    Xs = rng.uniform(0, N ** (1.0 / d), (M, d))
    y = np.sin(X.sum(1)) + 0.1 * rng.standard_normal(N)
    spec_f = ('SE', 1.3, np.array([0.8, 1.0, 1.2]), None)
    Kn = orc.tt_to_num(orc.kernel_cov(orc.with_noise(spec_f, noise), X))
    L = scipy.linalg.cholesky(Kn, lower=True)
    a_ref = scipy.linalg.solve_triangular(L, y, lower=True)
    V = scipy.linalg.solve_triangular(L, orc.tt_to_num(orc.kernel_cov(spec_f, Xs, X)).T, lower=True)
    ref = dict(logdet=np.log(np.diag(L)).sum(), quad=a_ref.dot(a_ref), a=a_ref, mu=V.T.dot(a_ref), ss=(V ** 2).sum(0))
    Np, Mp = _lib.roundup(N), _lib.roundup(M, 128)
    E = _lib.G3_RHS_PAD + Mp
    res = {}
    for name in SWEEPS:
        knobs, tile, stripe = _sweep_knobs(name, Np)
        with variant_context(monkeypatch, tmp_path, **knobs) as run:
            dev = run.dev
            K = dev.alloc(Np + E, Np, np.float64)
            W, a = dev.alloc_inverses(Np, np.float64), dev.alloc(1, Np, np.float64)
            mu, ss = dev.alloc(1, Mp, np.float64), dev.alloc(1, Mp, np.float64)
            st = dev.gp_factor_predict(compile_spec(orc.with_noise(spec_f, noise), d), compile_spec(spec_f, d), dev.upload(X),
                                       N, d, dev.upload(y), dev.upload(Xs), M, K, W, a, mu, ss)
            res[name] = dict(logdet=st['logdet'], quad=st['quad'], a=dev.download(a, 1, N)[0], mu=dev.download(mu, 1, M)[0],
                             ss=dev.download(ss, 1, M)[0])
        assert st['info'] == 0 and st['tries'] == 0
        _check_sweep_log(run.log, tile, stripe)
        if stripe is not None:      # the appended rows are in the first panel's stripe launch
            assert any(l.op == 'trsm' and l.m == Np + E - knobs['G3_NB'] for l in run.log), run.log
        for key in ('logdet', 'quad'):
            assert abs(res[name][key] - ref[key]) <= 1e-9 * max(1.0, abs(ref[key])), (name, key)
        for key in ('a', 'mu', 'ss'):
            np.testing.assert_allclose(res[name][key], ref[key], rtol=1e-8, atol=1e-8, err_msg='%s %s' % (name, key))
    for name in SWEEPS:
        for key, want in res['default'].items():
            diff = np.abs(res[name][key] - want).max()
            print('tall %s %s: max diff to the default context %.3e' % (name, key, diff))
            assert diff <= 1e-11 * np.abs(want).max(), (name, key)


# ------------------------------------------------------------------ 5. the batched big tile
def test_batched_sweep_on_the_big_tile(monkeypatch, tmp_path):
    """g3_gp_factor_batched, B = 3 SE members at N = 640, d = 2, with G3_COOP_MAX_N=0 G3_GEMM_BIG_MIN=1: the lock-step sweep
    with the member in grid.y on the 128 x 128 tile.  Every member's logdet, quad and a against SciPy on the oracle's
    covariance (1e-9 / 1e-8) and against the default context (64 x 64 tile) at 1e-11 relative."""
    from oracle import g3_oracle as orc
    from g3py_amd import _lib
    from g3py_amd.device import compile_spec
    rng = np.random.default_rng(640)
    N, d, B = 640, 2, 3
    X = rng.uniform(0, N ** (1.0 / d), (N, d))
    y = np.sin(X.sum(1) / 2) + 0.1 * rng.standard_normal(N)
    specs = [orc.with_noise(('SE', v, np.array(r), None), nz) for v, r, nz in
             ((1.0, [1.0, 1.0], 0.1), (1.3, [0.7, 1.2], 0.05), (0.8, [1.4, 0.9], 0.2))]
    progs = [compile_spec(s, d) for s in specs]
    Np = _lib.roundup(N)
    kstride = (Np + _lib.G3_RHS_PAD) * Np
    res = {}
    for name, knobs in (('default', {}), ('big', {'G3_COOP_MAX_N': 0, 'G3_GEMM_BIG_MIN': 1})):
        with variant_context(monkeypatch, tmp_path, **knobs) as run:
            dev = run.dev
            K = dev.alloc(B * (Np + _lib.G3_RHS_PAD), Np, np.float64)
            W = dev.alloc(B * Np, _lib.G3_PAD, np.float64)
            a = dev.alloc(B, Np, np.float64)
            st = dev.gp_factor_batched(progs, dev.upload(X), N, d, dev.upload(np.tile(y, (B, 1))), K, kstride, W, a, raw=True)
            res[name] = (st.copy(), dev.download(a, B, N))
        tiles = _tiles(run.log)
        if name == 'big':
            assert (128, 128, 8) in tiles, run.log
        else:
            assert (64, 64, 4) in tiles and (128, 128, 8) not in tiles, run.log
    (sd, ad), (sb, ab) = res['default'], res['big']
    assert np.all(sd[:, 2:] == 0) and np.all(sb[:, 2:] == 0)              # nothing non-finite, no retry, no failed pivot
    for b, spec in enumerate(specs):
        L = scipy.linalg.cholesky(orc.tt_to_num(orc.kernel_cov(spec, X)), lower=True)
        a_ref = scipy.linalg.solve_triangular(L, y, lower=True)
        for st_, a_ in ((sd, ad), (sb, ab)):
            assert abs(st_[b, 0] - np.log(np.diag(L)).sum()) <= 1e-9 * max(1.0, abs(np.log(np.diag(L)).sum())), b
            assert abs(st_[b, 1] - a_ref.dot(a_ref)) <= 1e-9 * max(1.0, a_ref.dot(a_ref)), b
            np.testing.assert_allclose(a_[b], a_ref, rtol=1e-8, atol=1e-8)
        np.testing.assert_allclose(sb[b, :2], sd[b, :2], rtol=1e-11, atol=0)
        assert np.abs(ab[b] - ad[b]).max() <= 1e-11 * np.abs(ad[b]).max(), b
