"""GPU tests of the MEMORY contracts of the C ABI (include/g3hip.h): what each entry point may read, what it must write,
and what it must leave alone.  Every case runs with the same seeded inputs

  clean    on the default context: inputs without slack, outputs and workspaces zero-filled (twice: clean == clean first,
           so that a difference below is attributable to the memory);
  hostile  on a context that larger problems have used (hostile_memory.dirty_device): every input embedded in NaN, every
           output and workspace NaN inside its documented extent and a canary band outside it, leading dimensions wider
           than the width

and asserts (a) equal return codes and host outputs, bit for bit; (b) equal bits and no NaN on the documented output
region; (c) nothing outside the documented extent written.  No tolerance anywhere: the library has no floating-point
atomics and its sums have a fixed order.

The second part tests the reduction and fix-up kernels of g3_api.hip directly, against math.fsum."""
import ctypes as C
import math

import numpy as np
import pytest

import hostile_memory as hm
from hostile_memory import CANARY_BYTE, NAN_BYTE, reduction_bound

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
D = 3
# contexts read their knobs when they are created: one (clean, dirty) pair per setting
MODES = {'default': {}, 'interp': {'G3_GRAM_JIT': 0}, 'coop': {'G3_COOP_MIN_BATCH': 2, 'G3_COOP_MAX_N': 1024},
         'sweep': {'G3_COOP_MIN_BATCH': 2, 'G3_COOP_MAX_N': 0}}


@pytest.fixture(scope='module')
def dev():
    import g3py_amd as g3
    return g3.Device.default()


@pytest.fixture(scope='module')
def pairs(dev):
    import g3py_amd as g3
    made = {}

    def get(mode):
        if mode not in made:
            if mode == 'default':
                clean = dev
            else:
                with hm.environment(**MODES[mode]):
                    clean = g3.Device(0)
            made[mode] = (clean, hm.dirty_device(**MODES[mode]))
        return made[mode]
    yield get
    for clean, dirty in made.values():
        dirty.close()
        if clean is not dev:
            clean.close()


def _code(dt):
    from g3py_amd import _lib
    return _lib.dtype_code(dt)


def _rup(n):
    return (int(n) + 127) // 128 * 128


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _iptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


# --------------------------------------------------------------------------------------- one side of a case
class Side:
    """The operands of one run of a case: `hostile` False -> plain buffers (inputs without slack, outputs zeroed), True ->
    every buffer embedded (hostile_memory.embed).  Remembers what it handed out; collect() downloads it all and, on the
    hostile side, checks that nothing outside each buffer's written mask changed."""

    def __init__(self, dev, hostile):
        self.dev, self.hostile = dev, hostile
        self.lib, self.ctx = dev.lib, dev.ctx
        self.arrays, self.hosts, self.notes = {}, {}, {}

    def _ld(self, cols, dt, compact, ld):
        if ld is not None:
            return ld                   # a leading dimension that is the case's own (an odd one): the same on both sides
        if not self.hostile or compact:
            return cols
        return cols + hm.slack(dt)

    def inp(self, name, array, dt, mask=None, compact=False):
        """an input (mask None: nothing of it may change) or an in/out operand (mask: what may; True = all of it); `array`
        is float64 and may hold NaN where the contract says the entry is not read.  The clean side's allocation is GUARD
        zeroed rows longer than the array, so that no kernel under test can leave it either."""
        array = np.atleast_2d(np.asarray(array, dtype=np.float64)).astype(dt)
        rows, cols = array.shape
        if mask is True:
            mask = np.ones((rows, cols), bool)
        if self.hostile:
            d, owner = hm.embed(self.dev, array, rows, self._ld(cols, dt, compact, None), dt, NAN_BYTE)
        else:
            d, owner = self.dev.upload(array, pad_rows=rows + hm.GUARD), None
        self.arrays[name] = (d, owner, mask, rows)
        return d

    def out(self, name, rows, cols, dt, mask=True, compact=False, ld=None, rows_total=None):
        """an output or workspace of the documented extent rows x cols; rows_total > rows: further rows behind it that
        belong to the caller (a member slot that is not part of the batch) and carry the canary"""
        total = rows if rows_total is None else rows_total
        if mask is True:
            mask = np.ones((rows, cols), bool)
        if self.hostile:
            d, owner = hm.embed(self.dev, (rows, cols), total, self._ld(cols, dt, compact, ld), dt, CANARY_BYTE)
        else:
            d, owner = self.dev.alloc(total + hm.GUARD, cols, dt, ld=self._ld(cols, dt, compact, ld), zero=True), None
        self.arrays[name] = (d, owner, mask, rows)
        return d

    def host(self, name, n, dtype):
        """a host out-array of n entries: a slice of a longer array with a canary tail"""
        a = np.full(n + 16, hm.fill_value(CANARY_BYTE, dtype), dtype=dtype)
        self.hosts[name] = (a, n)
        return a

    def ok(self, rc, what):
        assert rc == 0, '%s returned %d (%s)' % (what, rc, (self.lib.g3_last_error(self.ctx) or b'').decode())

    def note(self, name, value):
        self.notes[name] = np.atleast_1d(np.asarray(value))

    def collect(self):
        self.dev.sync()
        res = {}
        for name, (d, owner, mask, rows) in self.arrays.items():          # the documented extent of each buffer
            if owner is None:
                res[name] = self.dev.download(d, rows)
            else:
                res[name] = owner.block(hm.check_untouched(self.dev, owner, mask, what=name))[:rows]
        for name, (a, n) in self.hosts.items():
            assert hm.first_difference(a[n:], np.full(16, hm.fill_value(CANARY_BYTE, a.dtype), a.dtype)) is None, \
                '%s: the host array was written past its %d entries' % (name, n)
            res['host:' + name] = a[:n].copy()
        for name, v in self.notes.items():
            res['host:' + name] = v
        return res


def _compare(x, y, regions, what):
    assert set(x) == set(y)
    for name in x:
        if name.startswith('host:'):
            at = hm.first_difference(x[name], y[name])
            assert at is None, '%s: host output %s differs at %s: %r != %r' % (what, name, at, x[name], y[name])
        elif name in regions:
            hm.same_bits(x[name], y[name], regions[name], '%s: %s' % (what, name))


def run_case(pairs, mode, case, *args):
    """clean, clean again, hostile; returns (clean results, hostile results, regions)"""
    clean, dirty = pairs(mode)

    def once(dev, hostile):
        side = Side(dev, hostile)
        regions = case(side, *args)
        return side.collect(), regions
    a, regions = once(clean, False)
    b, _ = once(clean, False)
    _compare(a, b, regions, 'clean vs clean')
    h, _ = once(dirty, True)
    _compare(a, h, regions, 'clean vs hostile')
    return a, h, regions


# --------------------------------------------------------------------------------------- seeded problems, computed once
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def _points(n, seed):
    return _cached(('X', n, seed), lambda: np.random.default_rng(seed).uniform(0, 3, (n, D)))


def _spd(n):
    def make():
        rng = np.random.default_rng(n)
        B = rng.standard_normal((n, max(8, n // 4)))
        return B @ B.T / B.shape[1] + np.eye(n)
    return _cached(('spd', n), make)


def _chol(n):
    return _cached(('chol', n), lambda: np.linalg.cholesky(_spd(n)))


def _poison_upper(side, A):
    """the strict upper triangle: NaN on the hostile side (the contract says it is not read), as given on the clean side"""
    if not side.hostile:
        return A
    return np.where(hm.tril_mask(A.shape[0], cols=A.shape[1]), A, np.nan)


RATE = np.array([0.8, 1.0, 1.3])
SPECS = {
    'table': ('sum', ('SE', 1.3, RATE, None), ('NOISE', 0.1)),
    'generated': ('sum', ('prod', ('SE', 1.3, RATE, None), ('COS', 0.7, np.array([0.2, 0.3, 0.1]), None)), ('WN', 0.1, None)),
}
PATH_OF = {'table': ('default', 'table', 'table'), 'generated': ('default', 'generated', 'generated'),
           'interpreted': ('interp', 'generated', 'interpreted')}       # name -> (mode, spec, counter that must move)


def _prog(name):
    from g3py_amd.device import compile_spec
    return compile_spec(SPECS[name], D)


def _cross_prog(name):
    from g3py_amd.device import compile_spec
    return compile_spec(SPECS[name][1], D)


# --------------------------------------------------------------------------------------- Gram assembly
GRAM_VARIANTS = {'factor': 1 | 2 | 4, 'plain': 0, 'cross': 2, 'oddld': 4}


def case_gram(side, spec, n, dt, variant):
    from g3py_amd import _lib
    prog = _prog(spec)
    flags = GRAM_VARIANTS.get(variant, 0)
    X = side.inp('X', _points(n, 1), dt)
    n1pad = _rup(n)
    if variant == 'cross':
        n2 = 65
        X2 = side.inp('X2', _points(n2, 2), dt)
        n2pad = 128
    elif variant == 'blockcol':
        X2, n2, n2pad = None, n, 128
    else:
        X2, n2, n2pad = None, n, n1pad
    mask = hm.lower_tile_mask(n1pad, n2pad) if flags & _lib.G3_GRAM_LOWER else True
    ld = n2pad + (65 if np.dtype(dt) == np.float64 else 97) if variant == 'oddld' else None
    K = side.out('K', n1pad, n2pad, dt, mask=mask, ld=ld)
    if variant == 'oddld' and side.hostile:
        assert K.ld & 1
    before = side.dev.gram_path_stats()
    side.ok(side.lib.g3_gram(side.ctx, C.byref(prog), X.ptr, n, X.ld, X2.ptr if X2 is not None else None,
                             n2 if X2 is not None else 0, X2.ld if X2 is not None else 0, D, _code(dt), K.ptr, K.ld, n1pad,
                             n2pad, flags), 'g3_gram')
    after = side.dev.gram_path_stats()
    side.note('path', [after[k] - before[k] for k in COUNTERS])
    return {'K': None if mask is True else mask}


COUNTERS = ('table', 'generated', 'interpreted')


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('variant', ['factor', 'plain', 'cross'])
@pytest.mark.parametrize('n', [1, 65, 130, 257])
@pytest.mark.parametrize('path', ['table', 'generated', 'interpreted'])
def test_gram(pairs, path, n, variant, dt):
    """g3_gram, one program per Gram path: every element of [0, n1pad) x [0, n2pad) is written (with G3_GRAM_LOWER: of the
    64 x 128 tiles on or below the diagonal), none beyond; the padding is exactly 0, or the identity with PAD_EYE; X beyond
    its n rows and d columns is not read"""
    _gram_check(pairs, path, n, variant, dt)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('variant,n', [('blockcol', 257), ('oddld', 130), ('oddld', 257)])
@pytest.mark.parametrize('path', ['table', 'generated'])
def test_gram_block_column_and_odd_leading_dimension(pairs, path, n, variant, dt):
    """the symmetric case with n2pad = 128 < n1 (a block column, as the multi-GPU path stores it), and an odd ldk, on which
    the store path falls back from two-element to scalar stores"""
    _gram_check(pairs, path, n, variant, dt)


def _gram_check(pairs, path, n, variant, dt):
    mode, spec, counter = PATH_OF[path]
    a, h, regions = run_case(pairs, mode, case_gram, spec, n, dt, variant)
    assert list(h['host:path']) == [int(k == counter) for k in COUNTERS], (counter, h['host:path'])
    K = h['K']
    rows, cols = np.indices(K.shape)
    n2 = 65 if variant == 'cross' else n
    pad = (rows >= n) | (cols >= n2)
    if regions['K'] is not None:
        pad &= regions['K']
    eye = GRAM_VARIANTS.get(variant, 0) & 4
    want = np.where((rows == cols) & bool(eye), 1.0, 0.0).astype(dt)
    at = hm.first_difference(K, want, pad)
    assert at is None, 'padding element %s holds %r' % (at, K[at])


def case_gram_rows(side, N, row0, nrows, dt, flags):
    prog = _prog('table')
    X = side.inp('X', _points(N, 3), dt)
    K = side.out('K', nrows, row0 + nrows, dt)
    side.ok(side.lib.g3_gram_rows(side.ctx, C.byref(prog), X.ptr, N, X.ld, D, row0, nrows, _code(dt), K.ptr, K.ld, flags),
            'g3_gram_rows')
    return {'K': None}


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('row0,nrows,flags', [(128, 172, 2), (0, 300, 2), (128, 256, 2 | 4), (0, 384, 0)])
def test_gram_rows(pairs, row0, nrows, flags, dt):
    """g3_gram_rows at N = 300: the nrows x (row0 + nrows) block is written and nothing else; rows / columns beyond N are 0,
    or the identity with PAD_EYE"""
    N = 300
    a, h, _ = run_case(pairs, 'default', case_gram_rows, N, row0, nrows, dt, flags)
    K = h['K']
    rows, cols = np.indices(K.shape)
    pad = (rows + row0 >= N) | (cols >= N)
    want = np.where((rows + row0 == cols) & bool(flags & 4), 1.0, 0.0).astype(dt)
    at = hm.first_difference(K, want, pad)
    assert at is None, 'padding element %s holds %r' % (at, K[at])


def case_gram_diag(side, n, dt, spec):
    prog = _prog(spec)
    X = side.inp('X', _points(n, 4), dt)
    out = side.out('diag', 1, n, dt)
    side.ok(side.lib.g3_gram_diag(side.ctx, C.byref(prog), X.ptr, n, X.ld, D, _code(dt), out.ptr), 'g3_gram_diag')
    return {'diag': None}


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('spec', ['table', 'generated'])
def test_gram_diag(pairs, spec, dt):
    """g3_gram_diag at n = 130: n entries, the ones from n on untouched"""
    run_case(pairs, 'default', case_gram_diag, 130, dt, spec)


# --------------------------------------------------------------------------------------- factorisation and solves
def _block_inverses(L):
    n = L.shape[0]
    return np.concatenate([np.tril(np.linalg.inv(L[k:k + 128, k:k + 128])) for k in range(0, n, 128)])


def case_potrf(side, n, dt, variant):
    A = side.inp('A', _poison_upper(side, _spd(n)), dt, mask=hm.tril_mask(n))
    W = None if variant == 'ctx' else side.out('invd', n, 128, dt, compact=True)
    if variant == 'nowait':
        acc = side.dev.alloc(1, 1, np.float32, zero=True)
        side.ok(side.lib.g3_potrf_nowait(side.ctx, A.ptr, n, A.ld, _code(dt), W.ptr, acc.ptr), 'g3_potrf_nowait')
        side.dev.sync()
        side.note('info', side.dev.download(acc).view(np.int32))
    else:
        info = C.c_int(-1)
        side.ok(side.lib.g3_potrf(side.ctx, A.ptr, n, A.ld, _code(dt), W.ptr if W is not None else None, C.byref(info)),
                'g3_potrf')
        side.note('info', info.value)
    return {'A': hm.tril_mask(n), 'invd': None}


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('variant', ['given', 'ctx', 'nowait'])
@pytest.mark.parametrize('n', [128, 256, 384, 1152])
def test_potrf(pairs, n, variant, dt):
    """g3_potrf / g3_potrf_nowait: the strict upper triangle is NaN on entry and still that NaN afterwards, and the factor
    does not know; invd_dev starts as NaN and ends as n / 128 fully defined inverses whose strict upper triangles are
    exactly 0 (what g3_gp_cross_batched relies on), with nothing written behind them; invd_dev = NULL uses the context's
    own buffer, which larger factorisations have used"""
    a, h, _ = run_case(pairs, 'default', case_potrf, n, dt, variant)
    assert h['host:info'][0] == 0
    if variant != 'ctx':
        W = h['invd'].reshape(n // 128, 128, 128)
        assert not np.isnan(W).any() and np.count_nonzero(np.triu(W, 1)) == 0
        assert (np.diagonal(W, axis1=1, axis2=2) > 0).all()


def case_trsm_rlt(side, n, m, dt, given):
    L = _chol(n)
    Ld = side.inp('L', _poison_upper(side, L), dt)
    B = _cached(('B', m, n), lambda: np.random.default_rng(m + n).standard_normal((m, n)))
    Bd = side.inp('B', B, dt, mask=True)
    W = side.inp('invd', _cached(('Linv', n), lambda: _block_inverses(L)), dt, compact=True) if given else None
    side.ok(side.lib.g3_trsm_rlt(side.ctx, Ld.ptr, n, Ld.ld, Bd.ptr, m, Bd.ld, _code(dt), W.ptr if given else None),
            'g3_trsm_rlt')
    return {'B': None}


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('given', [False, True])
@pytest.mark.parametrize('n,m', [(128, 128), (384, 256), (1152, 128)])
def test_trsm_rlt(pairs, n, m, given, dt):
    """g3_trsm_rlt with L's strict upper triangle NaN: B is solved in place and its band untouched, with the block
    inverses given or computed into the context's (used) buffer"""
    run_case(pairs, 'default', case_trsm_rlt, n, m, dt, given)


def _block_tril(n, upper=False):
    b = np.arange(n) // 128
    return b[:, None] <= b[None, :] if upper else b[:, None] >= b[None, :]


def case_trtri_full(side, n, m, dt):
    code = _code(dt)
    A = side.inp('L', _poison_upper(side, _spd(n)), dt, mask=hm.tril_mask(n), compact=True)
    W = side.out('invd', n, 128, dt, compact=True)
    info = C.c_int(-1)
    side.ok(side.lib.g3_potrf(side.ctx, A.ptr, n, A.ld, code, W.ptr, C.byref(info)), 'g3_potrf')
    side.note('info', info.value)
    V = side.out('V', n, n, dt, mask=_block_tril(n), compact=True)
    Vt = side.out('Vt', n, n, dt, mask=_block_tril(n, upper=True), compact=True)
    U = side.out('U', n, n, dt, compact=True)
    side.ok(side.lib.g3_trtri_full(side.ctx, A.ptr, n, W.ptr, V.ptr, Vt.ptr, U.ptr, code), 'g3_trtri_full')
    B = _cached(('B', m, n), lambda: np.random.default_rng(m + n).standard_normal((m, n)))
    Bd = side.inp('B', B, dt)
    X = side.out('X', m, n, dt)
    side.ok(side.lib.g3_trsm_full(side.ctx, V.ptr, n, V.ld, Bd.ptr, m, Bd.ld, X.ptr, X.ld, code), 'g3_trsm_full')
    return {'L': hm.tril_mask(n), 'invd': None, 'V': _block_tril(n), 'X': None}


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('n', [256, 512])
def test_trtri_full_and_trsm_full(pairs, n, dt):
    """g3_trtri_full writes the lower block triangle of V only (V, Vt, U start as NaN), and the one-product solve
    g3_trsm_full does not read the rest of V: X has no NaN and its band is untouched"""
    a, h, _ = run_case(pairs, 'default', case_trtri_full, n, 64, dt)
    assert h['host:info'][0] == 0
    assert np.count_nonzero(np.triu(h['V'], 1)[_block_tril(n)]) == 0        # inside the diagonal blocks: exact zeros


def case_potri(side, n, dt):
    N = n - 28
    L = np.eye(n)
    L[:N, :N] = _chol(N)
    Ld = side.inp('L', _poison_upper(side, L), dt)
    Y = side.out('Y', n, n, dt)
    Ki = side.out('Kinv', n, n, dt)
    code = _code(dt)
    side.ok(side.lib.g3_potri(side.ctx, Ld.ptr, n, Ld.ld, None, code, Y.ptr, Y.ld, Ki.ptr, Ki.ld), 'g3_potri')
    # the chain of g3_gp_dlogp: the kernel-parameter sums read these buffers as they were left, NaN remainder included
    prog = _prog('table')
    gmap = side.dev.grad_layout(prog)
    X = side.inp('X', _points(N, 5), dt)
    al = side.inp('alpha', _cached(('alpha', N), lambda: np.random.default_rng(N).standard_normal(N)), dt)
    s1 = side.host('slots', gmap.nslots, np.float64)
    side.ok(side.lib.g3_gram_grad(side.ctx, C.byref(prog), C.byref(gmap), X.ptr, N, X.ld, D, code, Ki.ptr, Ki.ld, al.ptr,
                                  _dptr(s1)), 'g3_gram_grad')
    s2 = side.host('slots_rows', gmap.nslots, np.float64)
    side.ok(side.lib.g3_gram_grad_rows(side.ctx, C.byref(prog), C.byref(gmap), X.ptr, N, X.ld, D, code, 64, N - 64,
                                       Ki.offset(64), Ki.ld, al.ptr, _dptr(s2)), 'g3_gram_grad_rows')
    return {'Y': np.triu(np.ones((n, n), bool)), 'Kinv': hm.tril_mask(n)}


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('n', [128, 384, 1024])
def test_potri_and_the_gradient_sums_on_its_buffers(pairs, n, dt):
    """g3_potri (n >= 768: the two-stream schedule) with L's strict upper triangle NaN and Y, Kinv starting as NaN: the upper
    triangle of Y and the lower triangle of Kinv are fully defined; g3_gram_grad and g3_gram_grad_rows (row0 = 64) on those
    buffers read the lower triangle of Kinv only"""
    a, h, _ = run_case(pairs, 'default', case_potri, n, dt)
    assert np.isfinite(h['host:slots']).all() and np.isfinite(h['host:slots_rows']).all()


# --------------------------------------------------------------------------------------- the fused hot path
def _gp_problem(N, M, kind):
    def make():
        rng = np.random.default_rng(N + M)
        X = rng.uniform(0, 3, (N, D))
        Xs = rng.uniform(0, 3, (M, D))
        delta = np.sin(X.sum(1) / 2) + 0.1 * rng.standard_normal(N)
        if kind == 'jitter':
            X[1] = X[0]                                  # a duplicated input: singular without noise
        if kind == 'nonfinite':
            X[7, 1] = np.inf
        return X, Xs, delta
    return _cached(('gp', N, M, kind), make)


def _gp_progs(kind):
    from g3py_amd.device import compile_spec
    if kind == 'jitter':
        se = ('SE', 1.0, RATE, None)
        return compile_spec(('sum', se, ('NOISE', 0.0)), D), compile_spec(se, D)
    if kind == 'indefinite':
        # exp(+2 * 17 sin^2), up to 6e14 off a unit diagonal: indefinite beyond the last jitter (1e13) -> the 1e-10 * I
        # fallback, and V = K(Xs, X) * 1e10 still fits fp32
        sin = ('SIN', 1.0, np.array([0.37]), np.array([17.0]), [0])
        return compile_spec(sin, D), compile_spec(sin, D)
    return _prog('table'), _cross_prog('table')


def case_gp(side, N, M, dt, kind, predict):
    code = _code(dt)
    lib, ctx = side.lib, side.ctx
    prog, cross = _gp_progs(kind)
    Xh, Xsh, dh = _gp_problem(N, M, kind)
    Np, Mp = _rup(N), _rup(M)
    X, Xs, delta = side.inp('X', Xh, dt), side.inp('Xs', Xsh, dt), side.inp('delta', dh, dt)
    rows = Np + 128 + (Mp if predict else 0)
    K = side.out('K', rows, Np, dt)
    W = side.out('invd', Np, 128, dt, compact=True)
    a = side.out('a', 1, Np, dt)
    out = side.host('out', 6, np.float64)
    regions = {'K': np.concatenate([hm.tril_mask(Np), np.ones((rows - Np, Np), bool)]), 'invd': None, 'a': None}
    if predict:
        mu, ss = side.out('mu', 1, M, dt), side.out('ss', 1, M, dt)
        side.ok(lib.g3_gp_factor_predict(ctx, C.byref(prog), C.byref(cross), X.ptr, N, X.ld, D, delta.ptr, Xs.ptr, M, Xs.ld, code,
                                         K.ptr, K.ld, W.ptr, a.ptr, mu.ptr, ss.ptr, _dptr(out)), 'g3_gp_factor_predict')
        regions.update(mu=None, ss=None)
    else:
        side.ok(lib.g3_gp_factor(ctx, C.byref(prog), X.ptr, N, X.ld, D, delta.ptr, code, K.ptr, K.ld, W.ptr, a.ptr, _dptr(out)),
                'g3_gp_factor')
    # ---- the consumers of the factor, on the buffers as they were left
    V = side.out('V', Mp, Np, dt)
    mu2, ss2 = side.out('mu2', 1, M, dt), side.out('ss2', 1, M, dt)
    side.ok(lib.g3_gp_cross(ctx, C.byref(cross), Xs.ptr, M, Xs.ld, X.ptr, N, X.ld, D, K.ptr, K.ld, W.ptr, a.ptr, code, V.ptr,
                            V.ld, mu2.ptr, ss2.ptr), 'g3_gp_cross')
    gmap = side.dev.grad_layout(prog)
    Y, Ki, al = side.out('Y', Np, Np, dt), side.out('Kinv', Np, Np, dt), side.out('alpha', 1, Np, dt)
    slots = side.host('slots', max(gmap.nslots, 1), np.float64)
    side.ok(lib.g3_gp_dlogp(ctx, C.byref(prog), C.byref(gmap), X.ptr, N, X.ld, D, K.ptr, K.ld, W.ptr, a.ptr, code, Y.ptr, Y.ld,
                            Ki.ptr, Ki.ld, al.ptr, _dptr(slots)), 'g3_gp_dlogp')
    Y2, al2, kd = side.out('Y2', Np, Np, dt), side.out('alpha2', 1, Np, dt), side.out('kdiag', 1, Np, dt)
    side.ok(lib.g3_gp_loo(ctx, K.ptr, N, K.ld, W.ptr, a.ptr, code, Y2.ptr, Y2.ld, al2.ptr, kd.ptr), 'g3_gp_loo')
    upper = np.triu(np.ones((Np, Np), bool))
    regions.update(V=None, mu2=None, ss2=None, Y=upper, Kinv=hm.tril_mask(Np), alpha=None, Y2=upper, alpha2=None, kdiag=None)
    return regions


def _gp_check(pairs, N, M, dt, kind, predict):
    a, h, _ = run_case(pairs, 'default', case_gp, N, M, dt, kind, predict)
    Np = _rup(N)
    out = h['host:out']
    for name in ('a', 'alpha2', 'kdiag'):
        assert np.count_nonzero(h[name][0, N:Np]) == 0, '%s: entries from N on are not 0' % name
    if kind in ('plain', 'jitter'):
        assert np.isfinite(h['host:slots']).all()
    return out


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('predict', [False, True])
@pytest.mark.parametrize('N,M', [(100, 24), (200, 150), (300, 24), (1100, 150)])
def test_gp_factor_and_the_consumers_of_the_factor(pairs, N, M, predict, dt):
    """g3_gp_factor / g3_gp_factor_predict with the whole tall K buffer, invd, a, mu, ss starting as NaN (the tiles above
    the diagonal of the factor are never written: G3_GRAM_LOWER), then g3_gp_cross, g3_gp_dlogp and g3_gp_loo on the
    buffers as left; a, alpha and kdiag of the leave-one-out call are exactly 0 on [N, Npad)"""
    out = _gp_check(pairs, N, M, dt, 'plain', predict)
    assert out[3] == 0 and out[4] == 0 and out[5] == 0


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('kind', ['jitter', 'nonfinite', 'indefinite'])
def test_gp_factor_jitter_schedule_and_fallback(pairs, kind, dt):
    """the same at (200, 150) through the jitter schedule (duplicated inputs, no noise: tries >= 1), with one non-finite
    input, and through the 1e-10 * I fallback (an indefinite kernel), which rebuild K and re-solve in the same buffers"""
    out = _gp_check(pairs, 200, 150, dt, kind, True)
    if kind == 'jitter':
        assert out[3] >= 1 and out[4] == 0 and out[5] != 0
    if kind == 'indefinite':
        assert out[3] == 20 and out[4] == 1


# --------------------------------------------------------------------------------------- robust factorisation, draws
def _robust_matrix(n, kind):
    def make():
        K = _spd(n).copy()
        if kind == 'jitter':                 # a duplicated row and column, and 1e-3 less on its diagonal: indefinite
            K[3, :], K[:, 3] = K[2, :], K[:, 2]
            K[3, 3] = K[2, 2] - 1e-3
        if kind == 'nonfinite':
            K[n - 1, 0] = K[0, n - 1] = np.nan
        return K
    return _cached(('robust', n, kind), make)


def case_potrf_robust(side, n, dt, kind):
    K = side.inp('K', _robust_matrix(n, kind), dt)
    L = side.out('L', n, n, dt)
    tries, fb, jit = side.host('tries', 1, np.int32), side.host('fb', 1, np.int32), side.host('jitter', 1, np.float64)
    side.ok(side.lib.g3_potrf_robust(side.ctx, K.ptr, K.ld, L.ptr, L.ld, n, _code(dt), 20, _iptr(tries), _iptr(fb), _dptr(jit)),
            'g3_potrf_robust')
    return {'L': None}


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('n,kind', [(7, 'spd'), (100, 'spd'), (129, 'spd'), (300, 'spd'), (129, 'jitter'), (100, 'nonfinite')])
def test_potrf_robust(pairs, n, kind, dt):
    """g3_potrf_robust: K's bytes unchanged, L's strict upper triangle zeroed (L starts as NaN), its band untouched; the
    padded work matrix lives in the context's workspace, which larger problems have used"""
    a, h, _ = run_case(pairs, 'default', case_potrf_robust, n, dt, kind)
    assert np.count_nonzero(np.triu(h['L'], 1)) == 0
    tries, fb = h['host:tries'][0], h['host:fb'][0]
    if kind == 'spd':
        assert (tries, fb) == (0, 0)
    elif kind == 'jitter':
        assert tries >= 1 and fb == 0
    else:
        assert (tries, fb) == (20, 1)


def case_gp_sample(side, M, S, dt):
    Mp = _rup(M)
    L = np.zeros((Mp, Mp))
    L[:M, :M] = _chol(M)
    Ld = side.inp('L', L, dt)
    rng = np.random.default_rng(M + S)
    loc = np.ascontiguousarray(rng.standard_normal(M), dtype=dt)
    Z = np.ascontiguousarray(rng.standard_normal((M, S)), dtype=dt)
    out = side.host('out', M * S, dt)
    side.ok(side.lib.g3_gp_sample(side.ctx, Ld.ptr, M, Ld.ld, loc.ctypes.data, Z.ctypes.data, S, _code(dt), out.ctypes.data),
            'g3_gp_sample')
    return {}


@pytest.mark.parametrize('dt', DTYPES)
def test_gp_sample(pairs, dt):
    """g3_gp_sample at M = 130, S = 3: the M x S draws and not an entry more of the host array"""
    a, h, _ = run_case(pairs, 'default', case_gp_sample, 130, 3, dt)
    assert np.isfinite(h['host:out']).all()


# --------------------------------------------------------------------------------------- copies and fix-ups
def _dirty_matrix(n):
    def make():
        rng = np.random.default_rng(n)
        A = rng.standard_normal((n, n))
        A[0, n - 1], A[n - 1, 0], A[n // 2, n // 2] = np.nan, np.inf, -np.inf
        return A
    return _cached(('dirty', n), make)


def case_small(side, op, n, dt):
    code = _code(dt)
    lib, ctx = side.lib, side.ctx
    diag = np.eye(n, dtype=bool)
    if op == 'copy2d':
        src = side.inp('src', _spd(n), dt)
        dst = side.out('dst', n, n, dt)
        side.ok(lib.g3_copy2d(ctx, dst.ptr, dst.ld, src.ptr, src.ld, n, n, code), 'g3_copy2d')
        return {'dst': None}
    if op == 'scrub':
        A = side.inp('A', _dirty_matrix(n), dt, mask=True)
        side.ok(lib.g3_scrub(ctx, A.ptr, n, n, A.ld, code), 'g3_scrub')
    elif op == 'cov_lift':
        K = _spd(n).copy()
        K[n - 1, n - 1] = -0.25
        A = side.inp('A', K, dt, mask=diag)
        side.ok(lib.g3_cov_lift(ctx, A.ptr, n, A.ld, code), 'g3_cov_lift')
    else:
        A = side.inp('A', _spd(n), dt, mask=diag)
        side.ok(lib.g3_diag_add(ctx, A.ptr, n, A.ld, code, 0.375), 'g3_diag_add')
    return {'A': None}


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('n', [3, 130])
@pytest.mark.parametrize('op', ['copy2d', 'scrub', 'cov_lift', 'diag_add'])
def test_copies_and_fixups_change_only_their_rectangle_or_diagonal(pairs, op, n, dt):
    """g3_copy2d, g3_scrub, g3_cov_lift, g3_diag_add: only the rectangle / the diagonal changes; the NaN around g3_scrub's
    matrix stays NaN"""
    a, h, _ = run_case(pairs, 'default', case_small, op, n, dt)
    if op == 'copy2d':
        assert hm.first_difference(h['dst'], _spd(n).astype(dt)) is None
    elif op == 'scrub':
        from oracle import g3_oracle as orc
        assert hm.first_difference(h['A'], orc.tt_to_num(_dirty_matrix(n).astype(dt))) is None
    elif op == 'diag_add':
        want = _spd(n).astype(dt)
        want[np.eye(n, dtype=bool)] += dt(0.375)
        assert hm.first_difference(h['A'], want) is None
    else:
        from oracle import g3_oracle as orc
        K = _spd(n).copy()
        K[n - 1, n - 1] = -0.25
        assert hm.first_difference(h['A'], orc.tt_to_cov(K.astype(dt))) is None


# --------------------------------------------------------------------------------------- the reductions, directly
def _embedded(dev, array, dt):
    """a matrix / vector on the device with ld > width and NaN around it"""
    array = np.atleast_2d(np.asarray(array, dtype=np.float64)).astype(dt)
    view, owner = hm.embed(dev, array, array.shape[0], array.shape[1] + hm.slack(dt), dt, NAN_BYTE)
    return view, owner


def _diag_matrix(n, dt, special, seed):
    """an n x n matrix of NaN but for its diagonal (nothing else may be read), the vector a, and the diagonal / a as stored"""
    rng = np.random.default_rng(seed)
    diag = np.exp(rng.uniform(-3, 3, n))
    a = rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 2, n)
    at = (n * 2) // 3
    if special == 'nan':
        diag[at] = a[n // 2] = np.nan
    elif special == 'inf':
        diag[at] = a[n // 2] = np.inf
    elif special == 'nonpositive':
        diag[at] = -0.5
    A = np.full((n, n), np.nan)
    A[np.arange(n), np.arange(n)] = diag
    return A, a, diag.astype(dt).astype(np.float64), a.astype(dt).astype(np.float64)


SPECIALS = ['none', 'nan', 'inf', 'nonpositive']


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('special', SPECIALS)
@pytest.mark.parametrize('n', [1, 63, 1023, 1024, 1025, 2049])
def test_logp_terms_against_fsum(dev, n, special, dt):
    """g3_logp_terms around the 1024-thread stride and the 16-wave combine, with and without a: the two sums within
    n * 2^-52 * sum |terms| of math.fsum over the inputs as stored (the kernel accumulates in double), the two counts
    exact; a NaN, an Inf and a non-positive diagonal entry each in a case of its own.  Everything but the diagonal is NaN."""
    A, a, dg, av = _diag_matrix(n, dt, special, n)
    Ad, oa = _embedded(dev, A, dt)
    ad, ob = _embedded(dev, a, dt)
    with np.errstate(all='ignore'):
        logs = np.log(dg)
    squares = av * av
    for with_a in (True, False):
        got = dev.logp_terms(Ad, n, ad if with_a else None)
        print('logp_terms n=%d %s a=%d: %r' % (n, special, with_a, got))
        for k, terms in ((0, logs), (1, squares if with_a else np.zeros(0))):
            if np.isfinite(terms).all():
                ref = math.fsum(terms)
                assert abs(got[k] - ref) <= reduction_bound(terms, n), (k, got[k], ref)
            elif np.isnan(terms).any() or (np.isinf(terms).any() and len(set(np.sign(terms[np.isinf(terms)]))) > 1):
                assert np.isnan(got[k]), (k, got[k])
            else:
                assert got[k] == terms[np.isinf(terms)][0], (k, got[k])
        assert got[2] == (np.count_nonzero(~np.isfinite(av)) if with_a else 0)
        assert got[3] == np.count_nonzero(~(dg > 0) | np.isinf(dg))
    hm.check_untouched(dev, oa)
    hm.check_untouched(dev, ob)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('special', SPECIALS)
@pytest.mark.parametrize('n', [1, 63, 1023, 1024, 1025, 2049])
def test_diag_stats_against_fsum(dev, n, special, dt):
    """g3_diag_stats: min and max exact and NaN-propagating (numpy.min / max), the mean within the bound of its sum"""
    A, _, dg, _ = _diag_matrix(n, dt, special, n + 7)
    Ad, oa = _embedded(dev, A, dt)
    out = (C.c_double * 3)()
    assert dev.lib.g3_diag_stats(dev.ctx, Ad.ptr, n, Ad.ld, _code(dt), out) == 0
    got = list(out)
    print('diag_stats n=%d %s: %r' % (n, special, got))
    if np.isnan(dg).any():
        assert np.isnan(got[0]) and np.isnan(got[2])            # as numpy.min / numpy.max
    else:
        assert got[0] == dg.min() and got[2] == dg.max()
    if np.isfinite(dg).all():
        ref = math.fsum(dg)
        assert abs(got[1] * n - ref) <= reduction_bound(dg, n) + 2.0 ** -52 * abs(ref), (got[1], ref / n)   # + the division
    else:
        assert np.isnan(got[1]) if np.isnan(dg).any() else got[1] == np.inf
    hm.check_untouched(dev, oa)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('use', ['both', 'no_a', 'no_dot', 'no_ss'])
@pytest.mark.parametrize('m,n', [(1, 1), (5, 255), (5, 256), (5, 257), (130, 1000)])
def test_rows_dot_ss_against_fsum(dev, m, n, use, dt):
    """g3_rows_dot_ss around the 256-thread stride, with a, with a = NULL, with dot or ss NULL: each entry within
    n * 2^-52 * sum |terms| of math.fsum plus, for fp32 outputs, one rounding of the stored result (2^-24 |ref|); the outputs
    start as NaN inside their m entries and nothing is written behind them"""
    rng = np.random.default_rng(m * 1000 + n)
    V = (rng.standard_normal((m, n)) * 10.0 ** rng.uniform(-2, 2, (m, n))).astype(dt)
    a = rng.standard_normal(n).astype(dt)
    Vd, ov = _embedded(dev, V, dt)
    ad, oa = _embedded(dev, a, dt)
    dot, od = hm.embed(dev, (1, m), 1, m + hm.slack(dt), dt, CANARY_BYTE)
    ss, os_ = hm.embed(dev, (1, m), 1, m + hm.slack(dt), dt, CANARY_BYTE)
    dev.rows_dot_ss(Vd, m, n, None if use == 'no_a' else ad, None if use == 'no_dot' else dot, None if use == 'no_ss' else ss)
    dev.sync()
    V64, a64 = V.astype(np.float64), a.astype(np.float64)
    store = 2.0 ** -24 if np.dtype(dt) == np.float32 else 2.0 ** -53
    worst = 0.0
    for name, arr, owner, terms_of in (('dot', dot, od, lambda i: V64[i] * a64), ('ss', ss, os_, lambda i: V64[i] * V64[i])):
        written = use != 'no_' + name
        whole = hm.check_untouched(dev, owner, np.ones((1, m), bool) if written else None, what=name)
        if not written:
            continue
        got = owner.block(whole)[0].astype(np.float64)
        if name == 'dot' and use == 'no_a':
            continue                        # a = NULL: the dot product has no second operand, its value is not specified
        for i in range(m):
            terms = terms_of(i)
            ref = math.fsum(terms)
            bound = reduction_bound(terms, n) + store * abs(ref)
            worst = max(worst, abs(got[i] - ref) / bound if bound else 0.0)
            assert abs(got[i] - ref) <= bound, (name, i, got[i], ref, bound)
    print('rows_dot_ss m=%d n=%d %s: worst error / bound %.3f' % (m, n, use, worst))
    hm.check_untouched(dev, ov)
    hm.check_untouched(dev, oa)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('case', ['zero', 'tiny_positive', 'negative', 'nan'])
@pytest.mark.parametrize('n', [3, 130, 1025])
def test_cov_lift_against_the_oracle(dev, n, case, dt):
    """g3_cov_lift (after g3_scrub, as its contract says) == oracle tt_to_cov, exactly: the lift is 1e-6f - min in the
    matrix's dtype, applied iff !(min > 0) -- min = 0 exactly, min tiny and positive (no lift), a negative minimum, and a NaN
    diagonal entry (which tt_to_num turns into 0); only the diagonal changes"""
    from oracle import g3_oracle as orc
    rng = np.random.default_rng(n)
    K = rng.standard_normal((n, n))
    K[np.arange(n), np.arange(n)] = rng.uniform(0.5, 2.0, n)
    K[n // 2, n // 2] = {'zero': 0.0, 'tiny_positive': 1e-30, 'negative': -0.75, 'nan': np.nan}[case]
    K = K.astype(dt)
    Kd, owner = hm.embed(dev, K, n, n + hm.slack(dt), dt, NAN_BYTE)
    dev.scrub(Kd, n, n)
    dev.cov_lift(Kd, n)
    dev.sync()
    mask = np.eye(n, dtype=bool) | np.isnan(K)              # the diagonal, and what the scrub replaced
    got = owner.block(hm.check_untouched(dev, owner, mask))
    want = orc.tt_to_cov(K)
    assert want.dtype == K.dtype
    at = hm.first_difference(got, want)
    assert at is None, (at, got[at], want[at])
    if case == 'tiny_positive':
        assert hm.first_difference(got, K) is None


# --------------------------------------------------------------------------------------- chains: the batched entry points
B = 5
FAILS = 2          # this member's first factorisation fails: duplicated inputs, unit variance, no noise
HYP = [(1.3, 0.9, 0.10), (0.8, 1.2, 0.05), (1.0, 1.0, 0.0), (1.6, 0.7, 0.20), (1.1, 1.1, 0.15)]      # var, rate scale, noise
CHAIN = {100: 'default', 200: 'default', 300: None}      # N -> mode (300: 'coop' and 'sweep')


def _chain_problem(N):
    def make():
        rng = np.random.default_rng(N)
        X = rng.uniform(0, 3, (N, D))
        X[1] = X[0]
        Xs = rng.uniform(0, 3, (150, D))
        deltas = np.sin(X.sum(1) / 2)[None, :] + 0.1 * rng.standard_normal((B, N))
        return X, Xs, deltas
    return _cached(('chain', N), make)


def _chain_progs():
    from g3py_amd import _lib
    from g3py_amd.device import compile_spec
    progs = [compile_spec(('sum', ('SE', v, r * RATE, None), ('NOISE', nz)), D) for v, r, nz in HYP]
    cross = [compile_spec(('SE', v, r * RATE, None), D) for v, r, nz in HYP]
    return (_lib.KernelProg * B)(*progs), (_lib.KernelProg * B)(*cross), progs


def _chain_fields():
    from g3py_amd.device import Rows, compile_spec_rows
    rows = lambda a: np.asarray(a, dtype=np.float64).view(Rows)
    var, rate, nz = (np.array(c) for c in zip(*HYP))
    spec_rows = ('sum', ('SE', rows(var), rows(rate[:, None] * RATE[None, :]), None), ('NOISE', rows(nz)))
    spec0 = ('sum', ('SE', var[0], rate[0] * RATE, None), ('NOISE', nz[0]))
    return compile_spec_rows(spec_rows, spec0, D, B)


def _stack(one, members, slot_rows):
    """a per-member mask (rows x cols) repeated over member slots of slot_rows rows"""
    out = np.zeros((members * slot_rows, one.shape[1]), bool)
    for b in range(members):
        out[b * slot_rows:b * slot_rows + one.shape[0]] = one
    return out


def case_chain(side, N, dt, abi):
    code = _code(dt)
    lib, ctx = side.lib, side.ctx
    arr, cross, progs = _chain_progs()
    Xh, Xsh, dh = _chain_problem(N)
    Np, slot = _rup(N), _rup(N) + 128
    X, Xs, delta = side.inp('X', Xh, dt), side.inp('Xs', Xsh, dt), side.inp('delta', dh, dt)
    # every per-member buffer has a sixth member slot behind the batch that belongs to the caller
    K = side.out('K', B * slot, Np, dt, rows_total=(B + 1) * slot)
    W = side.out('invd', B * Np, 128, dt, compact=True, rows_total=(B + 1) * Np)
    a = side.out('a', B, Np, dt, compact=True, rows_total=B + 1)
    out = side.host('out', 6 * B, np.float64)
    kstride = slot * K.ld
    if abi == 'fields':
        tmpl, offs, fields = _chain_fields()
        side.ok(lib.g3_gp_factor_batched_fields(ctx, C.byref(tmpl), B, fields.ctypes.data, offs.ctypes.data, len(offs), X.ptr, N,
                                                X.ld, D, delta.ptr, delta.ld, code, K.ptr, K.ld, kstride, W.ptr, a.ptr,
                                                _dptr(out)), 'g3_gp_factor_batched_fields')
    else:
        side.ok(lib.g3_gp_factor_batched(ctx, arr, B, X.ptr, N, X.ld, D, delta.ptr, delta.ld, code, K.ptr, K.ld, kstride, W.ptr,
                                         a.ptr, _dptr(out)), 'g3_gp_factor_batched')
    lower, upper = hm.tril_mask(Np), np.triu(np.ones((Np, Np), bool))
    regions = {'K': _stack(lower, B + 1, slot)[:B * slot], 'invd': None, 'a': None}
    # ---- the consumers, on the buffers as they were left
    for M in (24, 150):
        Mp = _rup(M)
        valid = np.zeros((B, Mp), bool)
        valid[:, :M] = True
        mu, ss, kd = (side.out('%s%d' % (nm, M), B, Mp, dt, compact=True, rows_total=B + 1) for nm in ('mu', 'ss', 'kdiag'))
        side.ok(lib.g3_gp_cross_batched(ctx, cross, B, Xs.ptr, M, Xs.ld, X.ptr, N, X.ld, D, K.ptr, K.ld, kstride, W.ptr, a.ptr,
                                        code, mu.ptr, ss.ptr, kd.ptr), 'g3_gp_cross_batched')
        regions.update({'mu%d' % M: valid, 'ss%d' % M: valid, 'kdiag%d' % M: valid})
        S = 3
        rng = np.random.default_rng(N + M)
        loc = np.ascontiguousarray(rng.standard_normal((B, M)), dtype=dt)
        Z = np.ascontiguousarray(rng.standard_normal((B, M, S)), dtype=dt)
        draws = side.host('draws%d' % M, B * M * S, dt)
        Cm = side.out('C%d' % M, B * Mp, Mp, dt, compact=True, rows_total=(B + 1) * Mp)
        Lp = side.out('Lp%d' % M, B * Mp, Mp, dt, compact=True, rows_total=(B + 1) * Mp)
        tries, fb, jit = side.host('tries%d' % M, B, np.int32), side.host('fb%d' % M, B, np.int32), side.host('jit%d' % M, B, np.float64)
        side.ok(lib.g3_gp_draws_batched(ctx, arr, B, Xs.ptr, M, Xs.ld, X.ptr, N, X.ld, D, K.ptr, K.ld, kstride, W.ptr, a.ptr, code,
                                        1, loc.ctypes.data, Z.ctypes.data, S, draws.ctypes.data, Cm.ptr, Lp.ptr, 20, _iptr(tries),
                                        _iptr(fb), _dptr(jit)), 'g3_gp_draws_batched')
        inner = np.zeros((Mp, Mp), bool)
        inner[:M, :M] = hm.tril_mask(M)
        regions.update({'C%d' % M: _stack(inner, B, Mp), 'Lp%d' % M: None})
    gmap = side.dev.grad_layout(progs[0])
    member_rows = _stack(np.ones((Np, Np), bool), B + 1, slot)[:B * slot]
    Y = side.out('Y', B * slot, Np, dt, mask=member_rows, rows_total=(B + 1) * slot)
    Ki = side.out('Kinv', B * slot, Np, dt, mask=member_rows, rows_total=(B + 1) * slot)
    assert Y.ld == K.ld and Ki.ld == K.ld
    al = side.out('alpha', B, Np, dt, compact=True, rows_total=B + 1)
    slots = side.host('slots', B * gmap.nslots, np.float64)
    side.ok(lib.g3_gp_dlogp_batched(ctx, arr, B, C.byref(gmap), X.ptr, N, X.ld, D, K.ptr, K.ld, kstride, W.ptr, a.ptr, code, Y.ptr,
                                    Ki.ptr, al.ptr, _dptr(slots)), 'g3_gp_dlogp_batched')
    Yl = side.out('Yl', Np, Np, dt, compact=True) if Np > 256 else None
    al2 = side.out('alpha2', B, Np, dt, compact=True, rows_total=B + 1)
    kd2 = side.out('kdiag2', B, Np, dt, compact=True, rows_total=B + 1)
    side.ok(lib.g3_gp_loo_batched(ctx, B, K.ptr, N, K.ld, kstride, W.ptr, a.ptr, code, Yl.ptr if Yl is not None else None,
                                  al2.ptr, kd2.ptr), 'g3_gp_loo_batched')
    regions.update(Y=_stack(upper, B + 1, slot)[:B * slot], Kinv=_stack(lower, B + 1, slot)[:B * slot], alpha=None, alpha2=None,
                   kdiag2=None)
    return regions


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('abi', ['progs', 'fields'])
@pytest.mark.parametrize('N,mode', [(100, 'default'), (200, 'default'), (300, 'coop'), (300, 'sweep')])
def test_chain_factor_and_its_consumers(pairs, N, mode, abi, dt):
    """g3_gp_factor_batched(_fields) with B = 5 -- one workgroup per member (N = 100, 200), the cooperative kernel and the
    lock-step sweep (N = 300) -- where one member fails its first factorisation and is re-run alone, then
    g3_gp_cross_batched and g3_gp_draws_batched (M = 24 and 150, C_dev and Lp_dev given), g3_gp_dlogp_batched and
    g3_gp_loo_batched on the buffers as left.  Every per-member buffer starts as NaN and has a sixth, canary member slot
    behind the batch; entries beyond M of the prediction rows are unspecified: they may be written, they are not compared."""
    a, h, _ = run_case(pairs, mode, case_chain, N, dt, abi)
    Np = _rup(N)
    out = h['host:out'].reshape(B, 6)
    assert out[FAILS, 3] >= 1 and out[FAILS, 5] != 0 and np.count_nonzero(np.delete(out[:, 3:], FAILS, axis=0)) == 0
    for name in ('a', 'alpha2', 'kdiag2'):
        assert np.count_nonzero(h[name][:B, N:Np]) == 0, '%s: entries from N on are not 0' % name
    for M in (24, 150):
        Mp = _rup(M)
        Lp = h['Lp%d' % M][:B * Mp].reshape(B, Mp, Mp)
        outside = ~np.pad(hm.tril_mask(M), (0, Mp - M))
        assert np.count_nonzero(Lp[:, outside]) == 0, 'Lp is not zero outside its M x M lower triangle'
        assert np.isfinite(h['host:draws%d' % M]).all()


def case_potrf_robust_batched(side, n, dt):
    nb, npad = 3, _rup(n)
    Ks = np.concatenate([_robust_matrix(n, kind) for kind in ('spd', 'jitter', 'nonfinite')])
    K = side.inp('K', Ks, dt)
    L = side.out('L', nb * npad, npad, dt, rows_total=(nb + 1) * npad)
    tries, fb, jit = side.host('tries', nb, np.int32), side.host('fb', nb, np.int32), side.host('jit', nb, np.float64)
    side.ok(side.lib.g3_potrf_robust_batched(side.ctx, K.ptr, K.ld, n * K.ld, L.ptr, L.ld, npad * L.ld, nb, n, _code(dt), 20,
                                             _iptr(tries), _iptr(fb), _dptr(jit)), 'g3_potrf_robust_batched')
    return {'L': None}


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('n', [7, 129, 200, 300])
def test_potrf_robust_batched(pairs, n, dt):
    """g3_potrf_robust_batched, batch = 3 (one clean member, one that needs the jitter schedule, one non-finite: fallback):
    the device schedule (n <= 256) and the loop over single calls (300); K unchanged, every slot of L -- NaN on entry -- zero
    outside its n x n lower triangle, and a fourth, canary slot behind the batch untouched"""
    a, h, _ = run_case(pairs, 'default', case_potrf_robust_batched, n, dt)
    npad = _rup(n)
    L = h['L'][:3 * npad].reshape(3, npad, npad)
    outside = ~np.pad(hm.tril_mask(n), (0, npad - n))
    assert np.count_nonzero(L[:, outside]) == 0
    tries, fb = h['host:tries'], h['host:fb']
    assert tries[0] == 0 and tries[1] >= 1 and tries[2] == 20 and list(fb) == [0, 0, 1]
