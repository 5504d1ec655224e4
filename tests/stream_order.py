"""Helpers of tests/test_gpu_stream_order.py: a torch stream kept busy with a marker event behind the work, device operands
that live in torch tensors (so that torch can produce the inputs and consume the outputs on the same stream as the
library), the three passes every scenario makes, and the call sequences with their CPU references.

  busy(stream, ms)     one spin kernel (torch.cuda._sleep) or a row of matmuls that occupies `stream` for at least `ms`,
                       calibrated once per session with HIP events, and an event recorded right behind it.  While the
                       event is incomplete everything enqueued on the stream since is still waiting: what the library
                       launches there -- and on the side stream it forks from there -- has not started.
  Buffers              inputs (a staging tensor with the values, a live tensor the library reads), in/out operands and
                       outputs; poison() fills every live tensor with NaN, produce() copies the inputs into place ON THE
                       STREAM, snapshot() copies every output ON THE STREAM
  run_passes           warm-up (twice; the second is timed: the host enqueue time), reference (a g3_ctx_sync after every
                       call; checked against the CPU reference), asynchronous (busy, produce, the calls, snapshot; compared
                       with the reference pass bit for bit)

The references are NumPy / SciPy in fp64 on the inputs as the device type sees them (fp32: rounded to fp32 first) and the
oracle under oracle/ for the covariance functions; every tolerance is the one tests/test_gpu_kernels.py,
tests/test_gpu_kernel_variants.py, tests/test_gpu_gram.py, tests/test_gpu_fuzz.py or tests/test_gpu_process.py already
uses for that entry point."""
import collections
import ctypes as C
import functools
import math
import time

import numpy as np
import scipy.linalg

BUSY_FLOOR_MS = 50.0      # no scenario runs behind less than this
BUSY_MARGIN = 20.0        # times the host enqueue time of the scenario: host launch time varies several-fold on a shared box
BUSY_CAP_MS = 1000.0      # a scenario that would need more than this in all is a finding, not a reason to wait longer
D = 3
POISON_INT = 0x7fc00000   # what an int32 operand holds before its values are produced (the bits of a float NaN)

Call = collections.namedtuple('Call', 'name fn blocks')      # fn() -> status; blocks: the header says it synchronises


# --------------------------------------------------------------------------------------- a busy stream
_CAL = {}


def _calibration():
    """once per session: how many spin cycles (or matmuls) make a millisecond, measured with HIP events"""
    if _CAL:
        return _CAL
    import torch
    s = torch.cuda.Stream()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record(s)
            fn()
            e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1)
    if hasattr(torch.cuda, '_sleep'):
        cycles, ms = 1000000, 0.0
        timed(lambda: torch.cuda._sleep(cycles))
        for _ in range(6):
            ms = min(timed(lambda: torch.cuda._sleep(cycles)) for _ in range(2))
            if ms >= 2.0:
                break
            cycles *= 8
        if ms >= 2.0:
            _CAL.update(kind='sleep', per_ms=cycles / ms, unit_ms=ms)
    if not _CAL:
        a = torch.randn(4096, 4096, device='cuda')
        out = torch.empty_like(a)
        torch.cuda.synchronize()
        timed(lambda: torch.mm(a, a, out=out))
        ms = min(timed(lambda: torch.mm(a, a, out=out)) for _ in range(3))
        _CAL.update(kind='matmul', a=a, out=out, unit_ms=ms)
    print('stream_order: busy() calibrated on %s, one unit = %.3f ms' % (_CAL['kind'], _CAL['unit_ms']))
    return _CAL


def busy(stream, ms):
    """keep `stream` occupied for at least `ms` milliseconds; returns the marker event recorded right behind that work"""
    import torch
    cal = _calibration()
    ms = 1.1 * float(ms)          # the calibration is a minimum over a few runs: a tenth on top
    with torch.cuda.stream(stream):
        if cal['kind'] == 'sleep':
            torch.cuda._sleep(int(ms * cal['per_ms']))
        else:
            for _ in range(int(math.ceil(ms / cal['unit_ms']))):
                torch.mm(cal['a'], cal['a'], out=cal['out'])
        marker = torch.cuda.Event()
        marker.record(stream)
    return marker


def busy_ms(host_seconds):
    """how long a scenario whose enqueue sequence took `host_seconds` on the host must keep its stream busy"""
    ms = max(BUSY_FLOOR_MS, BUSY_MARGIN * host_seconds * 1e3)
    assert ms <= BUSY_CAP_MS, 'enqueueing took %.1f ms on the host: %.0f ms of busy stream would be needed' % (host_seconds * 1e3, ms)
    return ms


def assert_busy(marker, where):
    """the condition for `this case exercised anything`: the work in front of the marker is still running"""
    if marker.query():
        raise AssertionError('the stream was idle %s: the marker behind the busy work had already completed, '
                             'so the case exercised nothing' % where)


# --------------------------------------------------------------------------------------- operands in torch tensors
def _tdtype(dtype):
    import torch
    return {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32}[np.dtype(dtype)]


class Buffers:
    """The device operands of one call sequence on one context, held in torch tensors and handed to the library through
    Device.wrap.  Everything a method enqueues goes on `stream`, whichever stream that is."""

    def __init__(self, dev, stream):
        self.dev, self.stream = dev, stream
        self.live, self.staging, self.outputs, self.snaps = {}, {}, [], {}

    def _wrap(self, t, dtype):
        rows, cols = t.shape
        return self.dev.wrap(t.data_ptr(), rows, cols, cols, dtype, keep=t)

    def inp(self, name, array, dtype, output=False):
        """an input (output=True: an operand the library overwrites in place, an output as well)"""
        import torch
        array = np.ascontiguousarray(np.atleast_2d(np.asarray(array)).astype(dtype))
        self.staging[name] = torch.from_numpy(array).cuda()
        self.live[name] = torch.empty_like(self.staging[name])
        if output:
            self._output(name)
        return self._wrap(self.live[name], dtype)

    def out(self, name, rows, cols, dtype):
        import torch
        self.live[name] = torch.empty((rows, cols), dtype=_tdtype(dtype), device='cuda')
        self._output(name)
        return self._wrap(self.live[name], dtype)

    def _output(self, name):
        import torch
        self.outputs.append(name)
        self.snaps[name] = torch.empty_like(self.live[name])

    def poison(self):
        import torch
        with torch.cuda.stream(self.stream):
            for t in list(self.live.values()) + list(self.snaps.values()):
                t.fill_(float('nan') if t.is_floating_point() else POISON_INT)

    def produce(self):
        """the real inputs, copied into place device to device on the stream"""
        import torch
        with torch.cuda.stream(self.stream):
            for name, t in self.staging.items():
                self.live[name].copy_(t, non_blocking=True)

    def snapshot(self):
        """a copy of every output, enqueued on the stream behind whatever is queued there now (the last output first)"""
        import torch
        with torch.cuda.stream(self.stream):
            for name in reversed(self.outputs):
                self.snaps[name].copy_(self.live[name], non_blocking=True)

    def read(self, snaps=False):
        """host copies of the outputs (or of their snapshots); the caller has synchronised"""
        src = self.snaps if snaps else self.live
        return {name: src[name].cpu().numpy() for name in self.outputs}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same_bits(got, want, what):
    assert set(got) == set(want), what
    for name in want:
        if not same_bits(got[name], want[name]):
            a, b = np.atleast_1d(got[name]), np.atleast_1d(want[name])
            diff = a.view(np.uint8).reshape(-1) != b.view(np.uint8).reshape(-1)
            at = np.unravel_index(int(np.flatnonzero(diff)[0]) // a.dtype.itemsize, a.shape)
            raise AssertionError('%s: %s differs in %d bytes, first at %s: %r != %r' % (what, name, int(diff.sum()), at, a[at], b[at]))


def run_calls(dev, calls, sync_each=False, marker=None, after_each=False):
    """make the calls in order; after_each: `marker` must still be incomplete when each call without a host out-parameter
    returns -- until a call that synchronises has been made: it drains the stream, marker included"""
    for c in calls:
        rc = c.fn()
        assert rc == 0, '%s returned %d (%s)' % (c.name, rc, (dev.lib.g3_last_error(dev.ctx) or b'').decode())
        if c.blocks:
            marker = None
        if marker is not None and after_each:
            assert_busy(marker, 'when %s returned: an entry point without a host out-parameter blocked' % c.name)
        if sync_each:
            dev.sync()


def run_passes(dev, stream, bufs, calls, host, check, label, after_each=False, snapshot=False):
    """the three passes of a scenario on the adopted `stream`; `host` is the dict the blocking calls put their host
    outputs into.  after_each: the marker must still be incomplete when each asynchronous call returns (scenario 2);
    snapshot: the outputs are copied on the stream right after the last call and the copies compared too.
    Returns (outputs of the reference pass, host outputs of the reference pass)."""
    # warm-up, twice: the first takes the one-time costs (hipRTC, the side-stream probe, scratch growth), the second
    # measures what the enqueue sequence costs the host
    for _ in range(2):
        bufs.poison()
        bufs.produce()
        stream.synchronize()
        t0 = time.perf_counter()
        run_calls(dev, calls)
        enqueue = time.perf_counter() - t0
        dev.sync()
    # reference: a synchronisation after every call
    bufs.poison()
    bufs.produce()
    stream.synchronize()
    host.clear()
    run_calls(dev, calls, sync_each=True)
    stream.synchronize()
    ref, ref_host = bufs.read(), {k: np.array(v, copy=True) for k, v in host.items()}
    check(ref, ref_host)
    # asynchronous: the inputs are produced, and the outputs consumed, on a stream that is busy from start to finish
    bufs.poison()
    stream.synchronize()
    host.clear()
    ms = busy_ms(enqueue)
    marker = busy(stream, ms)
    bufs.produce()
    assert_busy(marker, 'just before the first library call')
    run_calls(dev, calls, marker=marker, after_each=after_each)
    if snapshot:
        bufs.snapshot()
    stream.synchronize()
    print('%s: busy %.1f ms, enqueue %.3f ms' % (label, ms, enqueue * 1e3))
    got = bufs.read()
    assert_same_bits(got, ref, '%s: asynchronous pass vs reference pass' % label)
    assert_same_bits({k: np.asarray(v) for k, v in host.items()}, ref_host, '%s: host outputs' % label)
    if snapshot:
        assert_same_bits(bufs.read(snaps=True), got, '%s: outputs consumed on the stream vs outputs after synchronisation' % label)
    return ref, ref_host


# --------------------------------------------------------------------------------------- seeded problems, computed once
def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def spd(n):
    rng = np.random.default_rng(n)
    B = rng.standard_normal((n, max(8, n // 4)))
    return _frozen(B @ B.T / B.shape[1] + np.eye(n))


@functools.lru_cache(maxsize=None)
def rhs(m, n):
    return _frozen(np.random.default_rng(m + n).standard_normal((m, n)))


@functools.lru_cache(maxsize=None)
def chol_of(n, dtname):
    """(K as the type sees it, scipy's factor of that K in fp64, cond_2 of the factor)"""
    K = spd(n).astype(dtname)
    L = scipy.linalg.cholesky(K.astype(np.float64), lower=True)
    w = np.linalg.eigvalsh(K.astype(np.float64))
    return _frozen(K, L) + (float(np.sqrt(w[-1] / w[0])),)


def code_of(dt):
    from g3py_amd import _lib
    return _lib.dtype_code(dt)


def _f64(dt):
    return np.dtype(dt) == np.float64


def block_inverses(L):
    n = L.shape[0]
    return np.concatenate([np.tril(np.linalg.inv(L[k:k + 128, k:k + 128])) for k in range(0, n, 128)])


# --------------------------------------------------------------------------------------- Gram assembly
RATE = np.array([0.8, 1.0, 1.3])
SE = ('SE', 1.3, RATE, None)
SPEC_TABLE = ('sum', SE, ('NOISE', 0.1))
GRAM_RTOL = {True: (1e-12, 1e-13), False: (3e-4, 3e-5)}       # tests/test_gpu_gram.py: rtol, atol for fp64 / fp32


@functools.lru_cache(maxsize=None)
def points(n, seed):
    return _frozen(np.random.default_rng(seed).uniform(0, 3, (n, D)))


def gram_sequence(dev, bufs, dt, N=300, M=130):
    """g3_gram (square with LOWER | PAD_EYE | SCRUB, and cross), g3_gram_rows and g3_gram_diag at N = 300, d = 3"""
    from oracle import g3_oracle as orc
    from g3py_amd.device import compile_spec
    lib, ctx, code = dev.lib, dev.ctx, code_of(dt)
    prog, cross = compile_spec(SPEC_TABLE, D), compile_spec(SE, D)
    Np, Mp, row0, nrows = 384, 256, 128, 256
    Xh, Xsh = points(N, 1).astype(dt), points(M, 2).astype(dt)
    X, Xs = bufs.inp('X', Xh, dt), bufs.inp('Xs', Xsh, dt)
    Ksq, Kx = bufs.out('Ksq', Np, Np, dt), bufs.out('Kx', Mp, Np, dt)
    Kr, dg = bufs.out('Krows', nrows, row0 + nrows, dt), bufs.out('diag', 1, N, dt)
    calls = [
        Call('g3_gram (square)', lambda: lib.g3_gram(ctx, C.byref(prog), X.ptr, N, X.ld, None, 0, 0, D, code, Ksq.ptr, Ksq.ld,
                                                    Np, Np, 1 | 2 | 4), False),
        Call('g3_gram (cross)', lambda: lib.g3_gram(ctx, C.byref(cross), Xs.ptr, M, Xs.ld, X.ptr, N, X.ld, D, code, Kx.ptr, Kx.ld,
                                                   Mp, Np, 2), False),
        Call('g3_gram_rows', lambda: lib.g3_gram_rows(ctx, C.byref(prog), X.ptr, N, X.ld, D, row0, nrows, code, Kr.ptr, Kr.ld,
                                                     2 | 4), False),
        Call('g3_gram_diag', lambda: lib.g3_gram_diag(ctx, C.byref(prog), X.ptr, N, X.ld, D, code, dg.ptr), False),
    ]
    X64, Xs64 = Xh.astype(np.float64), Xsh.astype(np.float64)
    full = np.eye(Np)
    full[:N, :N] = orc.tt_to_num(orc.kernel_cov(SPEC_TABLE, X64))
    crs = np.zeros((Mp, Np))
    crs[:M, :N] = orc.tt_to_num(orc.kernel_cov(SE, Xs64, X64))
    rtol, atol = GRAM_RTOL[_f64(dt)]

    def check(out, host):
        low = np.tril(np.ones((Np, Np), bool))
        np.testing.assert_allclose(out['Ksq'][low], full[low], rtol=rtol, atol=atol, err_msg='g3_gram, square')
        np.testing.assert_allclose(out['Kx'], crs, rtol=rtol, atol=atol, err_msg='g3_gram, cross')
        np.testing.assert_allclose(out['Krows'], full[row0:row0 + nrows, :row0 + nrows], rtol=rtol, atol=atol, err_msg='g3_gram_rows')
        np.testing.assert_allclose(out['diag'][0], np.diag(full)[:N], rtol=rtol, atol=atol, err_msg='g3_gram_diag')
    return calls, {}, check


# --------------------------------------------------------------------------------------- factor, solve, row sums
def _tri_tol(dt, cond):
    """fp64: the figure of the entry point's own test; fp32: 3e-4 cond(L), what the project accepts for fp32 triangular results
    (tests/test_gpu_kernel_variants.py, tests/test_gpu_kernels.py)"""
    return None if _f64(dt) else 3e-4 * cond


def check_factor(Kin, got, Lr, cond, dt, what):
    n = Lr.shape[0]
    np.testing.assert_array_equal(np.triu(got, 1), np.triu(Kin, 1), err_msg='%s: the strict upper triangle was touched' % what)
    err = np.abs(np.tril(got).astype(np.float64) - Lr).max()
    tol = 1e-12 * n ** 0.5 if _f64(dt) else _tri_tol(dt, cond) * np.abs(Lr).max()
    print('%s: max|L - L_lapack| %.3e (tol %.3e)' % (what, err, tol))
    assert err <= tol, what


def check_solve(Lg, B, got, cond, dt, what):
    ref = scipy.linalg.solve_triangular(Lg, B.astype(np.float64).T, lower=True).T
    err = np.abs(got.astype(np.float64) - ref).max()
    tol = (1e-11 if _f64(dt) else _tri_tol(dt, cond)) * np.abs(ref).max()
    print('%s: max|X - X_ref| %.3e (tol %.3e)' % (what, err, tol))
    assert err <= tol, what


def sweep_sequence(dev, bufs, dt, n, m, first='nowait', tag=''):
    """g3_potrf_nowait (first='potrf': the synchronising g3_potrf) then g3_trsm_rlt (m rows, the factor's block inverses) then
    g3_rows_dot_ss"""
    lib, ctx, code = dev.lib, dev.ctx, code_of(dt)
    Kh, Lr, cond = chol_of(n, np.dtype(dt).name)
    Bh, ah = rhs(m, n).astype(dt), rhs(1, n).astype(dt)
    K, W = bufs.inp(tag + 'K', Kh, dt, output=True), bufs.out(tag + 'invd', n, 128, dt)
    B, a = bufs.inp(tag + 'B', Bh, dt, output=True), bufs.inp(tag + 'a', ah, dt)
    dot, ss = bufs.out(tag + 'dot', 1, m, dt), bufs.out(tag + 'ss', 1, m, dt)
    host = {}
    if first == 'nowait':
        acc = bufs.inp(tag + 'info', np.zeros((1, 1), np.int32), np.int32, output=True)
        factor = Call('g3_potrf_nowait', lambda: lib.g3_potrf_nowait(ctx, K.ptr, n, K.ld, code, W.ptr, acc.ptr), False)
    else:
        def potrf():
            info = C.c_int(-1)
            rc = lib.g3_potrf(ctx, K.ptr, n, K.ld, code, W.ptr, C.byref(info))
            host[tag + 'info'] = info.value
            return rc
        factor = Call('g3_potrf', potrf, True)
    calls = [factor,
             Call('g3_trsm_rlt', lambda: lib.g3_trsm_rlt(ctx, K.ptr, n, K.ld, B.ptr, m, B.ld, code, W.ptr), False),
             Call('g3_rows_dot_ss', lambda: lib.g3_rows_dot_ss(ctx, B.ptr, m, n, B.ld, a.ptr, code, dot.ptr, ss.ptr), False)]

    def check(out, hst):
        what = '%ssweep %s n=%d %s' % (tag, np.dtype(dt).name, n, first)
        info = int(out[tag + 'info'][0, 0]) if first == 'nowait' else int(hst[tag + 'info'])
        assert info == 0, (what, info)
        check_factor(Kh, out[tag + 'K'], Lr, cond, dt, what)
        Lg = np.tril(out[tag + 'K']).astype(np.float64)
        # the block inverses against the inverses of the factor's own diagonal blocks: the bound of g3_trtri_full's test
        Wr = block_inverses(Lg)
        wtol = (5e-13 if _f64(dt) else 3e-4) * cond * np.abs(Wr).max()
        assert np.abs(out[tag + 'invd'].astype(np.float64) - Wr).max() <= wtol, what
        check_solve(Lg, Bh, out[tag + 'B'], cond, dt, what)
        # the row sums of the solved rows as they are on the device: n 2^-52 sum|terms| plus one rounding of the stored result
        # (tests/test_gpu_memory_contracts.py::test_rows_dot_ss_against_fsum)
        Xg, a64 = out[tag + 'B'].astype(np.float64), ah.astype(np.float64)[0]
        store = 2.0 ** -53 if _f64(dt) else 2.0 ** -24
        for name, terms in ((tag + 'dot', Xg * a64), (tag + 'ss', Xg * Xg)):
            want = np.array([math.fsum(t) for t in terms])
            bound = n * 2.0 ** -52 * np.abs(terms).sum(1) + store * np.abs(want)
            assert (np.abs(out[name][0].astype(np.float64) - want) <= bound).all(), (what, name)
    return calls, host, check


def potri_sequence(dev, bufs, dt, n, tag=''):
    """g3_potri on a given factor, the block inverses computed into the context's own buffer"""
    lib, ctx, code = dev.lib, dev.ctx, code_of(dt)
    Lh = np.tril(chol_of(n, 'float64')[1]).astype(dt)
    L = bufs.inp(tag + 'L', Lh, dt)
    Y, Ki = bufs.out(tag + 'Y', n, n, dt), bufs.out(tag + 'Kinv', n, n, dt)
    calls = [Call('g3_potri', lambda: lib.g3_potri(ctx, L.ptr, n, L.ld, None, code, Y.ptr, Y.ld, Ki.ptr, Ki.ld), False)]
    L64 = Lh.astype(np.float64)
    Linv = np.linalg.inv(L64)
    Kinv = Linv.T @ Linv

    def check(out, host):
        tol = 1e-10 if _f64(dt) else 2e-4                 # tests/test_gpu_kernels.py::test_potri_matches_lapack
        assert np.abs(out[tag + 'Y'] - Linv.T).max() < tol * np.abs(Linv).max(), 'g3_potri: Y'
        assert np.abs(np.tril(out[tag + 'Kinv']) - np.tril(Kinv)).max() < tol * np.abs(Kinv).max(), 'g3_potri: K^-1'
    return calls, {}, check


def trsm_sequence(dev, bufs, dt, n, m):
    """g3_trsm_rlt alone, the block inverses computed from L into the context's own buffer"""
    lib, ctx, code = dev.lib, dev.ctx, code_of(dt)
    _, Lr, cond = chol_of(n, np.dtype(dt).name)
    Lh, Bh = Lr.astype(dt), rhs(m, n).astype(dt)
    L, B = bufs.inp('L', Lh, dt), bufs.inp('B', Bh, dt, output=True)
    calls = [Call('g3_trsm_rlt', lambda: lib.g3_trsm_rlt(ctx, L.ptr, n, L.ld, B.ptr, m, B.ld, code, None), False)]

    def check(out, host):
        check_solve(Lh.astype(np.float64), Bh, out['B'], cond, dt, 'trsm %s n=%d m=%d' % (np.dtype(dt).name, n, m))
    return calls, {}, check


def trtri_sequence(dev, bufs, dt, n, m):
    """g3_trtri_full then g3_trsm_full on a given factor and its block inverses"""
    lib, ctx, code = dev.lib, dev.ctx, code_of(dt)
    _, Lr, cond = chol_of(n, np.dtype(dt).name)
    Lh, Bh = Lr.astype(dt), rhs(m, n).astype(dt)
    L64 = Lh.astype(np.float64)
    L, W, B = bufs.inp('L', Lh, dt), bufs.inp('invd', block_inverses(L64), dt), bufs.inp('B', Bh, dt)
    V, Vt, U, X = bufs.out('V', n, n, dt), bufs.out('Vt', n, n, dt), bufs.out('U', n, n, dt), bufs.out('X', m, n, dt)
    calls = [Call('g3_trtri_full', lambda: lib.g3_trtri_full(ctx, L.ptr, n, W.ptr, V.ptr, Vt.ptr, U.ptr, code), False),
             Call('g3_trsm_full', lambda: lib.g3_trsm_full(ctx, V.ptr, n, n, B.ptr, m, n, X.ptr, n, code), False)]
    ref = np.linalg.inv(L64)
    want = scipy.linalg.solve_triangular(L64, Bh.astype(np.float64).T, lower=True).T
    blocks = (np.arange(n) // 128)[:, None] >= (np.arange(n) // 128)[None, :]      # V's lower block triangle is what is written

    def check(out, host):
        tol = (5e-13 if _f64(dt) else 3e-4) * cond        # tests/test_gpu_kernels.py: the full inverse and the one-product solve
        assert np.abs(out['V'].astype(np.float64) - ref)[blocks].max() <= tol * np.abs(ref).max(), 'g3_trtri_full'
        assert np.abs(out['X'].astype(np.float64) - want).max() <= tol * np.abs(want).max(), 'g3_trsm_full'
    return calls, {}, check


# --------------------------------------------------------------------------------------- the fused entries
SPEC_F = ('SE', 1.3, np.array([0.8, 1.0, 1.2]), None)
NOISE = 0.1


@functools.lru_cache(maxsize=None)
def _gp_problem(N, M, dtname):
    from oracle import g3_oracle as orc
    rng = np.random.default_rng(N + M)
    X = rng.uniform(0, N ** (1.0 / D), (N, D)).astype(dtname)
    Xs = rng.uniform(0, N ** (1.0 / D), (M, D)).astype(dtname)
    y = (np.sin(X.sum(1)) + 0.1 * rng.standard_normal(N)).astype(dtname)
    X64, Xs64, y64 = X.astype(np.float64), Xs.astype(np.float64), y.astype(np.float64)
    spec_n = orc.with_noise(SPEC_F, NOISE)
    K, grads = orc.kernel_cov_grads(spec_n, X64)
    L = scipy.linalg.cholesky(orc.tt_to_num(K), lower=True)
    a = scipy.linalg.solve_triangular(L, y64, lower=True)
    V = scipy.linalg.solve_triangular(L, orc.tt_to_num(orc.kernel_cov(SPEC_F, Xs64, X64)).T, lower=True)
    Kinv = np.linalg.inv(K)
    alpha = Kinv @ y64
    G = np.outer(alpha, alpha) - Kinv
    slots = [(leaf, pname, k, 0.5 * np.sum(G * dK), 0.5 * np.sum(np.abs(G * dK)) + 1e-30) for leaf, pname, k, dK in grads]
    ref = dict(logdet=float(np.log(np.diag(L)).sum()), quad=float(a.dot(a)), a=a, mu=V.T.dot(a), ss=(V ** 2).sum(0), alpha=alpha)
    return _frozen(X, Xs, y) + (ref, slots)


def fused_sequence(dev, bufs, dt, N=641, M=130):
    """g3_gp_factor_predict then g3_gp_dlogp: both synchronise before they return, but their first launch on either stream
    still has to wait for what is queued on the adopted stream"""
    from oracle import g3_oracle as orc
    from g3py_amd import _lib
    from g3py_amd.device import compile_spec
    lib, ctx, code = dev.lib, dev.ctx, code_of(dt)
    Xh, Xsh, yh, ref, slots_ref = _gp_problem(N, M, np.dtype(dt).name)
    prog, cross = compile_spec(orc.with_noise(SPEC_F, NOISE), D), compile_spec(SPEC_F, D)
    gmap = dev.grad_layout(prog)
    Np, Mp = _lib.roundup(N), _lib.roundup(M, 128)
    X, Xs, y = bufs.inp('X', Xh, dt), bufs.inp('Xs', Xsh, dt), bufs.inp('delta', yh, dt)
    K, W, a = bufs.out('K', Np + _lib.G3_RHS_PAD + Mp, Np, dt), bufs.out('invd', Np, 128, dt), bufs.out('a', 1, Np, dt)
    mu, ss = bufs.out('mu', 1, Mp, dt), bufs.out('ss', 1, Mp, dt)
    Y, Ki, al = bufs.out('Y', Np, Np, dt), bufs.out('Kinv', Np, Np, dt), bufs.out('alpha', 1, Np, dt)
    host = {}

    def factor_predict():
        out = (C.c_double * 6)()
        rc = lib.g3_gp_factor_predict(ctx, C.byref(prog), C.byref(cross), X.ptr, N, X.ld, D, y.ptr, Xs.ptr, M, Xs.ld, code,
                                      K.ptr, K.ld, W.ptr, a.ptr, mu.ptr, ss.ptr, out)
        host['stats'] = np.array(out[:])
        return rc

    def dlogp():
        out = (C.c_double * max(gmap.nslots, 1))()
        rc = lib.g3_gp_dlogp(ctx, C.byref(prog), C.byref(gmap), X.ptr, N, X.ld, D, K.ptr, K.ld, W.ptr, a.ptr, code, Y.ptr, Y.ld,
                             Ki.ptr, Ki.ld, al.ptr, out)
        host['slots'] = np.array(out[:gmap.nslots])
        return rc
    calls = [Call('g3_gp_factor_predict', factor_predict, True), Call('g3_gp_dlogp', dlogp, True)]

    def check(out, hst):
        st = hst['stats']
        assert st[2] == 0 and st[3] == 0 and st[4] == 0 and st[5] == 0, st         # nothing non-finite, no retry, no failed pivot
        f64 = _f64(dt)
        # fp64: tests/test_gpu_kernel_variants.py::test_tall_sweep_under_each_variant (scalars 1e-9, vectors 1e-8) and
        # tests/test_gpu_fuzz.py (alpha 1e-7 / 1e-8 max, sums 1e-8 of their scale); fp32: tests/test_gpu_process.py (logdet
        # 2e-4, quad 2e-3, a 2e-3 max|a|, posterior 2e-3) and tests/test_gpu_gram.py (sums 2e-4 of their scale)
        for key, got, rel in (('logdet', st[0], 1e-9 if f64 else 2e-4), ('quad', st[1], 1e-9 if f64 else 2e-3)):
            print('fused %s %s: %.12g (reference %.12g)' % (np.dtype(dt).name, key, got, ref[key]))
            assert abs(got - ref[key]) <= rel * max(1.0, abs(ref[key])), key
        vec = dict(rtol=1e-8, atol=1e-8) if f64 else dict(rtol=2e-3, atol=2e-3)
        np.testing.assert_allclose(out['a'][0, :N], ref['a'], err_msg='a', **(vec if f64 else dict(rtol=0, atol=2e-3 * np.abs(ref['a']).max())))
        np.testing.assert_allclose(out['mu'][0, :M], ref['mu'], err_msg='mu', **vec)
        np.testing.assert_allclose(out['ss'][0, :M], ref['ss'], err_msg='ss', **vec)
        amax = np.abs(ref['alpha']).max()
        np.testing.assert_allclose(out['alpha'][0, :N], ref['alpha'], err_msg='alpha',
                                   **(dict(rtol=1e-7, atol=1e-8 * amax) if f64 else dict(rtol=0, atol=2e-3 * amax)))
        for leaf, pname, k, want, scale in slots_ref:
            got = hst['slots'][getattr(gmap, pname)[leaf] + (0 if k is None else k)]
            assert abs(got - want) < (1e-8 if f64 else 2e-4) * scale, (leaf, pname, k, got, want)
    return calls, host, check


# --------------------------------------------------------------------------------------- the launch log
def bulk_launches(log):
    return [l for l in log if l.bulk == 1]
