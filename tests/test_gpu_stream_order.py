"""The stream-order and asynchrony contract of the C ABI (include/g3hip.h, "Conventions"):

    Work is enqueued on the context's HIP stream (g3_ctx_set_stream adopts a caller stream such as torch's current
    stream).  Functions with host out-parameters synchronise the stream before returning; functions with only device
    outputs are asynchronous.

Every other GPU test uploads with a synchronising copy, makes one call on the context's own stream and downloads with a
synchronising copy: the stream is idle when a call starts and drained before anyone looks.  Here the context works on an
adopted torch stream that is BUSY (stream_order.busy) while the calls are enqueued: torch produces the inputs on that stream
in front of the calls and consumes the outputs behind them, contexts are reused from call to call without a drain, the
kernel-program ring wraps onto launches that have not run, and the stream changes under a live context.  What keeps all of
that correct is host-side bookkeeping -- the opening fork and the closing join of the two-stream sweeps (g3_sweep_scope), the
pivot flag's info_clean / info_sync / info_stream, the ring's events, the per-stream placement of the side stream -- and a
missing fence gives wrong numbers only when the stream is not idle.

Every scenario (stream_order.run_passes) makes a warm-up pass (one-time costs, and the host enqueue time), a reference pass
with a g3_ctx_sync after every call, checked against a CPU reference at the tolerances the suite already uses for the entry
point, and the asynchronous pass, whose outputs must equal the reference pass BIT FOR BIT (the library has no floating-point
atomics and fixed summation orders; no entry point exercised here turned out not to be reproducible from run to run).  The
stream is kept busy for 20 times the measured enqueue time, 50 ms at least; each test prints both.  A scenario whose marker
event has completed at the point it names fails: no test passes on an idle stream.

A `two-stream` case proves with the `bulk` column of the launch log (G3_GEMM_LOG) that launches went to the side stream.
g3_potrf_nowait stays on ONE stream up to n = 2048 whatever G3_NB says (it is the diagonal-block factorisation of the
multi-GPU sweep), so its n = 640 cases are one-stream cases, asserted as such; the two-stream sweep behind the same entry
point is reached at n = 2176, and at n = 640 through g3_potrf: both are run as well."""
import ctypes as C
import os
import re
import time

import numpy as np
import pytest
import scipy.linalg

import stream_order as so
from stream_order import Call
from test_gpu_kernel_variants import variant_context

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (sequence builder, knobs of the context, whether launches must show on the bulk stream, dtypes)
SEQUENCES = {
    'gram300': (lambda dev, b, dt: so.gram_sequence(dev, b, dt), {}, False, (F64, F32)),
    'nowait640_sb1': (lambda dev, b, dt: so.sweep_sequence(dev, b, dt, 640, 128), {'G3_NB': 128, 'G3_SB': 1}, False, (F64, F32)),
    'nowait640_sb2': (lambda dev, b, dt: so.sweep_sequence(dev, b, dt, 640, 128), {'G3_NB': 128, 'G3_SB': 2}, False, (F64, F32)),
    'potrf640_sb1': (lambda dev, b, dt: so.sweep_sequence(dev, b, dt, 640, 128, 'potrf'), {'G3_NB': 128, 'G3_SB': 1}, True, (F64, F32)),
    'potrf640_sb2': (lambda dev, b, dt: so.sweep_sequence(dev, b, dt, 640, 128, 'potrf'), {'G3_NB': 128, 'G3_SB': 2}, True, (F64, F32)),
    'nowait2176_sb1': (lambda dev, b, dt: so.sweep_sequence(dev, b, dt, 2176, 128), {'G3_NB': 128, 'G3_SB': 1}, True, (F64, F32)),
    'nowait2176_sb2': (lambda dev, b, dt: so.sweep_sequence(dev, b, dt, 2176, 128), {'G3_NB': 128, 'G3_SB': 2}, True, (F64, F32)),
    'potri768': (lambda dev, b, dt: so.potri_sequence(dev, b, dt, 768), {}, True, (F64, F32)),
    'trsm4096': (lambda dev, b, dt: so.trsm_sequence(dev, b, dt, 4096, 128), {}, True, (F64,)),
    'trtri256': (lambda dev, b, dt: so.trtri_sequence(dev, b, dt, 256, 64), {}, False, (F64, F32)),
    'fused641': (lambda dev, b, dt: so.fused_sequence(dev, b, dt, 641, 130), {'G3_NB': 128}, True, (F64, F32)),
}
CASES = [pytest.param(name, dt, id='%s-%s' % (name, np.dtype(dt).name)) for name, v in SEQUENCES.items() for dt in v[3]]


def _adopt(run, stream):
    run.dev.set_stream(stream.cuda_stream)


def _scenario(monkeypatch, tmp_path, name, dt, what, **mode):
    import torch
    build, knobs, two_stream, _ = SEQUENCES[name]
    with variant_context(monkeypatch, tmp_path, **knobs) as run:
        s = torch.cuda.Stream()
        _adopt(run, s)
        bufs = so.Buffers(run.dev, s)
        calls, host, check = build(run.dev, bufs, dt)
        torch.cuda.synchronize()
        so.run_passes(run.dev, s, bufs, calls, host, check, '%s %s-%s' % (what, name, np.dtype(dt).name), **mode)
        run.dev.set_stream(None)          # the context lets go of the torch stream before either is destroyed
    bulk = so.bulk_launches(run.log)
    if two_stream:
        assert bulk, 'no launch on the bulk stream: the case did not reach the two-stream sweep\n%r' % (run.log,)
    else:
        assert not bulk, run.log


# ------------------------------------------------------------------ 1. inputs produced earlier on the adopted stream
@pytest.mark.parametrize('name,dt', CASES)
def test_inputs_produced_earlier_on_the_adopted_stream(monkeypatch, tmp_path, name, dt):
    """Every device input and output starts as NaN; on the adopted stream, with no synchronisation in between: busy work, a
    torch device-to-device copy of the real inputs into place, the library calls.  The marker behind the busy work must be
    incomplete just before the first call, so every launch of the sequence -- the first one on the side stream included --
    was enqueued while its inputs did not exist yet.  The synchronising entries (g3_potrf, g3_gp_factor_predict, g3_gp_dlogp)
    block at their end, but their first launch on either stream still has to wait for the copy."""
    _scenario(monkeypatch, tmp_path, name, dt, 'inputs-earlier')


# ------------------------------------------------------------------ 2. outputs consumed later on the adopted stream
@pytest.mark.parametrize('name,dt', CASES)
def test_outputs_consumed_later_on_the_adopted_stream(monkeypatch, tmp_path, name, dt):
    """The same sequences; right after the last call returns torch copies every output on the adopted stream, and only then
    is the stream synchronised: the copies must equal the outputs as they are after the synchronisation, and the reference
    pass -- the closing join() of each sweep.  After every call without a host out-parameter the marker must still be
    incomplete: the call returned while nothing it enqueued could have started."""
    _scenario(monkeypatch, tmp_path, name, dt, 'outputs-later', after_each=True, snapshot=True)


# ---- the entry points of include/g3hip.h, by what the header promises about them ------------------------------------
# asynchronous: a context, device outputs only, no host out-parameter
ASYNC_ENTRIES = ['g3_memcpy_d2d', 'g3_memset', 'g3_copy2d', 'g3_gram', 'g3_gram_diag', 'g3_gram_rows', 'g3_cov_lift', 'g3_scrub',
                 'g3_gemm_nt', 'g3_gemm_nt_stair', 'g3_potrf_nowait', 'g3_trsm_rlt', 'g3_trtri_full', 'g3_trsm_full', 'g3_diag_add',
                 'g3_rows_dot_ss', 'g3_gp_cross', 'g3_potri', 'g3_gp_loo', 'g3_gp_loo_batched', 'g3_gp_cross_dx', 'g3_gram_diag_dx',
                 'g3_potrf_vjp']
# no host out-parameter and still synchronising: the header says so at each of them
BLOCKING_ENTRIES = {
    'g3_ctx_set_stream': 'drains the stream the context leaves',
    'g3_ctx_sync': 'its purpose',
    'g3_ctx_destroy': 'drains the stream before the context goes',
    'g3_free': 'the buffer may be in use by queued work',
    'g3_memcpy_h2d': 'the host buffer is borrowed for the call only',
    'g3_prof_reset': 'the event records are reused',
    'g3_gp_cross_batched': 'the host programs are borrowed for the call only',
    'g3_gp_cross_batched_fields': 'the host template and fields are borrowed for the call only',
}
# a host out-parameter: synchronise before returning
HOST_OUT_ENTRIES = ['g3_memcpy_d2h', 'g3_potrf', 'g3_potrf_robust', 'g3_potrf_robust_batched', 'g3_logp_terms', 'g3_diag_stats',
                    'g3_gp_factor', 'g3_gp_factor_predict', 'g3_gp_factor_batched', 'g3_gp_factor_batched_fields', 'g3_gram_grad',
                    'g3_gram_grad_rows', 'g3_gp_dlogp', 'g3_gp_dlogp_batched', 'g3_gp_dlogp_batched_fields', 'g3_gp_cv', 'g3_gram_vjp',
                    'g3_gp_dloo', 'g3_gp_dloo_batched_fields', 'g3_gp_draws_batched', 'g3_gp_draws_batched_fields', 'g3_gp_sample',
                    'g3_prof_collect']
# nothing is enqueued: creation, allocation, host-side queries and checks
NO_STREAM_WORK = ['g3_ctx_create', 'g3_last_error', 'g3_version', 'g3_malloc', 'g3_gram_path_stats', 'g3_grad_path_stats',
                  'g3_gram_jit_check', 'g3_grad_jit_check', 'g3_grad_layout', 'g3_prof_enable']


def test_every_entry_point_of_the_header_is_classified():
    """the table above against include/g3hip.h: a new entry point has to say which of the header's two sentences it is under
    (the g3_dist_* driver owns its streams and communicators and is outside this contract)"""
    text = open(os.path.join(ROOT, 'include', 'g3hip.h')).read()
    names = set(re.findall(r'^(?:int|const char\*)\s+(g3_\w+)\(', text, re.M))
    assert len(names) > 60
    table = ASYNC_ENTRIES + list(BLOCKING_ENTRIES) + HOST_OUT_ENTRIES + NO_STREAM_WORK
    assert len(table) == len(set(table))
    assert {n for n in names if not n.startswith('g3_dist_')} == set(table)


class Bench:
    """one small Gaussian process (N = 200, M = 100, d = 3, fp64) factored on an adopted torch stream, its consumers' buffers,
    and one valid call of every asynchronous entry point on them"""

    def __init__(self, run):
        import torch
        from oracle import g3_oracle as orc
        from g3py_amd import _lib
        from g3py_amd.device import compile_spec
        self.dev = dev = run.dev
        self.stream = s = torch.cuda.Stream()
        _adopt(run, s)
        lib, ctx, code = dev.lib, dev.ctx, so.code_of(F64)
        N, M, d = 200, 100, so.D
        Np, Mp = 256, 128
        rng = np.random.default_rng(200)
        self.keep = keep = []

        def T(a, dtype=F64):
            t = torch.from_numpy(np.ascontiguousarray(np.atleast_2d(np.asarray(a)).astype(dtype))).cuda()
            keep.append(t)
            return t

        def E(rows, cols, dtype=torch.float64):
            t = torch.zeros((rows, cols), dtype=dtype, device='cuda')
            keep.append(t)
            return t
        P = lambda t: t.data_ptr()
        prog, cross = compile_spec(orc.with_noise(so.SE, 0.1), d), compile_spec(so.SE, d)
        X, Xs = T(rng.uniform(0, 3, (N, d))), T(rng.uniform(0, 3, (M, d)))
        delta = T(np.sin(np.arange(N) / 7.0))
        K, W, a = E(Np + 128, Np), E(Np, 128), E(1, Np)
        V, mu, ss = E(Mp, Np), E(1, Mp), E(1, Mp)
        Y, alpha, kdiag = E(Np, Np), E(1, Np), E(1, Np)
        alpha2, kdiag2 = E(1, Np), E(1, Np)
        Wd, dmu, dss, dk = E(Mp, Np), E(M, d), E(M, d), E(M, d)
        S0, S1, S2 = T(rng.standard_normal((256, 256))), E(256, 256), E(256, 256)
        spd0, spd1, W2, acc = T(so.spd(256)), E(256, 256), E(256, 128), E(1, 1, torch.int32)
        L256 = T(so.chol_of(256, 'float64')[1])
        W256 = T(so.block_inverses(so.chol_of(256, 'float64')[1]))
        B0, B1 = T(so.rhs(128, 256)), E(128, 256)
        Vf, Vt, U, Xo = E(256, 256), E(256, 256), E(256, 256), E(64, 256)
        dot, rss, dg = E(1, 128), E(1, 128), E(1, Np)
        Y2, Ki = E(256, 256), E(256, 256)
        Lbar, Kbar = T(rng.standard_normal((N, N))), E(N, N)
        Ast, Bst, Cst = T(rng.standard_normal((256, 128))), T(rng.standard_normal((256, 128))), E(256, 256)
        seg_rows, seg_cols = (C.c_int64 * 2)(128, 128), (C.c_int64 * 2)(128, 256)
        torch.cuda.synchronize()
        # the factor and what its consumers need, synchronised
        out = (C.c_double * 6)()
        assert lib.g3_gp_factor(ctx, C.byref(prog), P(X), N, d, d, P(delta), code, P(K), Np, P(W), P(a), out) == 0 and out[5] == 0
        dev.sync()
        kstride = (Np + 128) * Np

        def on_stream(fn):
            def prep():
                with torch.cuda.stream(s):
                    fn()
            return prep
        self.prep = {'g3_potrf_nowait': on_stream(lambda: (spd1.copy_(spd0), acc.zero_())), 'g3_trsm_rlt': on_stream(lambda: B1.copy_(B0)),
                     'g3_cov_lift': on_stream(lambda: S1.copy_(S0)), 'g3_scrub': on_stream(lambda: S1.copy_(S0)),
                     'g3_diag_add': on_stream(lambda: S1.copy_(S0))}
        self.calls = {
            'g3_memcpy_d2d': lambda: lib.g3_memcpy_d2d(ctx, P(S1), P(S0), 256 * 256 * 8),
            'g3_memset': lambda: lib.g3_memset(ctx, P(S2), 0, 256 * 256 * 8),
            'g3_copy2d': lambda: lib.g3_copy2d(ctx, P(S2), 256, P(S0), 256, 200, 130, code),
            'g3_gram': lambda: lib.g3_gram(ctx, C.byref(prog), P(X), N, d, None, 0, 0, d, code, P(S2), 256, Np, Np, 1 | 2 | 4),
            'g3_gram_diag': lambda: lib.g3_gram_diag(ctx, C.byref(prog), P(X), N, d, d, code, P(dg)),
            'g3_gram_rows': lambda: lib.g3_gram_rows(ctx, C.byref(prog), P(X), N, d, d, 128, 128, code, P(S2), 256, 2 | 4),
            'g3_cov_lift': lambda: lib.g3_cov_lift(ctx, P(S1), 256, 256, code),
            'g3_scrub': lambda: lib.g3_scrub(ctx, P(S1), 256, 256, 256, code),
            'g3_gemm_nt': lambda: lib.g3_gemm_nt(ctx, P(S2), 256, P(S0), 256, P(S0), 256, 128, 128, 64, -0.5, 0.0, code, 0),
            'g3_gemm_nt_stair': lambda: lib.g3_gemm_nt_stair(ctx, P(Cst), 256, P(Ast), 128, P(Bst), 128, 128, seg_rows, seg_cols, 2, 1.0,
                                                             0.0, code, 0, None, 0, None),
            'g3_potrf_nowait': lambda: lib.g3_potrf_nowait(ctx, P(spd1), 256, 256, code, P(W2), P(acc)),
            'g3_trsm_rlt': lambda: lib.g3_trsm_rlt(ctx, P(L256), 256, 256, P(B1), 128, 256, code, P(W256)),
            'g3_trtri_full': lambda: lib.g3_trtri_full(ctx, P(L256), 256, P(W256), P(Vf), P(Vt), P(U), code),
            'g3_trsm_full': lambda: lib.g3_trsm_full(ctx, P(Vf), 256, 256, P(B0), 64, 256, P(Xo), 256, code),
            'g3_diag_add': lambda: lib.g3_diag_add(ctx, P(S1), 256, 256, code, 0.5),
            'g3_rows_dot_ss': lambda: lib.g3_rows_dot_ss(ctx, P(B0), 128, 256, 256, P(a), code, P(dot), P(rss)),
            'g3_gp_cross': lambda: lib.g3_gp_cross(ctx, C.byref(cross), P(Xs), M, d, P(X), N, d, d, P(K), Np, P(W), P(a), code, P(V), Np,
                                                   P(mu), P(ss)),
            'g3_potri': lambda: lib.g3_potri(ctx, P(L256), 256, 256, P(W256), code, P(Y2), 256, P(Ki), 256),
            'g3_gp_loo': lambda: lib.g3_gp_loo(ctx, P(K), N, Np, P(W), P(a), code, P(Y), Np, P(alpha), P(kdiag)),
            'g3_gp_loo_batched': lambda: lib.g3_gp_loo_batched(ctx, 1, P(K), N, Np, kstride, P(W), P(a), code, None, P(alpha2), P(kdiag2)),
            'g3_gp_cross_dx': lambda: lib.g3_gp_cross_dx(ctx, C.byref(cross), P(Xs), M, d, P(X), N, d, d, code, P(alpha), P(V), Np, P(Y),
                                                         Np, P(Wd), Np, P(dmu), P(dss), d),
            'g3_gram_diag_dx': lambda: lib.g3_gram_diag_dx(ctx, C.byref(prog), P(Xs), M, d, d, code, P(dk), d),
            'g3_potrf_vjp': lambda: lib.g3_potrf_vjp(ctx, P(K), Np, P(Lbar), N, N, code, P(Kbar), N),
        }
        # the consumers read what these leave: g3_gp_cross_dx needs V (g3_gp_cross), Y and alpha (g3_gp_loo), g3_trsm_full needs V
        for name in ('g3_gp_cross', 'g3_gp_loo', 'g3_trtri_full'):
            assert self.calls[name]() == 0, name
        dev.sync()


@pytest.fixture(scope='module')
def bench(tmp_path_factory):
    mp = pytest.MonkeyPatch()
    try:
        with variant_context(mp, tmp_path_factory.mktemp('asynchrony')) as run:
            b = Bench(run)
            yield b
            run.dev.set_stream(None)
    finally:
        mp.undo()


def test_the_bench_covers_the_table(bench):
    assert sorted(bench.calls) == sorted(ASYNC_ENTRIES)


@pytest.mark.parametrize('name', ASYNC_ENTRIES)
def test_entry_points_without_a_host_out_parameter_return_at_once(bench, name):
    """after a warm-up call (first-use costs: hipRTC, workspace growth) the entry point is called behind busy work on the
    adopted stream: the marker must still be incomplete when the call returns.  What the calls compute is checked by the
    scenarios above and by the other GPU tests; here only that they do not wait"""
    dev, s = bench.dev, bench.stream
    call, prep = bench.calls[name], bench.prep.get(name, lambda: None)
    for _ in range(2):
        prep()
        s.synchronize()
        t0 = time.perf_counter()
        rc = call()
        enqueue = time.perf_counter() - t0
        assert rc == 0, (name, rc, dev.lib.g3_last_error(dev.ctx))
        s.synchronize()
    prep()
    s.synchronize()
    ms = so.busy_ms(enqueue)
    marker = so.busy(s, ms)
    so.assert_busy(marker, 'just before %s' % name)
    rc = call()
    done = marker.query()
    s.synchronize()
    print('asynchrony %s: busy %.1f ms, enqueue %.3f ms' % (name, ms, enqueue * 1e3))
    assert rc == 0, (name, rc, dev.lib.g3_last_error(dev.ctx))
    assert not done, '%s has no host out-parameter and returned only after the stream had drained' % name


def test_entry_points_that_say_they_block_drain_the_stream(bench):
    """g3_ctx_sync, g3_memcpy_h2d, g3_free, g3_prof_reset and g3_ctx_set_stream behind busy work: when each returns, the marker
    on the stream the context worked on has completed (for g3_ctx_set_stream: the stream it leaves)"""
    import torch
    dev, s = bench.dev, bench.stream
    lib, ctx = dev.lib, dev.ctx
    host = np.arange(16.0)
    buf = dev.alloc(1, 16, F64)
    spare = dev.alloc(1, 16, F64)
    other = torch.cuda.Stream()
    for name, fn in (('g3_ctx_sync', lambda: lib.g3_ctx_sync(ctx)),
                     ('g3_memcpy_h2d', lambda: lib.g3_memcpy_h2d(ctx, buf.ptr, host.ctypes.data, host.nbytes)),
                     ('g3_free', lambda: lib.g3_free(ctx, spare.ptr)),
                     ('g3_prof_reset', lambda: lib.g3_prof_reset(ctx)),
                     ('g3_ctx_set_stream', lambda: lib.g3_ctx_set_stream(ctx, other.cuda_stream))):
        marker = so.busy(s, so.BUSY_FLOOR_MS)
        so.assert_busy(marker, 'just before %s' % name)
        assert fn() == 0, name
        assert marker.query(), '%s returned while the stream was still busy' % name
        print('blocking %s: busy %.1f ms' % (name, so.BUSY_FLOOR_MS))
    spare.ptr = 0
    np.testing.assert_array_equal(dev.download(buf)[0], host)
    dev.set_stream(s.cuda_stream)


# ------------------------------------------------------------------ 3. back-to-back calls that share the context's scratch
def _scratch_sequence(dev, bufs, dt, n, m, tag):
    """g3_potrf_nowait (its own block inverses), g3_potri on the factor (event pool of the context), g3_trsm_rlt with the block
    inverses computed into the context's own buffer; every operand of the problem is its own"""
    lib, ctx, code = dev.lib, dev.ctx, so.code_of(dt)
    Kh, Lr, cond = so.chol_of(n, np.dtype(dt).name)
    Bh = so.rhs(m, n).astype(dt)
    K, W = bufs.inp(tag + 'K', Kh, dt, output=True), bufs.out(tag + 'invd', n, 128, dt)
    acc = bufs.inp(tag + 'info', np.zeros((1, 1), np.int32), np.int32, output=True)
    Y, Ki = bufs.out(tag + 'Y', n, n, dt), bufs.out(tag + 'Kinv', n, n, dt)
    B = bufs.inp(tag + 'B', Bh, dt, output=True)
    calls = [Call('g3_potrf_nowait', lambda: lib.g3_potrf_nowait(ctx, K.ptr, n, K.ld, code, W.ptr, acc.ptr), False),
             Call('g3_potri', lambda: lib.g3_potri(ctx, K.ptr, n, K.ld, W.ptr, code, Y.ptr, Y.ld, Ki.ptr, Ki.ld), False),
             Call('g3_trsm_rlt', lambda: lib.g3_trsm_rlt(ctx, K.ptr, n, K.ld, B.ptr, m, B.ld, code, None), False)]

    def check(out):
        what = 'scratch %s%s n=%d' % (tag, np.dtype(dt).name, n)
        assert int(out[tag + 'info'][0, 0]) == 0, what
        so.check_factor(Kh, out[tag + 'K'], Lr, cond, dt, what)
        Lg = np.tril(out[tag + 'K']).astype(np.float64)
        Linv = np.linalg.inv(Lg)
        tol = 1e-10 if dt == F64 else 2e-4              # tests/test_gpu_kernels.py::test_potri_matches_lapack
        assert np.abs(out[tag + 'Y'] - Linv.T).max() < tol * np.abs(Linv).max(), what
        assert np.abs(np.tril(out[tag + 'Kinv']) - np.tril(Linv.T @ Linv)).max() < tol * np.abs(Linv.T @ Linv).max(), what
        so.check_solve(Lg, Bh, out[tag + 'B'], cond, dt, what)
    return calls, check


def _untagged(out, tag):
    return {k[len(tag):]: v for k, v in out.items() if k.startswith(tag)}


@pytest.mark.parametrize('dt', [F64, F32], ids=['float64', 'float32'])
def test_back_to_back_problems_share_the_scratch_of_one_context(monkeypatch, tmp_path, dt):
    """One context, one busy stretch, no synchronisation: the potrf / potri / trsm sequence on problem A (n = 384), on problem B
    (n = 768: the event pool of the sweeps is destroyed and regrown while A's sweep is still queued, and the context's block
    inverses are reallocated, which is the one place the library waits), then on A again with outputs of its own, where the
    smaller problem reuses the events and the block-inverse buffer with nothing drained.  Each of the three results must equal,
    bit for bit, the run of that problem alone -- synchronised after every call, on another context -- and that run is
    checked against LAPACK.  (The context's `work` buffer is not used by these three entry points at sizes that are
    multiples of 128.)  The marker must be incomplete before the first call, after A's last call and after B's g3_potri."""
    import torch
    m = 128
    alone = {}
    with variant_context(monkeypatch, tmp_path) as ref:
        s = torch.cuda.Stream()
        _adopt(ref, s)
        bufs = so.Buffers(ref.dev, s)
        seqs = {n: _scratch_sequence(ref.dev, bufs, dt, n, m, 'n%d.' % n) for n in (384, 768)}
        torch.cuda.synchronize()
        for rep in range(2):
            bufs.poison()
            bufs.produce()
            s.synchronize()
            for n in (384, 768):
                so.run_calls(ref.dev, seqs[n][0], sync_each=True)
            s.synchronize()
        out = bufs.read()
        for n in (384, 768):
            seqs[n][1](out)
            alone[n] = _untagged(out, 'n%d.' % n)
        # what the whole chain of nine calls costs the host
        bufs.poison()
        bufs.produce()
        s.synchronize()
        t0 = time.perf_counter()
        for n in (384, 768, 384):
            so.run_calls(ref.dev, seqs[n][0])
        enqueue = time.perf_counter() - t0
        s.synchronize()
        ref.dev.set_stream(None)
    with variant_context(monkeypatch, tmp_path) as run:
        dev = run.dev
        s = torch.cuda.Stream()
        _adopt(run, s)
        bufs = so.Buffers(dev, s)
        order = [('A1.', 384), ('B.', 768), ('A2.', 384)]
        seqs = [_scratch_sequence(dev, bufs, dt, n, m, tag)[0] for tag, n in order]
        torch.cuda.synchronize()
        # warm-up on A alone: the side-stream probe of this (context, stream); the scratch stays at A's size
        bufs.poison()
        bufs.produce()
        s.synchronize()
        so.run_calls(dev, seqs[0])
        dev.sync()
        bufs.poison()
        s.synchronize()
        ms = so.busy_ms(enqueue)
        marker = so.busy(s, ms)
        bufs.produce()
        so.assert_busy(marker, 'just before the first library call')
        so.run_calls(dev, seqs[0])
        so.assert_busy(marker, "after problem A's last call")
        so.run_calls(dev, seqs[1][:2])
        so.assert_busy(marker, "after problem B's g3_potri, which regrew the event pool")
        so.run_calls(dev, seqs[1][2:])
        so.run_calls(dev, seqs[2])
        bufs.snapshot()
        s.synchronize()
        print('scratch %s: busy %.1f ms, enqueue %.3f ms' % (np.dtype(dt).name, ms, enqueue * 1e3))
        got, snaps = bufs.read(), bufs.read(snaps=True)
        dev.set_stream(None)
    for tag, n in order:
        so.assert_same_bits(_untagged(got, tag), alone[n], 'problem %s behind the others vs alone' % tag)
        so.assert_same_bits(_untagged(snaps, tag), alone[n], 'problem %s consumed on the stream vs alone' % tag)
    assert so.bulk_launches(ref.log) and so.bulk_launches(run.log)


# ------------------------------------------------------------------ 4. the program ring wrapped onto launches in flight
PROG_SLOTS = 8            # G3_PROG_SLOTS of g3_internal.h
RING_CALLS = 2 * PROG_SLOTS + 3


def _ring_spec(mode, i):
    """call i's program: variance and length-scale each a factor 1.5 from the next call's -- a swapped program is far outside
    any tolerance"""
    var, rate = 0.05 * 1.5 ** i, 0.02 * 1.5 ** i * so.RATE
    if mode == 'generated':
        return ('sum', ('prod', ('SE', var, rate, None), ('COS', 0.7, np.array([0.2, 0.3, 0.1]), None)), ('WN', 0.1 * var, None))
    return ('sum', ('SE', var, rate, None), ('NOISE', 0.1 * var))


RING_MODES = {'table': {}, 'generated': {}, 'nofast': {'G3_GRAM_NOFAST': 1}}


@pytest.mark.parametrize('dt', [F64, F32], ids=['float64', 'float32'])
@pytest.mark.parametrize('mode', list(RING_MODES))
def test_program_ring_wraps_onto_launches_in_flight(monkeypatch, tmp_path, mode, dt):
    """Behind one busy stretch, 2 x G3_PROG_SLOTS + 3 g3_gram calls at N = 130, each with its own program and its own output,
    a g3_gram_diag and a g3_gram_rows of the same program after each: every output must match the oracle for ITS program.
    `table`: g3_gram and g3_gram_rows take the compile-time kernel (parameters by value) and g3_gram_diag's uploads alone
    wrap the ring twice; `generated`: an expression outside the table, every call uploads; `nofast`: the table's expression
    under G3_GRAM_NOFAST=1, every call uploads.  The call that wraps the ring blocks on its slot's event -- the design -- so
    the marker has to be incomplete before the first call only."""
    import torch
    from oracle import g3_oracle as orc
    from g3py_amd.device import compile_spec
    N, Np, row0, nrows, d = 130, 256, 64, 66, so.D
    Xh = so.points(N, 3).astype(dt)
    X64 = Xh.astype(np.float64)
    code = so.code_of(dt)
    with variant_context(monkeypatch, tmp_path, **RING_MODES[mode]) as run:
        dev = run.dev
        lib, ctx = dev.lib, dev.ctx
        s = torch.cuda.Stream()
        _adopt(run, s)
        bufs = so.Buffers(dev, s)
        X = bufs.inp('X', Xh, dt)
        calls, refs = [], {}
        for i in range(RING_CALLS):
            spec = _ring_spec(mode, i)
            prog = compile_spec(spec, d)
            K, dg, Kr = bufs.out('K%d' % i, Np, Np, dt), bufs.out('diag%d' % i, 1, N, dt), bufs.out('rows%d' % i, nrows, row0 + nrows, dt)
            calls += [
                Call('g3_gram %d' % i, lambda prog=prog, K=K: lib.g3_gram(ctx, C.byref(prog), X.ptr, N, X.ld, None, 0, 0, d, code, K.ptr,
                                                                         K.ld, Np, Np, 2), False),
                Call('g3_gram_diag %d' % i, lambda prog=prog, dg=dg: lib.g3_gram_diag(ctx, C.byref(prog), X.ptr, N, X.ld, d, code, dg.ptr),
                     False),
                Call('g3_gram_rows %d' % i, lambda prog=prog, Kr=Kr: lib.g3_gram_rows(ctx, C.byref(prog), X.ptr, N, X.ld, d, row0, nrows,
                                                                                     code, Kr.ptr, Kr.ld, 2), False)]
            full = np.zeros((Np, Np))
            full[:N, :N] = orc.tt_to_num(orc.kernel_cov(spec, X64))
            refs[i] = full
        rtol, atol = so.GRAM_RTOL[dt == F64]

        def check(out, host):
            for i, full in refs.items():
                for name, want in (('K%d' % i, full), ('diag%d' % i, np.diag(full)[None, :N]),
                                   ('rows%d' % i, full[row0:row0 + nrows, :row0 + nrows])):
                    np.testing.assert_allclose(out[name], want, rtol=rtol, atol=atol, err_msg='%s %s' % (mode, name))
        torch.cuda.synchronize()
        so.run_passes(dev, s, bufs, calls, {}, check, 'ring %s-%s' % (mode, np.dtype(dt).name), snapshot=True)
        paths = dev.gram_path_stats()
        dev.set_stream(None)
    print('ring %s: Gram launches by path %r' % (mode, paths))
    if mode == 'table':
        assert paths['table'] > 0 and paths['generated'] + paths['interpreted'] == 0, paths
    else:
        assert paths['table'] == 0 and paths['generated'] + paths['interpreted'] > 0, paths


# ------------------------------------------------------------------ 5. changing streams, and the pivot flag across them
def test_results_do_not_depend_on_the_stream_the_context_works_on(monkeypatch, tmp_path):
    """One context, the two-stream potrf / trsm / row-sum sequence (n = 2176 under G3_NB=128 G3_SB=2, fp64) six times in a row:
    on torch stream s1, on s2, on the context's own stream, on s2, on s1, on its own -- the side stream is probed again at
    each change -- and the same under G3_PROBE=0: all twelve results are identical, and the first is checked against LAPACK.
    On s1 and s2 the calls are enqueued behind busy work (the probe synchronises, so the marker is asserted before the first
    call only); the context's own stream is not a torch stream: there the inputs are synchronised into place first."""
    import torch
    results = []
    for extra in ({}, {'G3_PROBE': 0}):
        with variant_context(monkeypatch, tmp_path, G3_NB=128, G3_SB=2, **extra) as run:
            dev = run.dev
            s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
            _adopt(run, s1)
            bufs = so.Buffers(dev, s1)
            calls, host, check = so.sweep_sequence(dev, bufs, F64, 2176, 128)
            torch.cuda.synchronize()
            for _ in range(2):
                bufs.poison()
                bufs.produce()
                s1.synchronize()
                t0 = time.perf_counter()
                so.run_calls(dev, calls)
                enqueue = time.perf_counter() - t0
                dev.sync()
            ms = so.busy_ms(enqueue)
            for leg in (s1, s2, None, s2, s1, None):
                bufs.stream = leg if leg is not None else s1
                dev.set_stream(leg.cuda_stream if leg is not None else None)
                bufs.poison()
                bufs.stream.synchronize()
                if leg is not None:
                    marker = so.busy(leg, ms)
                    bufs.produce()
                    so.assert_busy(marker, 'just before the first library call')
                else:
                    bufs.produce()
                    bufs.stream.synchronize()
                so.run_calls(dev, calls)
                dev.sync()
                results.append(bufs.read())
            print('streams %r: busy %.1f ms per leg on a torch stream, enqueue %.3f ms' % (extra, ms, enqueue * 1e3))
            dev.set_stream(None)
        assert so.bulk_launches(run.log)
    check(results[0], {})
    for i, r in enumerate(results[1:], 1):
        so.assert_same_bits(r, results[0], 'run %d vs run 0' % i)


BAD_N, BAD_AT = 512, 300


def _flag_operands(dev, b1, b2, dt=F64):
    """the operands of 5(b) / 5(c): a matrix with one planted non-positive pivot, a product, a solve and a good matrix"""
    Kbad = so.spd(BAD_N).copy()
    Kbad[BAD_AT, BAD_AT] = -5.0
    assert scipy.linalg.lapack.dpotrf(Kbad, lower=True)[1] == BAD_AT + 1
    rng = np.random.default_rng(5)
    ops = dict(
        Kbad=b1.inp('Kbad', Kbad, dt, output=True), Wbad=b1.out('Wbad', BAD_N, 128, dt),
        A=b2.inp('A', rng.standard_normal((128, 64)), dt), B=b2.inp('B', rng.standard_normal((128, 64)), dt),
        Cm=b2.inp('C', rng.standard_normal((128, 128)), dt, output=True),
        L=b2.inp('L', so.chol_of(256, 'float64')[1], dt), X=b2.inp('X', so.rhs(128, 256), dt, output=True),
        Kgood=b2.inp('Kgood', so.spd(BAD_N), dt, output=True), Wgood=b2.out('Wgood', BAD_N, 128, dt))
    return ops


def _check_flag_results(out, b2):
    A, B, Cm = (b2.staging[k].cpu().numpy() for k in ('A', 'B', 'C'))
    ref = Cm - 0.5 * A @ B.T
    err = np.abs(out['C'] - ref).max()
    print('gemm behind a failed pivot: max err %.3e' % err)
    assert err <= 5e-13 * np.abs(ref).max(), 'g3_gemm_nt behind a failed factorisation did not compute'      # tests/test_gpu_kernels.py
    _, Lr, cond = so.chol_of(BAD_N, 'float64')
    so.check_factor(so.spd(BAD_N), out['Kgood'], Lr, cond, F64, 'g3_potrf after a failed one')


def test_pivot_flag_of_a_failed_potrf_does_not_leak_across_streams(monkeypatch, tmp_path):
    """5(b): on s1, g3_potrf on a matrix with a planted non-positive pivot reports its 1-based index.  After
    g3_ctx_set_stream(s2), g3_gemm_nt and g3_trsm_rlt on good data must compute (a pivot flag left standing, or cleared on the
    stream the context has left, turns them into silent no-ops) and g3_potrf on an SPD matrix must report 0 and the right
    factor.  Every call is enqueued behind busy work on the stream it runs on."""
    import torch
    code = so.code_of(F64)
    with variant_context(monkeypatch, tmp_path) as run:
        dev = run.dev
        lib, ctx = dev.lib, dev.ctx
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        b1, b2 = so.Buffers(dev, s1), so.Buffers(dev, s2)
        o = _flag_operands(dev, b1, b2)
        torch.cuda.synchronize()
        info = C.c_int(-1)

        def potrf(K, W):
            assert lib.g3_potrf(ctx, K.ptr, BAD_N, K.ld, code, W.ptr, C.byref(info)) == 0
            return info.value
        on_s2 = [Call('g3_gemm_nt', lambda: lib.g3_gemm_nt(ctx, o['Cm'].ptr, 128, o['A'].ptr, 64, o['B'].ptr, 64, 128, 128, 64, -0.5, 1.0,
                                                          code, 0), False),
                 Call('g3_trsm_rlt', lambda: lib.g3_trsm_rlt(ctx, o['L'].ptr, 256, 256, o['X'].ptr, 128, 256, code, None), False)]
        ms = [so.BUSY_FLOOR_MS, so.BUSY_FLOOR_MS]
        for rep in range(3):             # two warm-up passes (the second is timed), then the pass behind busy work
            live = rep == 2
            dev.set_stream(s1.cuda_stream)
            b1.poison()
            s1.synchronize()
            if live:
                marker = so.busy(s1, ms[0])
            b1.produce()
            if live:
                so.assert_busy(marker, 'just before the failing g3_potrf')
            t0 = time.perf_counter()
            assert potrf(o['Kbad'], o['Wbad']) == BAD_AT + 1
            t1 = time.perf_counter() - t0
            dev.set_stream(s2.cuda_stream)
            b2.poison()
            s2.synchronize()
            if live:
                marker = so.busy(s2, ms[1])
            b2.produce()
            if live:
                so.assert_busy(marker, 'just before g3_gemm_nt')
            t0 = time.perf_counter()
            so.run_calls(dev, on_s2, marker=marker if live else None, after_each=True)
            assert potrf(o['Kgood'], o['Wgood']) == 0
            t2 = time.perf_counter() - t0
            s2.synchronize()
            if not live:                 # (in the live pass the two g3_potrf calls wait for the busy work: not an enqueue time)
                ms = [so.busy_ms(t1), so.busy_ms(t2)]
                enqueue = (t1, t2)
        print('flag (b): busy %.1f + %.1f ms, enqueue %.3f + %.3f ms' % (ms[0], ms[1], enqueue[0] * 1e3, enqueue[1] * 1e3))
        out = b2.read()
        dev.set_stream(None)
    _check_flag_results(out, b2)
    so.check_solve(so.chol_of(256, 'float64')[1], so.rhs(128, 256), out['X'], so.chol_of(256, 'float64')[2], F64,
                   'g3_trsm_rlt behind a failed factorisation')


def test_pivot_flag_of_a_failed_potrf_nowait_on_a_busy_stream(monkeypatch, tmp_path):
    """5(c): behind busy work on one stream, with no synchronisation: g3_potrf_nowait on the matrix with the planted pivot, a
    g3_gemm_nt on good data, a second g3_potrf_nowait on an SPD matrix with a fresh accumulator.  The first accumulator holds
    the planted index, the product is right, the second accumulator stays 0 and its factor is right."""
    import torch
    code = so.code_of(F64)
    with variant_context(monkeypatch, tmp_path) as run:
        dev = run.dev
        lib, ctx = dev.lib, dev.ctx
        s = torch.cuda.Stream()
        _adopt(run, s)
        bufs = so.Buffers(dev, s)
        o = _flag_operands(dev, bufs, bufs)
        acc1 = bufs.inp('acc1', np.zeros((1, 1), np.int32), np.int32, output=True)
        acc2 = bufs.inp('acc2', np.zeros((1, 1), np.int32), np.int32, output=True)
        calls = [Call('g3_potrf_nowait (planted pivot)', lambda: lib.g3_potrf_nowait(ctx, o['Kbad'].ptr, BAD_N, BAD_N, code, o['Wbad'].ptr,
                                                                                    acc1.ptr), False),
                 Call('g3_gemm_nt', lambda: lib.g3_gemm_nt(ctx, o['Cm'].ptr, 128, o['A'].ptr, 64, o['B'].ptr, 64, 128, 128, 64, -0.5, 1.0,
                                                          code, 0), False),
                 Call('g3_potrf_nowait (SPD)', lambda: lib.g3_potrf_nowait(ctx, o['Kgood'].ptr, BAD_N, BAD_N, code, o['Wgood'].ptr,
                                                                          acc2.ptr), False)]

        def check(out, host):
            assert int(out['acc1'][0, 0]) == BAD_AT + 1, out['acc1']
            assert int(out['acc2'][0, 0]) == 0, out['acc2']
            _check_flag_results(out, bufs)
        torch.cuda.synchronize()
        so.run_passes(dev, s, bufs, calls, {}, check, 'flag (c)', after_each=True, snapshot=True)
        dev.set_stream(None)
