"""Device plumbing over the C ABI: contexts, device arrays, kernel-program compilation.

Nothing here computes on the CPU: every numerical routine is a call into libg3hip.so.
"""
import atexit
import ctypes as C
import sys
import weakref

import numpy as np

from . import _lib
from ._lib import G3Error, KernelProg, roundup


def _check(dev, rc, what):
    if rc != 0:
        msg = ''
        if rc == -1000 and dev is not None and dev.ctx:
            msg = ': ' + (dev.lib.g3_last_error(dev.ctx) or b'').decode()
        raise G3Error('%s failed with status %d%s' % (what, rc, msg))


class DeviceArray:
    """A row-major device matrix (rows x cols, leading dimension ld, in elements)."""

    def __init__(self, dev, ptr, rows, cols, ld, dtype, owned=True, keep=None):
        self.dev, self.ptr, self.rows, self.cols, self.ld = dev, ptr, int(rows), int(cols), int(ld)
        self.dtype = np.dtype(dtype)
        self.owned = owned
        self._keep = keep
        if owned and self.ptr:
            dev._owned.add(self)

    @property
    def nbytes(self):
        return self.rows * self.ld * self.dtype.itemsize

    def offset(self, row, col=0):
        return self.ptr + (row * self.ld + col) * self.dtype.itemsize

    def free(self):
        """hipFree an owned buffer; a no-op once the context is closed (Device.close() has already
        released everything the context owned, and nothing may call into HIP after that)"""
        if self.owned and self.ptr and self.dev.ctx:
            self.dev.lib.g3_free(self.dev.ctx, self.ptr)
        self.ptr = 0

    def __del__(self):
        # never call into the HIP runtime from interpreter finalisation: by then the runtime (or a
        # profiler tool library layered over it) may already be shutting down
        if sys is None or sys.is_finalizing():
            return
        try:
            self.free()
        except Exception:
            pass


class Device:
    """One g3_ctx on one GPU.  Raises if the library or the GPU is missing."""
    _default = {}
    _live = weakref.WeakSet()      # every open context, closed by the atexit hook below

    def __init__(self, index=0):
        self.ctx = None
        self._owned = weakref.WeakSet()
        self.lib = _lib.load()
        h = C.c_void_p()
        rc = self.lib.g3_ctx_create(int(index), C.byref(h))
        if rc != 0:
            raise G3Error('g3_ctx_create(device=%d) failed with status %d: no usable MI355X; '
                          'g3py_amd has no CPU fallback' % (index, rc))
        self.ctx = h
        self.index = index
        Device._live.add(self)

    @classmethod
    def default(cls, index=0):
        if index not in cls._default:
            cls._default[index] = cls(index)
        return cls._default[index]

    def close(self):
        """Release everything the context owns -- device buffers handed out by alloc()/upload(), the
        library's streams, events, pinned mirrors and workspaces -- while the HIP runtime is alive.
        Idempotent; afterwards DeviceArray.free() is a no-op and any other call raises."""
        if not self.ctx:
            return
        try:
            self.lib.g3_ctx_sync(self.ctx)
        except Exception:
            pass
        for a in list(self._owned):
            try:
                a.free()
            except Exception:
                pass
        self.lib.g3_ctx_destroy(self.ctx)
        self.ctx = None
        Device._live.discard(self)
        for k in [k for k, v in Device._default.items() if v is self]:
            del Device._default[k]

    def __del__(self):
        if sys is None or sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    @classmethod
    def close_all(cls):
        """explicit teardown of every live context (registered with atexit: Python's exit hooks run
        before the C runtime's static destructors, i.e. while HIP and any profiler tool are intact)"""
        for d in list(cls._live):
            try:
                d.close()
            except Exception:
                pass
        cls._default.clear()

    def set_stream(self, stream_handle):
        _check(self, self.lib.g3_ctx_set_stream(self.ctx, stream_handle), 'g3_ctx_set_stream')

    def sync(self):
        _check(self, self.lib.g3_ctx_sync(self.ctx), 'g3_ctx_sync')

    # ---- profiling (HIP events on the context's stream)
    def prof_enable(self, on=True):
        _check(self, self.lib.g3_prof_enable(self.ctx, int(on)), 'g3_prof_enable')

    def prof_reset(self):
        _check(self, self.lib.g3_prof_reset(self.ctx), 'g3_prof_reset')

    def prof_collect(self):
        out = (C.c_double * (3 * len(_lib.PROF_TAGS)))()
        _check(self, self.lib.g3_prof_collect(self.ctx, out), 'g3_prof_collect')
        return {t: dict(count=int(out[3 * i]), ms=out[3 * i + 1], work=out[3 * i + 2])
                for i, t in enumerate(_lib.PROF_TAGS)}

    # ---- memory
    def alloc(self, rows, cols, dtype, ld=None, zero=False):
        ld = int(cols if ld is None else ld)
        p = C.c_void_p()
        nbytes = int(rows) * ld * np.dtype(dtype).itemsize
        _check(self, self.lib.g3_malloc(self.ctx, nbytes, C.byref(p)), 'g3_malloc(%d)' % nbytes)
        a = DeviceArray(self, p.value or 0, rows, cols, ld, dtype)
        if zero and nbytes:
            _check(self, self.lib.g3_memset(self.ctx, a.ptr, 0, nbytes), 'g3_memset')
        return a

    def wrap(self, ptr, rows, cols, ld, dtype, keep=None):
        """Borrow foreign device memory (e.g. torch.Tensor.data_ptr())."""
        return DeviceArray(self, int(ptr), rows, cols, ld, dtype, owned=False, keep=keep)

    def upload(self, a, dtype=None, pad_rows=None, pad_cols=None):
        a = np.asarray(a)
        if dtype is not None:
            a = a.astype(dtype, copy=False)
        if a.ndim == 1:
            a = a[None, :]
        rows, cols = a.shape
        pr = rows if pad_rows is None else int(pad_rows)
        pc = cols if pad_cols is None else int(pad_cols)
        if (pr, pc) != (rows, cols):
            b = np.zeros((pr, pc), dtype=a.dtype)
            b[:rows, :cols] = a
            a = b
        a = np.ascontiguousarray(a)
        d = self.alloc(pr, pc, a.dtype)
        if a.nbytes:
            _check(self, self.lib.g3_memcpy_h2d(self.ctx, d.ptr, a.ctypes.data, a.nbytes), 'g3_memcpy_h2d')
        d.rows, d.cols = pr, pc
        return d

    def copy_in(self, d, a):
        """host array -> an existing device buffer of the same shape"""
        a = np.ascontiguousarray(a, dtype=d.dtype)
        if a.nbytes > d.nbytes:
            raise G3Error('copy_in: %d bytes do not fit in a buffer of %d' % (a.nbytes, d.nbytes))
        if a.nbytes:
            _check(self, self.lib.g3_memcpy_h2d(self.ctx, d.ptr, a.ctypes.data, a.nbytes), 'g3_memcpy_h2d')

    def download(self, d, rows=None, cols=None):
        rows = d.rows if rows is None else rows
        cols = d.cols if cols is None else cols
        full = np.empty((d.rows, d.ld), dtype=d.dtype)
        if full.nbytes:
            _check(self, self.lib.g3_memcpy_d2h(self.ctx, full.ctypes.data, d.ptr, full.nbytes), 'g3_memcpy_d2h')
        return np.ascontiguousarray(full[:rows, :cols])

    def gram_path_stats(self):
        """Gram launches of this context so far by kernel: compile-time table / generated at first use / interpreted"""
        out = (C.c_double * 3)()
        _check(self, self.lib.g3_gram_path_stats(self.ctx, out), 'g3_gram_path_stats')
        return {'table': int(out[0]), 'generated': int(out[1]), 'interpreted': int(out[2])}

    def grad_path_stats(self):
        """the same for the gradient's kernel-parameter sums"""
        out = (C.c_double * 3)()
        _check(self, self.lib.g3_grad_path_stats(self.ctx, out), 'g3_grad_path_stats')
        return {'table': int(out[0]), 'generated': int(out[1]), 'interpreted': int(out[2])}

    # ---- kernels (thin, argument-checked wrappers)
    def gram(self, prog, X1, X2, d, out, n1pad, n2pad, flags):
        dt = _lib.dtype_code(out.dtype)
        rc = self.lib.g3_gram(self.ctx, C.byref(prog), X1.ptr, X1.rows, X1.ld,
                              X2.ptr if X2 is not None else None, X2.rows if X2 is not None else 0,
                              X2.ld if X2 is not None else 0, d, dt, out.ptr, out.ld, n1pad, n2pad, flags)
        _check(self, rc, 'g3_gram')

    def gram_diag(self, prog, X, d, out):
        rc = self.lib.g3_gram_diag(self.ctx, C.byref(prog), X.ptr, X.rows, X.ld, d,
                                   _lib.dtype_code(out.dtype), out.ptr)
        _check(self, rc, 'g3_gram_diag')

    def cov_lift(self, K, n):
        _check(self, self.lib.g3_cov_lift(self.ctx, K.ptr, n, K.ld, _lib.dtype_code(K.dtype)), 'g3_cov_lift')

    def scrub(self, A, n1, n2):
        _check(self, self.lib.g3_scrub(self.ctx, A.ptr, n1, n2, A.ld, _lib.dtype_code(A.dtype)), 'g3_scrub')

    def gemm_nt(self, Cm, A, B, m, n, k, alpha=1.0, beta=0.0, lower_only=False, c_off=0, a_off=0, b_off=0):
        rc = self.lib.g3_gemm_nt(self.ctx, Cm.ptr + c_off, Cm.ld, A.ptr + a_off, A.ld, B.ptr + b_off, B.ld,
                                 m, n, k, alpha, beta, _lib.dtype_code(Cm.dtype), int(lower_only))
        _check(self, rc, 'g3_gemm_nt')

    def gemm_nt_stair(self, c_ptr, ldc, a_ptr, lda, b_ptr, ldb, k, seg_rows, seg_cols, dtype, alpha=1.0, beta=0.0,
                      b_block_rows=0, b_perm=None, seg_diag=None):
        """one launch over stacked row segments: segment s gets its first seg_cols[s] columns;
        b_perm[s] = physical position of logical row block s of B (blocks of b_block_rows rows);
        seg_diag[s] != 0: the last seg_rows[s] columns of segment s are its diagonal block (lower triangle wanted)"""
        n = len(seg_rows)
        rows = (C.c_int64 * n)(*[int(v) for v in seg_rows])
        cols = (C.c_int64 * n)(*[int(v) for v in seg_cols])
        perm, nperm = None, 0
        if b_perm is not None:
            nperm = len(b_perm)
            perm = (C.c_int32 * nperm)(*[int(v) for v in b_perm])
        diag = (C.c_int64 * n)(*[int(v) for v in seg_diag]) if seg_diag is not None else None
        rc = self.lib.g3_gemm_nt_stair(self.ctx, c_ptr, ldc, a_ptr, lda, b_ptr, ldb, k, rows, cols, n, alpha, beta,
                                       _lib.dtype_code(dtype), int(b_block_rows), perm, nperm, diag)
        _check(self, rc, 'g3_gemm_nt_stair')

    def potrf(self, A, n):
        info = C.c_int(0)
        rc = self.lib.g3_potrf(self.ctx, A.ptr, n, A.ld, _lib.dtype_code(A.dtype), None, C.byref(info))
        _check(self, rc, 'g3_potrf')
        return info.value

    def potrf_robust(self, K, L, n, maxtries=20):
        tries, fb, jit = C.c_int(0), C.c_int(0), C.c_double(0)
        rc = self.lib.g3_potrf_robust(self.ctx, K.ptr, K.ld, L.ptr, L.ld, n, _lib.dtype_code(K.dtype),
                                      maxtries, C.byref(tries), C.byref(fb), C.byref(jit))
        _check(self, rc, 'g3_potrf_robust')
        return tries.value, bool(fb.value), jit.value

    def potrf_robust_batched(self, K, kstride, L, lstride, batch, n, maxtries=20):
        """potrf_robust for `batch` n x n matrices `kstride` elements apart in K, factors `lstride` apart in L (each lower
        and zero elsewhere within its roundup(n, 128)-square slot); n <= 256 runs the jitter schedule on the device, one
        launch for the batch.  Returns (tries, fallback, jitter) arrays of length batch."""
        B = int(batch)
        tries, fb, jit = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.float64)
        rc = self.lib.g3_potrf_robust_batched(self.ctx, K.ptr, K.ld, int(kstride), L.ptr, L.ld, int(lstride), B, n,
                                              _lib.dtype_code(K.dtype), maxtries, tries.ctypes.data_as(C.POINTER(C.c_int)),
                                              fb.ctypes.data_as(C.POINTER(C.c_int)),
                                              jit.ctypes.data_as(C.POINTER(C.c_double)))
        _check(self, rc, 'g3_potrf_robust_batched')
        return tries, fb.astype(bool), jit

    def trsm_rlt(self, L, n, B, m, have_inverses=False):
        rc = self.lib.g3_trsm_rlt(self.ctx, L.ptr, n, L.ld, B.ptr, m, B.ld, _lib.dtype_code(L.dtype), None)
        _check(self, rc, 'g3_trsm_rlt')

    def logp_terms(self, L, n, a):
        out = (C.c_double * 4)()
        rc = self.lib.g3_logp_terms(self.ctx, L.ptr, n, L.ld, a.ptr if a is not None else None,
                                    _lib.dtype_code(L.dtype), out)
        _check(self, rc, 'g3_logp_terms')
        return list(out)

    def rows_dot_ss(self, V, m, n, a, dot, ss):
        rc = self.lib.g3_rows_dot_ss(self.ctx, V.ptr, m, n, V.ld, a.ptr if a is not None else None,
                                     _lib.dtype_code(V.dtype), dot.ptr if dot is not None else None,
                                     ss.ptr if ss is not None else None)
        _check(self, rc, 'g3_rows_dot_ss')

    def alloc_inverses(self, Np, dtype):
        """buffer for the 128 x 128 diagonal-block inverses that belong to one factor"""
        return self.alloc(Np // _lib.G3_PAD * _lib.G3_PAD, _lib.G3_PAD, dtype)

    def gp_factor(self, prog, X, N, d, delta, K, W, a):
        """K must have roundup(N) + 128 rows (the trailing block carries delta through the factorisation)"""
        if K.rows < roundup(N) + _lib.G3_RHS_PAD:
            raise G3Error('g3_gp_factor needs a K buffer with roundup(N) + 128 rows')
        out = (C.c_double * 6)()
        rc = self.lib.g3_gp_factor(self.ctx, C.byref(prog), X.ptr, N, X.ld, d, delta.ptr,
                                   _lib.dtype_code(K.dtype), K.ptr, K.ld, W.ptr, a.ptr, out)
        _check(self, rc, 'g3_gp_factor')
        return dict(logdet=out[0], quad=out[1], nonfinite=out[2], tries=int(out[3]),
                    fallback=bool(out[4]), info=int(out[5]))

    def gp_factor_predict(self, prog, prog_cross, X, N, d, delta, Xs, M, K, W, a, mu, ss):
        """K must have roundup(N) + 128 + roundup(M, 128) rows"""
        out = (C.c_double * 6)()
        rc = self.lib.g3_gp_factor_predict(self.ctx, C.byref(prog), C.byref(prog_cross), X.ptr, N, X.ld, d, delta.ptr,
                                           Xs.ptr, M, Xs.ld, _lib.dtype_code(K.dtype), K.ptr, K.ld, W.ptr, a.ptr,
                                           mu.ptr, ss.ptr, out)
        _check(self, rc, 'g3_gp_factor_predict')
        return dict(logdet=out[0], quad=out[1], nonfinite=out[2], tries=int(out[3]),
                    fallback=bool(out[4]), info=int(out[5]))

    @staticmethod
    def _progs(progs):
        """the members' programs as a ctypes array: a list of KernelProg, or an array packed earlier (long chains: packing
        4096 programs costs more than evaluating them)"""
        return progs if isinstance(progs, C.Array) else (_lib.KernelProg * len(progs))(*progs)

    @staticmethod
    def _fields_args(name, tmpl, offsets, fields):
        """the members as template + fields (see compile_spec_rows): the leading arguments of a g3_*_batched_fields call
        behind the context, up to nfield (the two pointers keep the converted arrays alive), and the number of rows"""
        fields = np.ascontiguousarray(fields, dtype=np.float64)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        B, nf = fields.shape
        if len(offsets) != nf:
            raise G3Error('%s: %d offsets for %d fields' % (name, len(offsets), nf))
        return B, (C.byref(tmpl), B, fields.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p), nf)

    @staticmethod
    def _factor_args(B, X, N, d, delta, K, kstride, W, a):
        out = np.empty((B, 6))
        return out, (X.ptr, N, X.ld, d, delta.ptr, delta.ld, _lib.dtype_code(K.dtype), K.ptr, K.ld, kstride, W.ptr, a.ptr,
                     out.ctypes.data_as(C.POINTER(C.c_double)))

    def gp_factor_batched(self, progs, X, N, d, delta, K, kstride, W, a, raw=False):
        """len(progs) evaluations in one sweep; K holds the members `kstride` elements apart.  `progs`: a list of
        KernelProg or an existing ctypes array of them; raw=True returns the (B, 6) array
        [logdet, quad, nonfinite, tries, fallback, info] instead of dicts"""
        arr = self._progs(progs)
        out, args = self._factor_args(len(arr), X, N, d, delta, K, kstride, W, a)
        _check(self, self.lib.g3_gp_factor_batched(self.ctx, arr, len(arr), *args), 'g3_gp_factor_batched')
        if raw:
            return out
        return [dict(logdet=r[0], quad=r[1], nonfinite=r[2], tries=int(r[3]), fallback=bool(r[4]), info=int(r[5]))
                for r in out]

    def gp_factor_batched_fields(self, tmpl, offsets, fields, X, N, d, delta, K, kstride, W, a):
        """gp_factor_batched with the members given as one template program plus a (B, nfield) float64 matrix of the
        values that differ and the byte offsets in g3_kernel_prog they belong at (see compile_spec_rows); the library
        expands the programs on the device.  Returns the raw (B, 6) statistics."""
        B, members = self._fields_args('gp_factor_batched_fields', tmpl, offsets, fields)
        out, args = self._factor_args(B, X, N, d, delta, K, kstride, W, a)
        _check(self, self.lib.g3_gp_factor_batched_fields(self.ctx, *members, *args), 'g3_gp_factor_batched_fields')
        return out

    def gp_cross(self, prog, Xs, M, X, N, d, L, W, a, V, mu, ss):
        rc = self.lib.g3_gp_cross(self.ctx, C.byref(prog), Xs.ptr, M, Xs.ld, X.ptr, N, X.ld, d, L.ptr, L.ld,
                                  W.ptr, a.ptr if a is not None else None, _lib.dtype_code(L.dtype), V.ptr, V.ld,
                                  mu.ptr if mu is not None else None, ss.ptr if ss is not None else None)
        _check(self, rc, 'g3_gp_cross')

    # ---- appending observations to a factor (include/g3hip_online.h)
    def copy2d(self, dst, src, rows, cols):
        """dst[:rows, :cols] <- src[:rows, :cols] on the device (stream-ordered)"""
        rc = self.lib.g3_copy2d(self.ctx, dst.ptr, dst.ld, src.ptr, src.ld, int(rows), int(cols), _lib.dtype_code(dst.dtype))
        _check(self, rc, 'g3_copy2d')

    def gp_append(self, prog, X, N0, N1, d, delta, K, W, a):
        """after gp_factor (or gp_append) on the first N0 rows of X, with tries = 0, no fallback and info = 0: the factor, its
        block inverses and a for the first N1 rows.  K needs roundup(N1) + 128 rows of ld >= roundup(N1), W roundup(N1) / 128
        blocks, a and delta N1 entries (delta is read from rounddown(N0, 128) on).  Returns gp_factor's dict plus `refused`:
        True when the diagonal of the N1 points would have been lifted (nothing was written); with `refused` or a non-zero
        `info` the caller refits."""
        if K.rows < roundup(N1) + _lib.G3_RHS_PAD:
            raise G3Error('g3_gp_append needs a K buffer with roundup(N1) + 128 rows')
        out = (C.c_double * 8)()
        rc = self.lib.g3_gp_append(self.ctx, C.byref(prog), X.ptr, N0, N1, X.ld, d, delta.ptr, _lib.dtype_code(K.dtype),
                                   K.ptr, K.ld, W.ptr, a.ptr, out)
        _check(self, rc, 'g3_gp_append')
        return dict(logdet=out[0], quad=out[1], nonfinite=out[2], tries=int(out[3]), fallback=bool(out[4]), info=int(out[5]),
                    refused=bool(out[6]))

    def gp_cross_append(self, prog, Xs, M, X, N0, N1, d, L, W, a, V, mu, ss):
        """after gp_append from N0 to N1 rows: extend the cross solve gp_cross left in V (ld >= roundup(N1)) for the same Xs
        and program by the new columns, and recompute mu and ss over all of them; stream-ordered"""
        rc = self.lib.g3_gp_cross_append(self.ctx, C.byref(prog), Xs.ptr, M, Xs.ld, X.ptr, N0, N1, X.ld, d, L.ptr, L.ld,
                                         W.ptr, a.ptr if a is not None else None, _lib.dtype_code(L.dtype), V.ptr, V.ld,
                                         mu.ptr if mu is not None else None, ss.ptr if ss is not None else None)
        _check(self, rc, 'g3_gp_cross_append')

    @staticmethod
    def _ptr(a):
        return a.ptr if a is not None else None

    def _cross_args(self, Xs, M, X, N, d, K, kstride, W, a, mu, ss, kdiag):
        out = next(o for o in (mu, ss, kdiag) if o is not None)
        return (Xs.ptr, M, Xs.ld, X.ptr, N, X.ld, d, self._ptr(K), K.ld if K is not None else 0, kstride, self._ptr(W),
                self._ptr(a), _lib.dtype_code(out.dtype), self._ptr(mu), self._ptr(ss), self._ptr(kdiag))

    def gp_cross_batched(self, progs, Xs, M, X, N, d, K, kstride, W, a, mu, ss, kdiag):
        """after gp_factor_batched on the same buffers: per member b, mu[b] = V_b a_b, ss[b] = |rows of V_b|^2 for
        V_b = K_b(Xs, X) L_b^-T and kdiag[b] = diag K_b(Xs, Xs), each a device (B, roundup(M, 128)) matrix or None.
        With mu and ss both None the factor buffers K, W, a may be None too (the prior needs no factorisation)."""
        arr = self._progs(progs)
        args = self._cross_args(Xs, M, X, N, d, K, kstride, W, a, mu, ss, kdiag)
        _check(self, self.lib.g3_gp_cross_batched(self.ctx, arr, len(arr), *args), 'g3_gp_cross_batched')

    def gp_cross_batched_fields(self, tmpl, offsets, fields, Xs, M, X, N, d, K, kstride, W, a, mu, ss, kdiag):
        """gp_cross_batched for members given as template + fields (see compile_spec_rows), after
        gp_factor_batched_fields on the same buffers"""
        _, members = self._fields_args('gp_cross_batched_fields', tmpl, offsets, fields)
        args = self._cross_args(Xs, M, X, N, d, K, kstride, W, a, mu, ss, kdiag)
        _check(self, self.lib.g3_gp_cross_batched_fields(self.ctx, *members, *args), 'g3_gp_cross_batched_fields')

    def _draws_args(self, Xs, M, X, N, d, K, kstride, W, a, lift, loc, Z, Cm, Lp, maxtries):
        dtype = Xs.dtype
        Z = np.ascontiguousarray(Z, dtype=dtype)
        loc = np.ascontiguousarray(loc, dtype=dtype)
        if Z.ndim != 3 or Z.shape[1] != M or loc.shape != (Z.shape[0], M):
            raise G3Error('gp_draws_batched: loc must be (B, M) and Z (B, M, S)')
        B, _, S = Z.shape
        out = np.empty((B, M, S), dtype=dtype)
        tries, fb, jit = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.float64)
        args = (Xs.ptr, M, Xs.ld, self._ptr(X), N, X.ld if X is not None else 0, d, self._ptr(K),
                K.ld if K is not None else 0, int(kstride), self._ptr(W), self._ptr(a), _lib.dtype_code(dtype), int(bool(lift)),
                loc.ctypes.data, Z.ctypes.data, S, out.ctypes.data, self._ptr(Cm), self._ptr(Lp), int(maxtries),
                tries.ctypes.data_as(C.POINTER(C.c_int)), fb.ctypes.data_as(C.POINTER(C.c_int)),
                jit.ctypes.data_as(C.POINTER(C.c_double)))
        return B, args, (out, tries, fb, jit), (loc, Z)      # the last: only keeps the converted host arrays alive over the call

    def gp_draws_batched(self, progs, Xs, M, X, N, d, K, kstride, W, a, lift, loc, Z, Cm=None, Lp=None, maxtries=20):
        """after gp_factor_batched on the same buffers: per member b one set of joint draws loc[b] + mu_b + Lp_b Z[b] with
        Lp_b = cholesky_robust(K_b(Xs, Xs) - V_b V_b^T) (lift: the noise kernel's tt_to_cov on K_b(Xs, Xs)).  loc (B, M) and
        Z (B, M, S) are host arrays; Cm / Lp: optional device (B * Mp, Mp) buffers for the covariances and factors.  With
        K None the draws come from the prior.  Returns (out (B, M, S), tries, fallback, jitter)."""
        arr = self._progs(progs)
        B, args, res, keep = self._draws_args(Xs, M, X, N, d, K, kstride, W, a, lift, loc, Z, Cm, Lp, maxtries)
        if len(arr) != B:
            raise G3Error('gp_draws_batched: %d programs for %d members' % (len(arr), B))
        _check(self, self.lib.g3_gp_draws_batched(self.ctx, arr, B, *args), 'g3_gp_draws_batched')
        return res[0], res[1], res[2].astype(bool), res[3]

    def gp_draws_batched_fields(self, tmpl, offsets, fields, Xs, M, X, N, d, K, kstride, W, a, lift, loc, Z, Cm=None, Lp=None,
                                maxtries=20):
        """gp_draws_batched for members given as template + fields (see compile_spec_rows), after
        gp_factor_batched_fields on the same buffers"""
        rows, members = self._fields_args('gp_draws_batched_fields', tmpl, offsets, fields)
        B, args, res, keep = self._draws_args(Xs, M, X, N, d, K, kstride, W, a, lift, loc, Z, Cm, Lp, maxtries)
        if rows != B:
            raise G3Error('gp_draws_batched_fields: %d field rows for %d members' % (rows, B))
        _check(self, self.lib.g3_gp_draws_batched_fields(self.ctx, *members, *args), 'g3_gp_draws_batched_fields')
        return res[0], res[1], res[2].astype(bool), res[3]

    @staticmethod
    def _dlogp_args(B, gmap, X, N, d, K, kstride, W, a, Y, Kinv, alpha):
        out = np.empty((B, max(gmap.nslots, 1)))
        return out, (C.byref(gmap), X.ptr, N, X.ld, d, K.ptr, K.ld, kstride, W.ptr, a.ptr, _lib.dtype_code(K.dtype), Y.ptr,
                     Kinv.ptr, alpha.ptr, out.ctypes.data_as(C.POINTER(C.c_double)))

    def gp_dlogp_batched(self, progs, gmap, X, N, d, K, kstride, W, a, Y, Kinv, alpha):
        """after gp_factor_batched: per member K^-1, alpha and the kernel-parameter sums; returns (B, nslots)"""
        arr = self._progs(progs)
        out, args = self._dlogp_args(len(arr), gmap, X, N, d, K, kstride, W, a, Y, Kinv, alpha)
        _check(self, self.lib.g3_gp_dlogp_batched(self.ctx, arr, len(arr), *args), 'g3_gp_dlogp_batched')
        return out[:, :gmap.nslots]

    def gp_dlogp_batched_fields(self, tmpl, offsets, fields, gmap, X, N, d, K, kstride, W, a, Y, Kinv, alpha):
        """gp_dlogp_batched for members given as template + fields (after gp_factor_batched_fields on the same buffers);
        returns (B, nslots)"""
        B, members = self._fields_args('gp_dlogp_batched_fields', tmpl, offsets, fields)
        out, args = self._dlogp_args(B, gmap, X, N, d, K, kstride, W, a, Y, Kinv, alpha)
        _check(self, self.lib.g3_gp_dlogp_batched_fields(self.ctx, *members, *args), 'g3_gp_dlogp_batched_fields')
        return out[:, :gmap.nslots]

    def gp_sample(self, L, M, loc, Z):
        """loc[:, None] + L Z for host normals Z (M x S); L is the padded device factor"""
        Z = np.ascontiguousarray(Z, dtype=L.dtype)
        loc = np.ascontiguousarray(loc, dtype=L.dtype)
        S = Z.shape[1]
        out = np.empty((M, S), dtype=L.dtype)
        rc = self.lib.g3_gp_sample(self.ctx, L.ptr, M, L.ld, loc.ctypes.data, Z.ctypes.data, S,
                                   _lib.dtype_code(L.dtype), out.ctypes.data)
        _check(self, rc, 'g3_gp_sample')
        return out

    # ---- gradient of logp
    def grad_layout(self, prog):
        m = _lib.GradMap()
        _check(self, self.lib.g3_grad_layout(C.byref(prog), C.byref(m)), 'g3_grad_layout')
        return m

    def potri(self, L, n, W, Y, Kinv):
        rc = self.lib.g3_potri(self.ctx, L.ptr, n, L.ld, W.ptr if W is not None else None,
                               _lib.dtype_code(L.dtype), Y.ptr, Y.ld, Kinv.ptr, Kinv.ld)
        _check(self, rc, 'g3_potri')

    def gram_grad(self, prog, gmap, X, N, d, Kinv, alpha):
        out = (C.c_double * max(gmap.nslots, 1))()
        rc = self.lib.g3_gram_grad(self.ctx, C.byref(prog), C.byref(gmap), X.ptr, N, X.ld, d,
                                   _lib.dtype_code(Kinv.dtype), Kinv.ptr, Kinv.ld, alpha.ptr, out)
        _check(self, rc, 'g3_gram_grad')
        return np.array(out[:gmap.nslots])

    def gram_grad_rows(self, prog, gmap, X, N, d, row0, nrows, Kinv_rows, alpha):
        """rows [row0, row0 + nrows) of gram_grad's sum; Kinv_rows holds those rows of K^-1"""
        out = (C.c_double * max(gmap.nslots, 1))()
        rc = self.lib.g3_gram_grad_rows(self.ctx, C.byref(prog), C.byref(gmap), X.ptr, N, X.ld, d,
                                        _lib.dtype_code(Kinv_rows.dtype), row0, nrows, Kinv_rows.ptr, Kinv_rows.ld,
                                        alpha.ptr, out)
        _check(self, rc, 'g3_gram_grad_rows')
        return np.array(out[:gmap.nslots])

    def gp_dlogp(self, prog, gmap, X, N, d, L, W, a, Y, Kinv, alpha):
        """after gp_factor: K^-1, alpha = K^-1 delta and 1/2 sum G_ij dK_ij/dparam per slot"""
        out = (C.c_double * max(gmap.nslots, 1))()
        rc = self.lib.g3_gp_dlogp(self.ctx, C.byref(prog), C.byref(gmap), X.ptr, N, X.ld, d, L.ptr, L.ld, W.ptr,
                                  a.ptr, _lib.dtype_code(L.dtype), Y.ptr, Y.ld, Kinv.ptr, Kinv.ld, alpha.ptr, out)
        _check(self, rc, 'g3_gp_dlogp')
        return np.array(out[:gmap.nslots])

    # ---- leave-one-out predictions from the factor
    def gp_loo(self, N, L, W, a, Y, alpha, kdiag):
        """after gp_factor: Y <- L^-T, alpha = K^-1 delta and kdiag = diag K^-1 (roundup(N) entries each, 0 from N on);
        stream-ordered, the caller downloads"""
        rc = self.lib.g3_gp_loo(self.ctx, L.ptr, N, L.ld, W.ptr, a.ptr, _lib.dtype_code(L.dtype), Y.ptr, Y.ld, alpha.ptr,
                                kdiag.ptr)
        _check(self, rc, 'g3_gp_loo')

    def gp_loo_batched(self, B, N, K, kstride, W, a, Y, alpha, kdiag):
        """after gp_factor_batched(_fields) on the same buffers: alpha and kdiag of every member, (B, roundup(N)) device
        matrices; Y (one roundup(N)-square workspace) is needed above N = 256 only and may be None below"""
        rc = self.lib.g3_gp_loo_batched(self.ctx, int(B), K.ptr, N, K.ld, int(kstride), W.ptr, a.ptr, _lib.dtype_code(K.dtype),
                                        self._ptr(Y), alpha.ptr, kdiag.ptr)
        _check(self, rc, 'g3_gp_loo_batched')

    # ---- gradients of the posterior pieces with respect to the query inputs
    def gp_cross_dx(self, prog, Xs, M, X, N, d, alpha, V, Y, W, dmu, dss):
        """after gp_loo (Y = L^-T, alpha = K^-1 delta) and gp_cross (V) for the same Xs and program:
        dmu[i, c] = sum_j alpha_j d1_c k(xs_i, x_j) and dss[i, c] = 2 sum_j W_ij d1_c k(xs_i, x_j), W = V Y^T (roundup(M) x
        roundup(N) workspace), into M x d device matrices; either output may be None, and alpha is needed for dmu only, V, Y
        and W for dss only.  Stream-ordered, the caller downloads"""
        out = dmu if dmu is not None else dss
        rc = self.lib.g3_gp_cross_dx(self.ctx, C.byref(prog), Xs.ptr, M, Xs.ld, X.ptr, N, X.ld, d, _lib.dtype_code(X.dtype),
                                     self._ptr(alpha), self._ptr(V), V.ld if V is not None else 0, self._ptr(Y),
                                     Y.ld if Y is not None else 0, self._ptr(W), W.ld if W is not None else 0, self._ptr(dmu),
                                     self._ptr(dss), out.ld if out is not None else 0)
        _check(self, rc, 'g3_gp_cross_dx')

    def gram_diag_dx(self, prog, Xs, M, d, dk):
        """dk[i, c] = d k(x, x) / d x_c at x = xs_i (M x d device matrix): the derivative of gram_diag's output"""
        rc = self.lib.g3_gram_diag_dx(self.ctx, C.byref(prog), Xs.ptr, M, Xs.ld, d, _lib.dtype_code(dk.dtype), dk.ptr, dk.ld)
        _check(self, rc, 'g3_gram_diag_dx')

    # ---- leave-fold-out cross-validation from the factor
    def gp_cv(self, N, L, W, a, Y, Kinv, alpha, idx, ptr, resid, pvar):
        """after gp_factor: K^-1 and alpha as gp_dlogp leaves them, then for the folds idx[ptr[f]:ptr[f + 1]] (int32 indices,
        int64 pointers) resid = A_II^-1 alpha_I and pvar = diag A_II^-1 scattered to the observations (roundup(N) entries each,
        0 in no fold and from N on); returns (fold, info): fold (F, 2) = log det A_II and alpha_I^T A_II^-1 alpha_I, info (F,) the
        folds' pivot flags.  Synchronises; the caller downloads resid and pvar"""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        ptr = np.ascontiguousarray(ptr, dtype=np.int64)
        F = len(ptr) - 1
        fold, info = np.empty((max(F, 1), 2)), np.zeros(max(F, 1), dtype=np.int32)
        rc = self.lib.g3_gp_cv(self.ctx, L.ptr, N, L.ld, W.ptr, a.ptr, _lib.dtype_code(L.dtype), Y.ptr, Y.ld, Kinv.ptr, Kinv.ld,
                               alpha.ptr, idx.ctypes.data, ptr.ctypes.data, F, resid.ptr, pvar.ptr, fold.ctypes.data,
                               info.ctypes.data)
        _check(self, rc, 'g3_gp_cv')
        return fold[:F], info[:F]

    # ---- gradient of the leave-one-out log predictive
    def gp_dloo(self, prog, gmap, X, N, d, L, W, a, Y, Kinv, alpha, kdiag, u):
        """after gp_factor: K^-1, alpha = K^-1 delta, kdiag = diag K^-1, u = K^-1 (alpha / kdiag) (roundup(N) entries each,
        0 from N on) and sum_ij W_ij dK_ij/dparam per slot, W the covariance adjoint of the leave-one-out score"""
        out = (C.c_double * max(gmap.nslots, 1))()
        rc = self.lib.g3_gp_dloo(self.ctx, C.byref(prog), C.byref(gmap), X.ptr, N, X.ld, d, L.ptr, L.ld, W.ptr, a.ptr,
                                 _lib.dtype_code(L.dtype), Y.ptr, Y.ld, Kinv.ptr, Kinv.ld, alpha.ptr, kdiag.ptr, u.ptr, out)
        _check(self, rc, 'g3_gp_dloo')
        return np.array(out[:gmap.nslots])

    def gp_dloo_batched_fields(self, tmpl, offsets, fields, gmap, X, N, d, K, kstride, W, a, Y, Kinv, alpha, kdiag, u):
        """gp_dloo for members given as template + fields (after gp_factor_batched_fields on the same buffers); alpha,
        kdiag and u are (B, roundup(N)) device matrices; returns (B, nslots)"""
        B, members = self._fields_args('gp_dloo_batched_fields', tmpl, offsets, fields)
        out, args = self._dlogp_args(B, gmap, X, N, d, K, kstride, W, a, Y, Kinv, alpha)
        _check(self, self.lib.g3_gp_dloo_batched_fields(self.ctx, *members, *args[:-1], kdiag.ptr, u.ptr, args[-1]),
               'g3_gp_dloo_batched_fields')
        return out[:, :gmap.nslots]

    # ---- reverse mode through the factor (CholeskyRobust.grad, tensors.py:224-260)
    def potrf_vjp(self, L, Lbar, n, Kbar):
        """Kbar (n x n: lower triangle, zeros above) <- the covariance adjoint of Lbar = d f / d L at the factor L; only
        the lower triangles of L and Lbar are read; stream-ordered, the caller downloads"""
        rc = self.lib.g3_potrf_vjp(self.ctx, L.ptr, L.ld, Lbar.ptr, Lbar.ld, n, _lib.dtype_code(L.dtype), Kbar.ptr, Kbar.ld)
        _check(self, rc, 'g3_potrf_vjp')

    def gram_vjp(self, prog, gmap, X, N, d, Kbar):
        """sum over the lower triangle of Kbar_ij d prog(x_i, x_j) / d param per slot of gmap"""
        out = (C.c_double * max(gmap.nslots, 1))()
        rc = self.lib.g3_gram_vjp(self.ctx, C.byref(prog), C.byref(gmap), X.ptr, N, X.ld, d, _lib.dtype_code(Kbar.dtype),
                                  Kbar.ptr, Kbar.ld, out)
        _check(self, rc, 'g3_gram_vjp')
        return np.array(out[:gmap.nslots])


atexit.register(Device.close_all)


# --------------------------------------------------------------------------- kernel programs
def _expand(spec, leaves):
    """Expand a kernel spec tree (see g3py_amd.processes.hypers.kernels.Kernel.spec) into
    shift + sum_p coef_p * prod leaf  (KernelSum/Prod/Scale/Shift, kernels.py:192-244)."""
    op = spec[0]
    if op == 'sum':
        c1, t1 = _expand(spec[1], leaves)
        c2, t2 = _expand(spec[2], leaves)
        return c1 + c2, t1 + t2
    if op == 'prod':
        c1, t1 = _expand(spec[1], leaves)
        c2, t2 = _expand(spec[2], leaves)
        terms = [(a * b, fa + fb) for a, fa in t1 for b, fb in t2]
        if c1 != 0.0:
            terms += [(c1 * b, fb) for b, fb in t2]
        if c2 != 0.0:
            terms += [(c2 * a, fa) for a, fa in t1]
        return c1 * c2, terms
    if op == 'scale':
        c, t = _expand(spec[2], leaves)
        e = float(spec[1])
        return e * c, [(e * a, f) for a, f in t]
    if op == 'shift':
        c, t = _expand(spec[2], leaves)
        return float(spec[1]) + c, t
    leaves.append(spec)
    return 0.0, [(1.0, (len(leaves) - 1,))]


def spec_leaves(spec):
    """the leaves of a spec tree in the order compile_spec numbers them"""
    leaves = []
    _expand(spec, leaves)
    return leaves


# leaf kind -> which entry of the leaf's spec tuple feeds the `rate` / `alpha` / `freq` fields of g3_leaf (entry 1 is always
# `var`).  compile_spec, compile_spec_rows and the slot -> hyper routing of dlogp (processes/gaussian.py) all read it.  DOT =
# (var, rate, bias, p, dims) and NN = (var, rate, bias, dims) keep their bias in `alpha`; p is structure (freq[0], no gradient slot).
LEAF_FIELDS = {'SE': dict(rate=2), 'OU': dict(rate=2), 'MAT32': dict(rate=2), 'MAT52': dict(rate=2),
               'RQ': dict(rate=2, alpha=3), 'COS': dict(freq=2), 'SINC': dict(freq=2),
               'SIN': dict(freq=2, rate=3), 'SM': dict(freq=2, rate=3), 'NOISE': {}, 'WN': {},
               'DOT': dict(rate=2, alpha=3), 'NN': dict(rate=2, alpha=3), 'BW': {}, 'VAR': {}}


def compile_spec(spec, d):
    """spec tree -> g3_kernel_prog for an input with d columns."""
    leaves = []
    shift, terms = _expand(spec, leaves)
    if len(leaves) > _lib.G3_MAXLEAF or len(terms) > _lib.G3_MAXPROD:
        raise G3Error('kernel expression too large for one g3_kernel_prog (%d leaves, %d products)'
                      % (len(leaves), len(terms)))
    if d > _lib.G3_MAXCOLS:
        raise G3Error('inputs with more than %d columns are not supported' % _lib.G3_MAXCOLS)
    prog = KernelProg()
    prog.nleaf, prog.nprod, prog.shift = len(leaves), len(terms), float(shift)
    for i, lf in enumerate(leaves):
        L = prog.leaf[i]
        kind = lf[0]
        L.kind = _lib.KINDS[kind]
        L.var = float(lf[1])
        if kind in ('NOISE', 'VAR'):
            # these read no column: the index list they carry is cut at what a leaf holds, or an input of more than
            # G3_MAXD columns could have no noise term
            dims = np.arange(min(d, _lib.G3_MAXD))
        else:
            dims = np.arange(d) if lf[-1] is None else np.atleast_1d(np.asarray(lf[-1])).astype(int)
        dims = np.where(dims < 0, dims + d, dims)
        if len(dims) > _lib.G3_MAXD or (len(dims) and (dims.min() < 0 or dims.max() >= d)):
            raise G3Error('bad dims for kernel leaf %s' % kind)
        L.ndims = len(dims)
        for k, c in enumerate(dims):
            L.dims[k] = int(c)

        def put(dst, v):
            v = np.broadcast_to(np.asarray(v, dtype=np.float64), (len(dims),))
            for k in range(len(dims)):
                dst[k] = float(v[k])
        for member, idx in LEAF_FIELDS[kind].items():
            if member == 'alpha':
                L.alpha = float(lf[idx])
            else:
                put(getattr(L, member), lf[idx])
        if kind == 'DOT':
            p_exp = lf[4]
            if float(p_exp) != int(p_exp) or not 1 <= int(p_exp) <= _lib.G3_DOT_MAXP:
                raise G3Error('the exponent of a DOT leaf must be an integer in 1 .. %d (got %r)' % (_lib.G3_DOT_MAXP, p_exp))
            L.freq[0] = float(int(p_exp))
    for p, (coef, fac) in enumerate(terms):
        if len(fac) > _lib.G3_MAXFAC:
            raise G3Error('product of more than %d kernels is not supported' % _lib.G3_MAXFAC)
        prog.prod[p].coef = float(coef)
        prog.prod[p].nfac = len(fac)
        for k, f in enumerate(fac):
            prog.prod[p].fac[k] = int(f)
    return prog


class Rows(np.ndarray):
    """a hyper value with a leading axis over chain rows (marks batched values apart from constants in a spec)"""


def compile_spec_rows(spec_rows, spec0, d, B):
    """(template, offsets, fields) for gp_factor_batched_fields: `spec_rows` is a spec tree whose free hyper values are
    Rows arrays (B, ...), `spec0` the same tree for row 0.  Scale / shift constants are not hypers, so products and
    the shift are the template's; every Rows leaf value becomes field columns."""
    tmpl = compile_spec(spec0, d)
    leaves = spec_leaves(spec_rows)
    leaf0 = KernelProg.leaf.offset
    lsz = C.sizeof(_lib.Leaf)
    offs, cols = [], []

    def put(i, member, v, n):
        if not isinstance(v, Rows):
            return
        v = np.broadcast_to(np.asarray(v, dtype=np.float64).reshape(B, -1), (B, n))
        base = leaf0 + i * lsz + getattr(_lib.Leaf, member).offset
        for k in range(n):
            offs.append(base + 8 * k)
            cols.append(v[:, k])
    for i, lf in enumerate(leaves):
        kind, nd = lf[0], int(tmpl.leaf[i].ndims)
        put(i, 'var', lf[1], 1)
        for member, idx in LEAF_FIELDS[kind].items():     # (the exponent of a DOT leaf is not in the table: it stays the template's)
            put(i, member, lf[idx], 1 if member == 'alpha' else nd)
    fields = np.stack(cols, axis=1) if cols else np.zeros((B, 0))
    return tmpl, np.asarray(offs, dtype=np.int32), np.ascontiguousarray(fields)
