"""Hostile memory for the tests of the C ABI's memory contracts (include/g3hip.h).

A test that hands a kernel zeroed buffers and a fresh context cannot see a load one tile too far (it is multiplied by
zero), a workspace that is assumed to be zero, a store one column past the documented extent, or a flag left over from an
earlier call.  The helpers here put every operand where such a defect shows:

  embed            a host array at the top-left of a larger device buffer; everything around it carries a fill:
                   NaN (byte 0xFF, a NaN in fp64 and fp32) around what must not be READ, a canary (byte 0xA5, finite and
                   recognisable) around what must not be WRITTEN.  An output / workspace is embedded without data: NaN
                   inside its documented extent, the canary outside.
  check_untouched  byte-wise: everything outside a mask of the elements that may change still holds what embed put there
  same_bits        byte equality of two results on the documented output region (NaNs compare)
  dirty_device     a second context whose scratch buffers, flags and statistics have all been used by larger problems

Layout of an embedded buffer (row-major, leading dimension ld > width):

      GUARD rows of fill | rows_total rows: [ the block | ld - width columns of fill ] | GUARD rows of fill

The bands are one 128-row tile above and below, and the slack columns of every row; a store one column (or 128 columns)
past the width lands in the slack or in the next row, a store up to 128 rows past either end lands in a band: it is
reported, and it never leaves the allocation.  Nothing here reads or writes outside a buffer it allocated.

The comparison logic (first_difference, first_nan, same_bits, lower_tile_mask ...) works on host arrays and is tested on
the CPU with a NumPy stand-in for the device (test_hostile_memory_host.py).
"""
import contextlib
import math
import os

import numpy as np

NAN_BYTE = 0xFF      # 0xFFFF... is a (quiet, negative) NaN in both dtypes
CANARY_BYTE = 0xA5   # 0xA5A5... is finite: -2.4e-130 in fp64, -2.9e-16 in fp32
GUARD = 128          # rows of fill above and below every embedded block: one tile


def slack(dtype):
    """columns of fill behind the width: ld = width + 64 (fp64) / + 96 (fp32) keeps rows 16-byte aligned while the row
    ends fall inside a 128-column tile, so vector and scalar epilogues both occur"""
    return 64 if np.dtype(dtype) == np.float64 else 96


def fill_value(byte, dtype):
    """the element that a buffer memset to `byte` holds"""
    return np.frombuffer(bytes([byte]) * np.dtype(dtype).itemsize, dtype=dtype)[0]


# --------------------------------------------------------------------------------------- host-side comparison logic
def _bits(a):
    """an integer view of a float array (same shape): bit patterns compare where NaNs would not"""
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def first_difference(a, b, mask=None):
    """(row, col) of the first element (row-major) whose BITS differ between a and b where mask is true (None: everywhere),
    or None"""
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    diff = _bits(a) != _bits(b)
    if mask is not None:
        diff &= np.atleast_2d(mask)
    if not diff.any():
        return None
    r, c = np.unravel_index(int(np.argmax(diff)), diff.shape)
    return int(r), int(c)


def first_nan(a, mask=None):
    """(row, col) of the first NaN of a where mask is true, or None"""
    a = np.atleast_2d(a)
    bad = np.isnan(a)
    if mask is not None:
        bad &= np.atleast_2d(mask)
    if not bad.any():
        return None
    r, c = np.unravel_index(int(np.argmax(bad)), bad.shape)
    return int(r), int(c)


def same_bits(a, b, mask=None, what=''):
    """assert byte equality of two results on the documented output region, and that the region absorbed no NaN"""
    at = first_difference(a, b, mask)
    if at is not None:
        a2, b2 = np.atleast_2d(a), np.atleast_2d(b)
        raise AssertionError('%s: bits differ at (row %d, col %d): %r != %r' % (what, at[0], at[1], a2[at], b2[at]))
    at = first_nan(b, mask)
    if at is not None:
        raise AssertionError('%s: NaN in the documented output region at (row %d, col %d)' % (what, at[0], at[1]))


def lower_tile_mask(n1pad, n2pad, tile_rows=64, tile_cols=128):
    """G3_GRAM_LOWER: the 64 x 128 tiles on or below the diagonal -- row block b (64 rows) has b // 2 + 1 column tiles"""
    bi = np.arange(n1pad)[:, None] // tile_rows
    bj = np.arange(n2pad)[None, :] // tile_cols
    return bj <= bi // (tile_cols // tile_rows)


def tril_mask(n, cols=None):
    return np.tril(np.ones((n, n if cols is None else cols), dtype=bool))


def reduction_bound(terms, n_terms):
    """n * 2^-52 * sum |terms|: n - 1 additions of a recursive sum in any order cost at most (n - 1) u sum|t| to first
    order with u = 2^-53; 2^-52 = 2 u leaves the higher orders and the rounding of each term (one product, already counted
    in the terms as computed) ample room"""
    return n_terms * 2.0 ** -52 * math.fsum(abs(t) for t in terms)


# --------------------------------------------------------------------------------------- embedded device buffers
class Owner:
    """One embedded buffer: the device allocation, where the block lies in it, and the host image of what embed() put
    there (the fill, and the data where there is some)."""

    def __init__(self, dev, buf, view, image, row0):
        self.dev, self.buf, self.view, self.image, self.row0 = dev, buf, view, image, row0

    def download_all(self):
        return self.dev.download(self.buf, self.buf.rows, self.buf.ld)

    def block(self, whole=None):
        """the rows_total x width block (a copy) out of a download of the whole buffer"""
        whole = self.download_all() if whole is None else whole
        return np.ascontiguousarray(whole[self.row0:self.row0 + self.view.rows, :self.view.cols])


def _memset(dev, arr, byte):
    rc = dev.lib.g3_memset(dev.ctx, arr.ptr, int(byte), arr.nbytes)
    assert rc == 0, 'g3_memset failed with status %d' % rc


def embed(dev, array, rows_total, ld, dtype, fill):
    """Put `array` (host, 2-D or 1-D = one row) at the top-left of a (GUARD + rows_total + GUARD) x ld device buffer whose
    every other element carries the byte `fill`.  `array` may instead be a (rows, cols) shape: an output or workspace of that
    documented extent, holding NaN (NAN_BYTE) inside it and `fill` outside.  Returns (view, owner):
    the DeviceArray (dev.wrap) of the rows_total x width block with leading dimension ld, and the Owner."""
    dtype = np.dtype(dtype)
    if isinstance(array, tuple):
        rows, cols = array
        data = None
    else:
        data = np.atleast_2d(np.asarray(array)).astype(dtype, copy=False)
        rows, cols = data.shape
    rows_total = max(int(rows_total), rows)
    ld = int(ld)
    assert ld >= cols, (ld, cols)
    buf = dev.alloc(GUARD + rows_total + GUARD, ld, dtype, ld=ld)
    _memset(dev, buf, fill)
    image = np.full((buf.rows, ld), fill_value(fill, dtype), dtype=dtype)
    if data is not None:
        image[GUARD:GUARD + rows, :cols] = data
    else:
        image[GUARD:GUARD + rows, :cols] = fill_value(NAN_BYTE, dtype)
    if rows and cols:
        # whole rows of the image, fill included: one contiguous copy
        part = np.ascontiguousarray(image[GUARD:GUARD + rows])
        rc = dev.lib.g3_memcpy_h2d(dev.ctx, buf.offset(GUARD), part.ctypes.data, part.nbytes)
        assert rc == 0, 'g3_memcpy_h2d failed with status %d' % rc
    view = dev.wrap(buf.offset(GUARD), rows_total, cols, ld, dtype, keep=buf)
    return view, Owner(dev, buf, view, image, GUARD)


def check_untouched(dev, owner, written_mask=None, what='', whole=None):
    """Everything of the owner's buffer outside `written_mask` (boolean, rows_total x width of the block: the elements that
    may change; None: nothing may) still holds, byte for byte, what embed() put there.  Reports the first offending
    (row, col), counted from the block's top-left (negative rows: the band above)."""
    whole = owner.download_all() if whole is None else whole
    keep = np.ones(whole.shape, dtype=bool)
    if written_mask is not None:
        m = np.atleast_2d(written_mask)
        assert m.shape[0] <= owner.view.rows and m.shape[1] <= owner.view.cols, (m.shape, owner.view.rows, owner.view.cols)
        keep[owner.row0:owner.row0 + m.shape[0], :m.shape[1]] &= ~m
    at = first_difference(whole, owner.image, keep)
    if at is not None:
        raise AssertionError('%s: element (row %d, col %d) outside the documented extent was written: %r -> %r (block is '
                             '%d x %d, ld %d)' % (what, at[0] - owner.row0, at[1], owner.image[at], whole[at],
                                                  owner.view.rows, owner.view.cols, owner.view.ld))
    return whole


# --------------------------------------------------------------------------------------- a context that has been used
@contextlib.contextmanager
def environment(**knobs):
    """set environment knobs of the library (read when a context is created) for the duration of the block"""
    old = {k: os.environ.get(k) for k in knobs}
    try:
        for k, v in knobs.items():
            os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def dirty_device(**knobs):
    """A second g3.Device(0) (the caller closes it) on which larger problems than any test needs have already run, with
    inputs of magnitude about 1e6: a gp_factor_predict at N = 1300, M = 300; a g3_potrf that returns info != 0 (a negative
    diagonal entry is an ordinary return value); a gp_factor_batched of 64 members at N = 300 with gp_cross_batched and
    gp_dlogp_batched on it; potrf_robust on a ragged n = 700.  Its workspace, block-inverse buffer, batch buffer,
    statistics, program ring and info flags are populated afterwards.  `knobs`: environment settings for the context."""
    import g3py_amd as g3
    from g3py_amd import _lib
    from g3py_amd.device import compile_spec
    with environment(**knobs):
        dev = g3.Device(0)
    rng = np.random.default_rng(20261020)
    big = 1e6
    dt, d = np.float64, 3
    spec = ('sum', ('SE', big, np.ones(d) / big, None), ('NOISE', 0.1 * big))
    prog, cross = compile_spec(spec, d), compile_spec(spec[1], d)

    # one-GPU sweep with prediction rows
    N, M = 1300, 300
    Np, Mp = _lib.roundup(N), _lib.roundup(M)
    # (inputs with a tile of zero rows behind them: a kernel that read too far would still stay inside the allocation)
    X = dev.upload(rng.uniform(0, big, (N, d)), pad_rows=N + GUARD)
    Xs = dev.upload(rng.uniform(0, big, (M, d)), pad_rows=M + GUARD)
    delta = dev.upload(big * rng.standard_normal(N), pad_cols=N + GUARD)
    K = dev.alloc(Np + 128 + Mp, Np, dt)
    W, a = dev.alloc_inverses(Np, dt), dev.alloc(1, Np, dt)
    mu, ss = dev.alloc(1, Mp, dt), dev.alloc(1, Mp, dt)
    st = dev.gp_factor_predict(prog, cross, X, N, d, delta, Xs, M, K, W, a, mu, ss)
    assert st['info'] == 0, st

    # a factorisation that fails: the info flag has been set and read
    A = rng.standard_normal((256, 64))
    S = big * (A @ A.T / 64 + np.eye(256))
    S[200, 200] = -big
    assert dev.potrf(dev.upload(S), 256) == 201

    # a chain of 64 members and its consumers
    B, N = 64, 300
    Np = _lib.roundup(N)
    progs = [compile_spec(('sum', ('SE', big * (1 + 0.01 * b), np.ones(d) / big, None), ('NOISE', 0.1 * big)), d)
             for b in range(B)]
    crosses = [compile_spec(('SE', big * (1 + 0.01 * b), np.ones(d) / big, None), d) for b in range(B)]
    deltas = dev.upload(big * rng.standard_normal((B, N)), pad_rows=B + 1)
    kstride = (Np + 128) * Np
    Kb = dev.alloc(B * (Np + 128), Np, dt)
    Wb, ab = dev.alloc(B * Np, 128, dt), dev.alloc(B, Np, dt)
    Xb, Xsb = dev.wrap(X.ptr, N, d, d, dt), dev.wrap(Xs.ptr, M, d, d, dt)
    out = dev.gp_factor_batched(progs, Xb, N, d, deltas, Kb, kstride, Wb, ab, raw=True)
    assert not out[:, 5].any(), out[:, 5]
    mub, ssb, kdb = (dev.alloc(B, Mp, dt) for _ in range(3))
    dev.gp_cross_batched(crosses, Xsb, M, Xb, N, d, Kb, kstride, Wb, ab, mub, ssb, kdb)
    Yb, Kib = dev.alloc(B * (Np + 128), Np, dt), dev.alloc(B * (Np + 128), Np, dt)
    alb = dev.alloc(B, Np, dt)
    dev.gp_dlogp_batched(progs, dev.grad_layout(progs[0]), Xb, N, d, Kb, kstride, Wb, ab, Yb, Kib, alb)

    # the robust factorisation of a ragged matrix (works in the context's workspace)
    n = 700
    A = rng.standard_normal((n, 100))
    Kr = dev.upload(big * (A @ A.T / 100 + np.eye(n)))
    Lr = dev.alloc(n, n, dt)
    dev.potrf_robust(Kr, Lr, n)
    dev.sync()
    for arr in (X, Xs, delta, K, W, a, mu, ss, deltas, Kb, Wb, ab, mub, ssb, kdb, Yb, Kib, alb, Kr, Lr):
        arr.free()
    return dev
