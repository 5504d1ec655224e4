"""CPU tests of tests/hostile_memory.py: the checker is not vacuous.  A NumPy stand-in for the device (host memory behind
the same alloc / wrap / download / g3_memset / g3_memcpy_h2d interface) lets embed and check_untouched run unchanged; the
"kernels" are NumPy stores through a view of the fake allocation.  A planted write into a band is caught, a planted write
inside the mask is allowed, a result that absorbed a NaN is reported.

The second half checks the error bound that test_gpu_memory_contracts.py asserts for the reduction kernels on a NumPy
emulation of each kernel's summation order, so the bound is the reference's and not a fitted one."""
import ctypes as C
import math

import numpy as np
import pytest

import hostile_memory as hm


class _FakeLib:
    """the three memory calls of the C ABI on host addresses"""

    @staticmethod
    def g3_memset(ctx, ptr, byte, nbytes):
        C.memset(ptr, byte, nbytes)
        return 0

    @staticmethod
    def g3_memcpy_h2d(ctx, dst, src, nbytes):
        C.memmove(dst, src, nbytes)
        return 0


class _FakeArray:
    def __init__(self, ptr, rows, cols, ld, dtype, keep=None):
        self.ptr, self.rows, self.cols, self.ld, self.dtype, self._keep = ptr, rows, cols, ld, np.dtype(dtype), keep

    @property
    def nbytes(self):
        return self.rows * self.ld * self.dtype.itemsize

    def offset(self, row, col=0):
        return self.ptr + (row * self.ld + col) * self.dtype.itemsize

    def host(self):
        """a live NumPy view (rows x ld) of the memory: what a kernel would store through"""
        buf = (C.c_char * self.nbytes).from_address(self.ptr)
        return np.frombuffer(buf, dtype=self.dtype).reshape(self.rows, self.ld)


class FakeDevice:
    ctx = None
    lib = _FakeLib()

    def alloc(self, rows, cols, dtype, ld=None, zero=False):
        ld = cols if ld is None else ld
        raw = np.zeros(rows * ld * np.dtype(dtype).itemsize + 16, dtype=np.uint8)
        return _FakeArray(raw.ctypes.data, rows, cols, ld, dtype, keep=raw)

    def wrap(self, ptr, rows, cols, ld, dtype, keep=None):
        return _FakeArray(ptr, rows, cols, ld, dtype, keep=keep)

    def download(self, d, rows=None, cols=None):
        rows = d.rows if rows is None else rows
        cols = d.cols if cols is None else cols
        return np.array(d.host()[:rows, :cols])


DTYPES = [np.float64, np.float32]


@pytest.mark.parametrize('dt', DTYPES)
def test_fills_are_what_the_names_say(dt):
    assert np.isnan(hm.fill_value(hm.NAN_BYTE, dt))
    c = hm.fill_value(hm.CANARY_BYTE, dt)
    assert np.isfinite(c) and c != 0
    assert hm.GUARD >= 128 and hm.slack(dt) * np.dtype(dt).itemsize % 16 == 0


@pytest.mark.parametrize('dt', DTYPES)
def test_embed_lays_the_block_out_as_documented(dt):
    dev = FakeDevice()
    A = np.arange(15, dtype=dt).reshape(3, 5)
    view, owner = hm.embed(dev, A, rows_total=7, ld=5 + hm.slack(dt), dtype=dt, fill=hm.NAN_BYTE)
    assert (view.rows, view.cols, view.ld) == (7, 5, 5 + hm.slack(dt))
    whole = owner.download_all()
    assert whole.shape == (7 + 2 * hm.GUARD, view.ld)
    np.testing.assert_array_equal(whole[hm.GUARD:hm.GUARD + 3, :5], A)
    outside = np.ones(whole.shape, bool)
    outside[hm.GUARD:hm.GUARD + 3, :5] = False
    assert np.isnan(whole[outside]).all()
    np.testing.assert_array_equal(dev.download(view, 3, 5), A)           # the view addresses the block
    hm.check_untouched(dev, owner)                                       # nothing ran: nothing changed
    # an output: NaN inside its extent, the canary around it
    out, oo = hm.embed(dev, (4, 6), rows_total=4, ld=6 + hm.slack(dt), dtype=dt, fill=hm.CANARY_BYTE)
    whole = oo.download_all()
    assert np.isnan(whole[hm.GUARD:hm.GUARD + 4, :6]).all()
    whole[hm.GUARD:hm.GUARD + 4, :6] = 0
    assert (whole[:hm.GUARD] == hm.fill_value(hm.CANARY_BYTE, dt)).all() and np.isfinite(whole).all()


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('where', ['slack_column', 'row_below', 'row_above', 'inside_block_outside_mask', 'input_data'])
def test_a_planted_write_outside_the_mask_is_caught_and_located(dt, where):
    dev = FakeDevice()
    n, ld = 6, 6 + hm.slack(dt)
    if where == 'input_data':
        view, owner = hm.embed(dev, np.ones((n, n), dt), n, ld, dt, hm.NAN_BYTE)
    else:
        view, owner = hm.embed(dev, (n, n), n, ld, dt, hm.CANARY_BYTE)
    mask = hm.tril_mask(n)                                               # the "kernel" may write the lower triangle
    mem = owner.buf.host()
    mem[hm.GUARD:hm.GUARD + n, :n][mask] = 2.0                           # the legitimate stores
    hm.check_untouched(dev, owner, mask)
    r, c = {'slack_column': (2, n), 'row_below': (n, 1), 'row_above': (-1, 3), 'inside_block_outside_mask': (1, 4),
            'input_data': (0, 5)}[where]
    mem[hm.GUARD + r, c] = 3.0
    with pytest.raises(AssertionError, match=r'\(row %d, col %d\)' % (r, c)):
        hm.check_untouched(dev, owner, mask)


@pytest.mark.parametrize('dt', DTYPES)
def test_a_store_of_the_fill_value_elsewhere_and_a_sign_flip_are_seen_bytewise(dt):
    """the comparison is on bits: a NaN with another payload in a NaN band, or -0.0 over 0.0, is a write"""
    dev = FakeDevice()
    view, owner = hm.embed(dev, np.zeros((4, 4), dt), 4, 4 + hm.slack(dt), dt, hm.NAN_BYTE)
    mem = owner.buf.host()
    mem[hm.GUARD + 5, 0] = np.nan                                        # the canonical quiet NaN is not 0xFF..FF
    with pytest.raises(AssertionError, match=r'\(row 5, col 0\)'):
        hm.check_untouched(dev, owner)
    mem[hm.GUARD + 5, 0] = hm.fill_value(hm.NAN_BYTE, dt)
    hm.check_untouched(dev, owner)
    mem[hm.GUARD + 1, 1] = -0.0
    with pytest.raises(AssertionError, match=r'\(row 1, col 1\)'):
        hm.check_untouched(dev, owner)


def test_same_bits_compares_nans_as_bits_and_reports_absorbed_nans():
    a = np.array([[1.0, np.nan, 3.0], [4.0, 5.0, 6.0]])
    region = np.array([[True, False, True], [True, True, False]])
    hm.same_bits(a, a.copy(), region, 'equal')                           # the NaN lies outside the region
    b = a.copy()
    b[1, 2] = 7.0
    hm.same_bits(a, b, region, 'difference outside the region')
    b[1, 1] = np.nextafter(5.0, 6.0)                                     # one unit in the last place, inside the region
    with pytest.raises(AssertionError, match=r'bits differ at \(row 1, col 1\)'):
        hm.same_bits(a, b, region, 'ulp')
    # a hostile run that absorbed a NaN: equal bits would not help, and differing bits are reported first
    c = a.copy()
    c[0, 2] = np.nan
    with pytest.raises(AssertionError, match=r'bits differ at \(row 0, col 2\)'):
        hm.same_bits(a, c, region, 'absorbed')
    with pytest.raises(AssertionError, match=r'NaN in the documented output region at \(row 0, col 2\)'):
        hm.same_bits(c, c.copy(), region, 'both runs NaN')
    with pytest.raises(AssertionError, match=r'NaN in the documented output region at \(row 0, col 1\)'):
        hm.same_bits(a, a.copy(), None, 'whole array')
    assert hm.first_difference(np.array([0.0]), np.array([-0.0])) == (0, 0)
    assert hm.first_nan(np.array([1.0, 2.0])) is None


def test_lower_tile_mask_is_the_gram_kernels_tile_walk():
    """row block b of 64 rows owns the column tiles 0 .. b // 2 of 128 columns (g3_gram with G3_GRAM_LOWER)"""
    m = hm.lower_tile_mask(384, 384)
    want = np.zeros((384, 384), bool)
    for b in range(6):
        want[64 * b:64 * (b + 1), :128 * (b // 2 + 1)] = True
    np.testing.assert_array_equal(m, want)
    assert hm.tril_mask(384)[m].sum() == hm.tril_mask(384).sum()         # the whole lower triangle is inside
    assert hm.lower_tile_mask(128, 128).all() and not hm.lower_tile_mask(256, 256)[:128, 128:].any()


# ------------------------------------------------------------------ the bound of the reduction tests, on the CPU
def _emulated_block_sum(terms, threads):
    """the kernels' order: thread t adds terms t, t + threads, ... in turn; the 64 lanes of a wave are combined by a
    butterfly (pairwise), the waves' sums in order"""
    terms = np.asarray(terms, dtype=np.float64)
    part = np.zeros(threads)
    for t in range(min(threads, len(terms))):
        s = 0.0
        for v in terms[t::threads]:
            s += v
        part[t] = s
    waves = part.reshape(-1, 64)
    step = 32
    while step:
        waves = waves[:, :step] + waves[:, step:2 * step]
        step //= 2
    total = 0.0
    for w in waves[:, 0]:
        total += w
    return total


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('n,threads', [(1, 1024), (63, 1024), (1023, 1024), (1024, 1024), (1025, 1024), (2049, 1024),
                                        (1, 256), (255, 256), (256, 256), (257, 256), (1000, 256)])
def test_the_reduction_bound_covers_the_kernels_summation_order(dt, n, threads):
    rng = np.random.default_rng(n + threads)
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(dt).astype(np.float64)
    a = rng.standard_normal(n).astype(dt).astype(np.float64)
    for terms in (x * x, x * a, np.log(np.abs(x) + 1e-3), x):
        got = _emulated_block_sum(terms, threads)
        ref = math.fsum(terms)
        assert abs(got - ref) <= hm.reduction_bound(terms, n), (got, ref)
        # ... and the result stored as fp32 adds one rounding of the output type
        assert abs(float(np.float32(got)) - ref) <= hm.reduction_bound(terms, n) + 2.0 ** -24 * abs(ref)
