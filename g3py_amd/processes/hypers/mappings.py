"""Warping maps on the path: Identity, LinearMapping, LogShifted, BoxCoxLinear, ArcsinhLinear
(g3py/processes/hypers/mappings.py:88-215, 309-333): element-wise O(N) host arithmetic
(`__call__`, `inv`, `logdet_dinv`) around the device path.

Every formula is written once.  Its parameters come from `param`, so with plain hyper values it is the one-row result
and with the Rows values of a chain block the (B, ...) result; sums run over axis=-1 (the observations)."""
import numpy as np

from . import Hypers, Slot, param as _param, per_row as _per_row, row_blocks as _row_blocks, each_row as _each_row


def _power(a, p):
    """a ** p with the exponent handed to np.power as a full array: with a scalar (or a broadcast, stride-0) exponent
    NumPy switches to square / sqrt at exactly 2.0 / 0.5, and one row and B rows of a chain would differ in the last bit"""
    e = np.empty(np.broadcast(a, p).shape, dtype=a.dtype)     # (either may carry the row axis alone: a slot given as a
    e[...] = p                                                # constant has none)
    return np.power(a, e)


class Mapping(Hypers):
    # True: `__call__`, `inv`, `logdet_dinv` and `grad` broadcast over Rows hyper values (read through `param`), and the
    # `*_rows` forms below call them on blocks of rows (`row_blocks`).  A user-defined mapping inherits False and is
    # evaluated row by row.
    BROADCASTS = False

    def __call__(self, x, values=None):
        raise NotImplementedError

    def inv(self, y, values=None):
        raise NotImplementedError

    def logdet_dinv(self, y, values=None):
        raise NotImplementedError

    def grad(self, y, values=None):
        """[(hyper, d inv(y) / d hyper (length N), d logdet_dinv(y) / d hyper)] in natural space:
        the pieces th_dlogp needs from the warping (mappings.py:88-215, 309-333 differentiated)"""
        return []

    def inv_rows(self, y, values_rows, B):
        """inv(y) for B rows of hyper values at once -> (B, N)"""
        if not self.BROADCASTS:
            return np.stack([np.asarray(r, dtype=y.dtype) for r in _each_row(self.inv, y, values_rows, B)])
        out = np.empty((B, y.shape[0]), dtype=y.dtype)
        for lo, hi, v in _row_blocks(values_rows, B, y.shape[0]):
            out[lo:hi] = self.inv(y, v)
        return out

    def logdet_dinv_rows(self, y, values_rows, B):
        with np.errstate(all='ignore'):
            if not self.BROADCASTS:
                return np.asarray(_each_row(self.logdet_dinv, y, values_rows, B), dtype=y.dtype)
            out = np.empty(B, dtype=y.dtype)
            for lo, hi, v in _row_blocks(values_rows, B, y.shape[0]):
                out[lo:hi] = self.logdet_dinv(y, v)
        return out

    def grad_rows(self, y, values_rows, B):
        """grad for B rows of hyper values: [(hyper, (B, N), (B,))]"""
        if not self.BROADCASTS:
            rows = _each_row(self.grad, y, values_rows, B)
            return [(rows[0][i][0], np.stack([np.asarray(p[i][1], dtype=np.float64) for p in rows]),
                     np.array([float(p[i][2]) for p in rows])) for i in range(len(rows[0]) if rows else 0)]
        out = None
        for lo, hi, v in _row_blocks(values_rows, B, y.shape[0]):
            per = self.grad(y, v)
            if out is None:
                out = [(h, np.empty((B, y.shape[0]), dtype=np.asarray(dinv).dtype), np.empty(B, dtype=np.asarray(dlogdet).dtype))
                       for h, dinv, dlogdet in per]
            for (_, dinv_rows, dlogdet_rows), (_, dinv, dlogdet) in zip(out, per):
                dinv_rows[lo:hi], dlogdet_rows[lo:hi] = dinv, dlogdet
        return out or []


class Identity(Mapping):
    BROADCASTS = True

    def __call__(self, x, values=None):
        return x

    def inv(self, y, values=None):
        return y

    def logdet_dinv(self, y, values=None):
        return 0.0


class LinearMapping(Mapping):
    BROADCASTS = True
    SLOTS = (Slot('shift', False, '_shift'), Slot('scale', True, '_scale'))

    def default_hypers(self, x=None, y=None):
        return {self.shift: 0.0, self.scale: 1.0}

    def _p(self, values, t):
        return _param(self.shift, values, t), _param(self.scale, values, t)

    def __call__(self, x, values=None):
        shift, scale = self._p(values, x.dtype.type)
        return scale * (x - shift)

    def inv(self, y, values=None):
        shift, scale = self._p(values, y.dtype.type)
        return y / scale + shift

    def logdet_dinv(self, y, values=None):
        shift, scale = self._p(values, y.dtype.type)
        return -y.dtype.type(y.shape[0]) * np.log(_per_row(scale))

    def grad(self, y, values=None):
        t = y.dtype.type
        shift, scale = self._p(values, t)
        return [(self.shift, np.ones_like(y), t(0)), (self.scale, -y / scale ** 2, -t(y.shape[0]) / _per_row(scale))]


class LogShifted(Mapping):
    BROADCASTS = True
    SLOTS = (Slot('shift', False, '_shift'),)

    def default_hypers(self, x=None, y=None):
        return {self.shift: y.min() - 1}

    def __call__(self, x, values=None):
        return np.exp(x) + _param(self.shift, values, x.dtype.type)

    def inv(self, y, values=None):
        t = y.dtype.type
        return np.log(np.maximum(y - _param(self.shift, values, t), t(np.float32(1e-32))))

    def logdet_dinv(self, y, values=None):
        with np.errstate(all='ignore'):
            return -np.sum(np.log(y - _param(self.shift, values, y.dtype.type)), axis=-1)

    def grad(self, y, values=None):
        t = y.dtype.type
        z = y - _param(self.shift, values, t)
        with np.errstate(all='ignore'):
            return [(self.shift, np.where(z > t(np.float32(1e-32)), -1 / z, t(0)), np.sum(1 / z, axis=-1))]


class BoxCoxLinear(Mapping):
    BROADCASTS = True
    SLOTS = (Slot('shift', False, '_shift'), Slot('scale', True, '_scale'), Slot('power', True, '_power'))

    def default_hypers(self, x=None, y=None):
        return {self.shift: 1.0, self.scale: 1.0, self.power: 1.0}

    def _p(self, values, t):
        return _param(self.shift, values, t), _param(self.scale, values, t), _param(self.power, values, t)

    def __call__(self, x, values=None):
        t = x.dtype.type
        shift, scale, power = self._p(values, t)
        scaled = power * x + t(1)
        transformed = np.sign(scaled) * _power(np.abs(scaled), t(1) / power)
        return transformed / scale - shift

    def inv(self, y, values=None):
        t = y.dtype.type
        shift, scale, power = self._p(values, t)
        shifted = scale * (y + shift)
        logs = power < np.float32(1e-5)                    # per row: the log limit of the transform
        with np.errstate(all='ignore'):
            r = ((np.sign(shifted) * _power(np.abs(shifted), power)) - t(1)) / power
            return np.where(logs, np.log(shifted), r) if logs.any() else r

    def logdet_dinv(self, y, values=None):
        t = y.dtype.type
        shift, scale, power = self._p(values, t)
        with np.errstate(all='ignore'):
            return (_per_row(power - t(1)) * np.sum(np.log(np.abs(scale * (y + shift))), axis=-1)
                    + t(y.shape[0]) * np.log(_per_row(scale)))

    def grad(self, y, values=None):
        t = y.dtype.type
        shift, scale, power = self._p(values, t)
        n = t(y.shape[0])
        sh = scale * (y + shift)
        with np.errstate(all='ignore'):
            a = np.abs(sh)
            sp = np.sign(sh) * _power(a, power)
            am1 = _power(a, power - 1)
            d_shift, d_scale = am1 * scale, am1 * (y + shift)
            d_power = (sp * np.log(a) * power - (sp - 1)) / power ** 2
            logs = power < np.float32(1e-5)                # per row: the log limit of the transform
            if logs.any():
                d_shift, d_scale = np.where(logs, scale / sh, d_shift), np.where(logs, (y + shift) / sh, d_scale)
                d_power = np.where(logs, t(0), d_power)
            return [(self.shift, d_shift, _per_row(power - 1) * np.sum(1 / (y + shift), axis=-1)),
                    (self.scale, d_scale, _per_row(power * n / scale)),
                    (self.power, d_power, np.sum(np.log(a), axis=-1))]


class ArcsinhLinear(Mapping):
    BROADCASTS = True
    SLOTS = (Slot('shift', False, '_shift'), Slot('scale', True, '_scale'))

    def default_hypers(self, x=None, y=None):
        return {self.shift: np.mean(y), self.scale: np.std(y)}

    def _p(self, values, t):
        return _param(self.shift, values, t), _param(self.scale, values, t)

    def __call__(self, x, values=None):
        shift, scale = self._p(values, x.dtype.type)
        return np.sinh((x - shift) / scale)

    def inv(self, y, values=None):
        shift, scale = self._p(values, y.dtype.type)
        return np.arcsinh(y) * scale + shift

    def logdet_dinv(self, y, values=None):
        t = y.dtype.type
        shift, scale = self._p(values, t)
        return t(y.shape[0]) * np.log(_per_row(scale)) - t(0.5) * np.sum(np.log1p(y ** 2), axis=-1)

    def grad(self, y, values=None):
        t = y.dtype.type
        shift, scale = self._p(values, t)
        return [(self.shift, np.ones_like(y), t(0)), (self.scale, np.arcsinh(y), t(y.shape[0]) / _per_row(scale))]
