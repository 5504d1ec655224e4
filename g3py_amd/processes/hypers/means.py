"""Location functions on the path: Zero, Bias, Linear
(g3py/processes/hypers/means.py:6-27, 117-159).  O(N d) host arithmetic feeding the device
path; `eval` takes natural-space hyper values -- one row of them, or the Rows values of a chain block (read through
`param`: the same formula then gives (B, N))."""
import numpy as np

from . import Hypers, Slot, param as _param, as_rows as _as_rows, each_row as _each_row


class Mean(Hypers):
    # True: `eval` broadcasts over Rows hyper values and `rows` is one call of it.  A user-defined mean inherits False and
    # is evaluated row by row.
    BROADCASTS = False

    def eval(self, x, values):
        raise NotImplementedError

    def __call__(self, x, values=None):
        x = np.asarray(x)
        return self.eval(x[:, self.dims] if self.dims is not None else x, values or {})

    def rows(self, x, values_rows, B):
        """m(x) for B rows of hyper values at once (values_rows[name][j] = row j) -> (B, N)"""
        if not self.BROADCASTS:
            return np.stack(_each_row(self, x, values_rows, B))
        return np.broadcast_to(self(x, _as_rows(values_rows)), (B, len(x)))

    # True only for means that are linear in their hypers (d m(x) / d hyper does not depend on the hyper values): the chain
    # gradient then evaluates `jac` once for all rows.  A user-defined mean inherits False and takes the per-row loop.
    JAC_CONSTANT = False

    def jac(self, x, values):
        """[(hyper, d m(x) / d hyper as an N x size array)] for the free hypers -- what Theano's
        reverse mode propagates through means.py:117-159 for th_dlogp"""
        return []

    def grad(self, x, values=None):
        x = np.asarray(x)
        return self.jac(x[:, self.dims] if self.dims is not None else x, values or {})

    def eval_dx(self, x, values):
        """d m(x_i) / d x_ic over the columns the mean uses, (M, columns used): what tt.grad(location, space) gives"""
        raise NotImplementedError('%s has no derivative with respect to its inputs' % type(self).__name__)

    def dx(self, x, values=None):
        """d m(x_i) / d x_ic as an (M, d) array over ALL the columns of x: zeros in the columns the mean does not use"""
        x = np.asarray(x)
        out = np.zeros(x.shape, dtype=x.dtype)
        cols = self.dims if self.dims is not None else slice(None)
        out[:, cols] = self.eval_dx(x[:, cols], values or {})
        return out

Location = Mean


class Zero(Mean):
    BROADCASTS = JAC_CONSTANT = True

    def eval(self, x, values):
        return np.zeros(x.shape[0], dtype=x.dtype)

    def eval_dx(self, x, values):
        return np.zeros(x.shape, dtype=x.dtype)


class Bias(Mean):
    BROADCASTS = JAC_CONSTANT = True
    SLOTS = (Slot('bias', False, '_Bias'),)

    def default_hypers(self, x=None, y=None):
        return {self.bias: y.mean()}

    def eval(self, x, values):
        return _param(self.bias, values, x.dtype.type) * np.ones(x.shape[0], dtype=x.dtype)

    def jac(self, x, values):
        return [(self.bias, np.ones((x.shape[0], 1), dtype=x.dtype))]

    def eval_dx(self, x, values):
        return np.zeros(x.shape, dtype=x.dtype)


class Linear(Mean):
    BROADCASTS = JAC_CONSTANT = True
    SLOTS = (Slot('constant', False, '_Constant'), Slot('coeff', False, '_Coeff', per_column=True))

    def default_hypers(self, x=None, y=None):
        return {self.constant: y.mean(), self.coeff: y.mean() / x.mean(axis=0)}

    def eval(self, x, values):
        t = x.dtype.type
        coeff = _param(self.coeff, values, t)
        coeff = np.broadcast_to(coeff, coeff.shape[:-1] + (x.shape[1],))
        # one matrix-vector product per row of coeff, stacked or not: the same routine, so the same bytes, either way
        return _param(self.constant, values, t) + np.matmul(x, coeff[..., :, None])[..., 0]

    def jac(self, x, values):
        return [(self.constant, np.ones((x.shape[0], 1), dtype=x.dtype)), (self.coeff, x)]

    def eval_dx(self, x, values):
        coeff = np.asarray(_param(self.coeff, values, x.dtype.type)).reshape(-1)
        return np.broadcast_to(np.broadcast_to(coeff, (x.shape[1],)), x.shape)
