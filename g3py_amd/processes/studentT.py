"""StudentTProcess / WarpedStudentTProcess (g3py/processes/studentT.py:16-146) on the HIP path.

Same covariance, Cholesky factor and triangular solves as the Gaussian process -- one
`g3_gp_factor` gives log det and beta = |L^-1 delta|^2 -- plus the scalar Student-t pieces:
the log-density (:114-146), the posterior scaling (nu + beta - 2) / (nu + n - 2) of variances and
covariances (:36-49), t quantiles (:51-55) and inverse-gamma scaled draws (:57-67).
"""
import numpy as np
from scipy import stats
from scipy.special import gammaln, digamma

from .. import _lib
from .elliptical import EllipticalProcess
from .gaussian import FactorLikelihood, gauss_hermite
from .hypers import Freedom, HyperVar


class StudentTProcess(FactorLikelihood, EllipticalProcess):
    def __init__(self, *args, **kwargs):
        if 'name' not in kwargs:
            kwargs['name'] = 'TP'
        if kwargs.get('degree') is None:
            kwargs['degree'] = Freedom()
        super().__init__(*args, **kwargs)

    # ---- log-density (WarpedStudentTDistribution.logp_cho, studentT.py:114-146) with nu = th_freedom(prior=True) (:31)
    def _density(self, logdet, quad, det_m, N, nu):
        t = self.dtype.type
        one = np.ndim(quad) == 0
        cast = t if one else (lambda v: np.asarray(v, dtype=self.dtype))
        nu, beta, n = cast(nu), cast(quad), t(N)
        r1 = t(-0.5) * (nu + n) * np.log1p(beta / (nu - t(2)))                           # :124
        gauss = lambda: -n * t(0.5) * np.log(t(2.0 * np.float32(np.pi)))                 # :125
        student = lambda: cast(gammaln((nu + n) * 0.5) - gammaln(nu * 0.5)) - t(0.5) * n * np.log((nu - t(2)) * t(np.float32(np.pi)))
        big = t(np.float32(1e6)) <= nu
        if one:          # one row takes its side of the switch alone (np.where evaluates both: two gammaln and a select)
            r2 = gauss() if big else student()
        else:
            r2 = np.where(big, gauss(), student())
        return r1 + r2 - cast(logdet) + det_m                                            # :127-135

    # ---- gradient of logp: the Gaussian chain rule with d logp / d beta = -s/2, s = (nu + n) / (nu - 2 + beta),
    #      plus the degrees-of-freedom term (what Theano's reverse mode gives for studentT.py:114-135)
    def _dlogp_scale(self, nu, quad, N, nat, ok=None):
        n = float(N)
        if np.ndim(quad) == 0:       # one row: the same arithmetic on Python floats (a NumPy scalar costs 10x per operation)
            nu, beta = float(nu), float(quad)
        else:
            nu, beta = np.asarray(nu, dtype=np.float64), np.asarray(quad, dtype=np.float64)
        deg = self.f_degree.degree
        with np.errstate(all='ignore'):
            if isinstance(deg, HyperVar) and deg.name in nat:
                g = -0.5 * np.log1p(beta / (nu - 2.0)) + 0.5 * (nu + n) * beta / ((nu - 2.0) * (nu - 2.0 + beta))
                g = g + np.where(float(np.float32(1e6)) <= nu, 0.0,
                                 0.5 * digamma((nu + n) * 0.5) - 0.5 * digamma(nu * 0.5) - 0.5 * n / (nu - 2.0))
                nat[deg.name] = nat[deg.name] + np.reshape(g if ok is None else np.where(ok, g, 0.0), np.shape(nat[deg.name]))
            return (nu + n) / (nu - 2.0 + beta)

    # ---- posterior scaling (studentT.py:36-49)
    def th_scaling(self, space, inputs, outputs, vector, params, prior=False, noise=False):
        t = self.dtype.type
        if prior:
            return t(1.0)
        values, _ = self._values(params)
        c = self._factor(values, inputs, outputs)
        st = self._solve(c, values, 'post')              # mapping_outputs = tt_to_num(mapping.inv(outputs))
        nu = self.f_degree(values)
        return t((nu + st['quad'] - 2.0) / (nu + c['N'] - 2.0))

    def th_variance(self, space, inputs, outputs, vector, params, prior=False, noise=False):
        return (super().th_variance(space, inputs, outputs, vector, params, prior=prior, noise=noise)
                * self.th_scaling(space, inputs, outputs, vector, params, prior=prior, noise=noise))

    def th_covariance(self, space, inputs, outputs, vector, params, prior=False, noise=False):
        return (super().th_covariance(space, inputs, outputs, vector, params, prior=prior, noise=noise)
                * self.th_scaling(space, inputs, outputs, vector, params, prior=prior, noise=noise))

    # ---- quantiles and draws (studentT.py:51-67)
    def quantiler(self, params=None, space=None, inputs=None, outputs=None, q=0.975, prior=False, noise=False,
                  simulations=None):
        p = stats.t.ppf(q, df=self.freedom(params, space, inputs, outputs, prior=prior, noise=noise))
        gp_quantiler = (self.location(params, space, inputs, outputs, prior=prior, noise=noise)
                        + p * self.kernel_sd(params, space, inputs, outputs, prior=prior, noise=noise))
        return self.mapping(params, space, inputs, outputs=gp_quantiler)

    def sampler(self, params=None, space=None, inputs=None, outputs=None, samples=1, prior=False, noise=False,
                rand=None):
        """location + cholesky . (randn * invgamma), mapped (studentT.py:57-67); `rand` (len(space) x
        samples, already scaled) may be supplied for reproducibility"""
        if space is None:
            space = self.space
        M = len(space)
        if rand is None:
            free = float(self.freedom(params, space, inputs, outputs, prior=prior, noise=noise))
            rand = np.random.randn(M, samples) * stats.invgamma.rvs(a=free / 2, scale=(free - 2) / 2, size=samples)
        rand = np.asarray(rand, dtype=self.dtype)
        S = rand.shape[1]
        loc = self.location(params, space, inputs, outputs, prior=prior, noise=noise)
        Ld, _, Mp = self._cholesky_dev(params, space, inputs, outputs, prior=prior, noise=noise)   # stays on the device
        dev = self.device
        Sp = _lib.roundup(S, 64)
        Zt = dev.upload(np.ascontiguousarray(rand.T), pad_rows=Sp, pad_cols=Mp)
        out = dev.alloc(Sp, Mp, self.dtype)
        dev.gemm_nt(out, Zt, Ld, Sp, Mp, Mp)                      # (L Z)^T in the MFMA GEMM
        g = loc[:, None] + dev.download(out, S, M).T
        return np.array([self.mapping(params, space, inputs, outputs=k.T) for k in g.T]).T

    _methods = EllipticalProcess._methods + (('dlogp', 'th_dlogp'),)


class WarpedStudentTProcess(StudentTProcess):
    def __init__(self, *args, **kwargs):
        if 'name' not in kwargs:
            kwargs['name'] = 'WTP'
        super().__init__(*args, **kwargs)

    def gauss_hermite(self, f, mu, sigma, n=10):
        """studentT.py:99-102"""
        return gauss_hermite(f, mu, sigma, n, self.dtype)

    def th_mean(self, space, inputs, outputs, vector, params, prior=False, noise=False, n=10):
        loc, sd, values = self._loc_sd(space, inputs, outputs, params, prior, noise)
        return self.gauss_hermite(lambda v: self.f_mapping(v, values), loc, sd, n)       # studentT.py:79-85

    def th_variance(self, space, inputs, outputs, vector, params, prior=False, noise=False, n=10):
        loc, sd, values = self._loc_sd(space, inputs, outputs, params, prior, noise)
        m = self.gauss_hermite(lambda v: self.f_mapping(v, values), loc, sd, n)
        return self.gauss_hermite(lambda v: self.f_mapping(v, values) ** 2, loc, sd, n) - m ** 2   # :88-94

    # th_covariance is a stub in the reference (studentT.py:96-97): not bound
    _methods = tuple(m for m in StudentTProcess._methods if m[0] != 'covariance')
