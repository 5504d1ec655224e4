"""GaussianProcess / WarpedGaussianProcess (g3py/processes/gaussian.py:18-260) on the HIP path."""
from types import SimpleNamespace

import numpy as np
from scipy import stats

from .. import _lib
from ..device import compile_spec_rows
from ..libs.tensors import to_num
from .elliptical import EllipticalProcess, SENTINEL


def _logp_diag(delta, sd, det_m, dtype):
    """log density of independent normal marginals with a DIAGONAL factor `sd` at latent residuals `delta`, plus the
    warp's log-Jacobian `det_m` (WarpedGaussianDistribution.logp_cho, gaussian.py:42-54, 192-241): the sum over the last
    axis, so (N,) arguments give a scalar and the (B, N) rows of a chain block (B,).  A row with a non-finite delta,
    det_m, sd or delta / sd takes the constant -1e30 (gaussian.py:234-241)."""
    t = np.dtype(dtype).type
    with np.errstate(all='ignore'):
        lcho = delta / sd
        r = (t(-0.5) * t(sd.shape[-1]) * np.log(t(2.0 * np.pi)) + t(-0.5) * (lcho * lcho).sum(axis=-1)
             - np.log(sd).sum(axis=-1) + det_m)
    bad = ~(np.isfinite(delta).all(axis=-1) & np.isfinite(det_m) & np.isfinite(sd).all(axis=-1) & np.isfinite(lcho).all(axis=-1))
    return np.where(bad, t(SENTINEL), r).astype(dtype)[()]


def logp_cho_diag(value, mu, sd, mapping, values, dtype):
    """_logp_diag of the observations `value` under independent latent N(mu, sd^2) marginals: O(M) host arithmetic on
    device-produced vectors"""
    value = np.asarray(value, dtype=dtype)
    with np.errstate(all='ignore'):
        delta = np.asarray(mapping.inv(value, values)) - mu
        det_m = mapping.logdet_dinv(value, values)
    return _logp_diag(delta, np.asarray(sd), det_m, dtype)


def gauss_hermite(f, mu, sigma, n, dtype):
    """E f(N(mu, sigma^2)) by n-point Gauss-Hermite quadrature (gaussian.py:162-174)"""
    t = np.dtype(dtype).type
    _a, _w = np.polynomial.hermite.hermgauss(n)
    a = _a.astype(dtype)[:, None]
    w = _w.astype(dtype)
    grille = mu + sigma * t(np.sqrt(2)) * a
    return np.dot(w, f(grille.flatten()).reshape(grille.shape)) / t(np.sqrt(np.pi))


def loo_assemble(alpha, kdiag, z, mapping, values, y=None, dtype=np.float64, hermite=None, mean=True, std=True, var=False,
                 median=False, logpred=True):
    """The O(N) host side of leave-one-out: from alpha = K^-1 (z - m(X)) and kdiag = diag K^-1 of the factored, noisy K,
    observation i predicted from all the others is latent-normal with
        loc_i = z_i - alpha_i / kdiag_i        sd_i = 1 / sqrt(kdiag_i)
    (z = T^-1(y), scrubbed by the caller where it must be).  Returns a DictObj under predict's keys -- mean, variance, std,
    median through the mapping (hermite=None: a plain process, mapping(loc) and sd^2 as elliptical.py:190-200; hermite=n:
    the warped process's n-point Gauss-Hermite moments, gaussian.py:127-157) -- plus `logpredictive` =
    logp_cho_diag(y, loc, sd, ...), the summed log density of every y_i under its own leave-one-out predictive.
    Two-dimensional alpha / kdiag / z (rows of a chain, `values` from _values_rows): only `logpredictive`, one per row --
    logp_cho_diag's _logp_diag over the rows, with z = mapping.inv_rows(y) as the caller has it (NOT scrubbed: a row with
    a non-finite entry takes the sentinel) and the mapping's logdet_dinv_rows; the curve switches and `hermite` play no
    part there.  No device, no process: a pure function of its arguments."""
    from ..libs import DictObj
    t = np.dtype(dtype).type
    alpha, kdiag, z = (np.asarray(v, dtype=dtype) for v in (alpha, kdiag, z))
    with np.errstate(all='ignore'):
        loc = z - alpha / kdiag
        sd = t(1) / np.sqrt(kdiag)
    out = DictObj()
    if alpha.ndim == 2:
        det_m = np.asarray(mapping.logdet_dinv_rows(np.asarray(y, dtype=dtype), values, len(alpha)), dtype=dtype)
        with np.errstate(all='ignore'):
            out['logpredictive'] = _logp_diag(z - loc, sd, det_m, dtype)
        return out
    with np.errstate(all='ignore'):
        if hermite is None:
            m, v = (mapping(loc, values), sd * sd) if (mean or std or var) else (None, None)
        else:
            m = gauss_hermite(lambda u: mapping(u, values), loc, sd, hermite, dtype) if (mean or std or var) else None
            v = gauss_hermite(lambda u: mapping(u, values) ** 2, loc, sd, hermite, dtype) - m ** 2 if (std or var) else None
        if mean:
            out['mean'] = m
        if var:
            out['variance'] = v
        if std:
            out['std'] = np.sqrt(v)
        if median:
            out['median'] = mapping(loc, values)
    if logpred:
        out['logpredictive'] = logp_cho_diag(y, loc, sd, mapping, values, dtype)
    return out


def parse_folds(folds, N):
    """The folds of `cv` as a list of int64 index arrays into the N observations, from
        an int k                    np.array_split(np.arange(N), k): contiguous blocks
        a length-N integer array    labels; observations that share a label >= 0 form a fold (in the order of the labels),
                                    a negative label is in no fold
        a sequence of index arrays  as given
    Anything else, and the first offence of a sequence -- an index outside [0, N), an index in two places, more than 4096
    folds -- is a ValueError.  No device: a pure function."""
    if isinstance(folds, (int, np.integer)) and not isinstance(folds, (bool, np.bool_)):
        if folds < 1:
            raise ValueError('cv needs at least one fold, got %d' % folds)
        if folds > _lib.G3_MAX_BATCH:
            raise ValueError('more than %d folds (%d)' % (_lib.G3_MAX_BATCH, folds))
        return [a.astype(np.int64) for a in np.array_split(np.arange(N), int(folds))]
    if isinstance(folds, (str, bytes, dict)) or not hasattr(folds, '__len__'):
        raise ValueError('folds: an int, a length-N array of integer labels or a sequence of index arrays, not %r' % type(folds).__name__)
    flat = None
    try:
        flat = np.asarray(folds)
    except ValueError:          # ragged: a sequence of index arrays
        pass
    if flat is not None and flat.ndim == 1 and flat.dtype != object and len(flat) > 0:
        if not np.issubdtype(flat.dtype, np.integer):
            raise ValueError('fold labels must be integers, not %s' % flat.dtype)
        if len(flat) != N:
            raise ValueError('%d fold labels for %d observations' % (len(flat), N))
        labels = np.unique(flat[flat >= 0])
        if len(labels) > _lib.G3_MAX_BATCH:
            raise ValueError('more than %d folds (%d)' % (_lib.G3_MAX_BATCH, len(labels)))
        return [np.flatnonzero(flat == u).astype(np.int64) for u in labels]
    if len(folds) == 0:
        raise ValueError('cv needs at least one fold')
    if len(folds) > _lib.G3_MAX_BATCH:
        raise ValueError('more than %d folds (%d)' % (_lib.G3_MAX_BATCH, len(folds)))
    out, seen = [], np.zeros(N, dtype=bool)
    for f, one in enumerate(folds):
        a = np.asarray(one)
        if a.ndim != 1 or (len(a) and not np.issubdtype(a.dtype, np.integer)):
            raise ValueError('fold %d is not a one-dimensional array of integer indices' % f)
        a = a.astype(np.int64)
        for i in a:
            if i < 0 or i >= N:
                raise ValueError('fold %d: index %d is out of range for %d observations' % (f, i, N))
            if seen[i]:
                raise ValueError('fold %d: index %d is in two folds (overlap)' % (f, i))
            seen[i] = True
        out.append(a)
    return out


def cv_assemble(resid, pvar, fold, info, folds, z, mapping, values, y, dtype=np.float64, hermite=None, mean=True, std=True,
                var=False, median=False, logpred=True):
    """The O(N) host side of leave-fold-out cross-validation, from what g3_gp_cv returns: resid_i = [A_II^-1 alpha_I]_i and
    pvar_i = [A_II^-1]_ii for the fold I that holds i, so that observation i given everything outside its fold is latent-normal
    with loc_i = z_i - resid_i and variance pvar_i -- loo_assemble's formulas at alpha' = resid / pvar, kdiag' = 1 / pvar -- and
    per fold (log det A_II, alpha_I^T A_II^-1 alpha_I).  Returns a DictObj under loo's keys: the curves have length N with NaN at
    observations in no fold; `logpredictive` sums the held-out points' marginal log densities; `logpredictive_joint` sums over
    the folds log p(y_I | rest) = -1/2 quad + 1/2 logdet - |I| / 2 log 2 pi plus the warp's logdet_dinv of the held-out y.  A fold
    with a non-zero pivot flag sends both scores to the -1e30 sentinel.  `folds` and `info` are handed through.  No device, no
    process: a pure function of its arguments."""
    t = np.dtype(dtype).type
    N = len(z)
    held = np.concatenate([np.asarray(f, dtype=np.int64) for f in folds]) if len(folds) else np.zeros(0, dtype=np.int64)
    resid, pvar, z, y = (np.asarray(v, dtype=dtype) for v in (resid, pvar, z, y))
    with np.errstate(all='ignore'):
        part = loo_assemble(resid[held] / pvar[held], t(1) / pvar[held], z[held], mapping, values, y=y[held], dtype=dtype,
                            hermite=hermite, mean=mean, std=std, var=var, median=median, logpred=logpred)
    from ..libs import DictObj
    out = DictObj()
    for k in ('mean', 'variance', 'std', 'median'):
        if k in part:
            out[k] = np.full(N, np.nan, dtype=dtype)
            out[k][held] = part[k]
    if logpred:
        bad = bool(np.any(np.asarray(info) != 0))
        out['logpredictive'] = t(SENTINEL) if bad else part['logpredictive']
        fold = np.asarray(fold, dtype=np.float64).reshape(-1, 2)
        with np.errstate(all='ignore'):
            det_m = mapping.logdet_dinv(y[held], values) if len(held) else 0.0
            joint = (-0.5 * fold[:, 1] + 0.5 * fold[:, 0]).sum() - 0.5 * len(held) * np.log(2.0 * np.pi) + det_m
        out['logpredictive_joint'] = t(SENTINEL) if bad or not np.isfinite(joint) else t(joint)
    out['folds'] = list(folds)
    out['info'] = np.asarray(info)
    return out


class _Ref:
    """placeholder a kernel's spec() carries where a free hyper-parameter's value would go"""

    def __init__(self, name):
        self.name = name


class _Refs(dict):
    def __getitem__(self, name):
        return _Ref(name)


class _ScoreChain:
    """The block loop of logp_chain, dlogp_chain, loo_chain and dloo_chain: `with _ScoreChain(...) as sc: for blk in sc:`.
    X is uploaded once, the chain workspace sc.ws holds sc.batch members (None: what fits in 4 GB -- three matrices per
    member with the K^-1 workspaces of `grad`, else one); every block is factored in ONE batched sweep before the caller
    gets it, with blk.ok the rows that do NOT take the constant -1e30 branch (gaussian.py:234-237; st[:, 2] counts the
    factor's non-finite entries).  Leaving the `with`, whether the loop ended or raised, frees X and what sc.alloc gave."""

    def __init__(self, proc, chain, batch, grad=False):
        self.proc, self.chain = proc, chain
        self.X, self.y, self.N, self.d, self.Np, self.kstride, self.batch, self.Xd, self.ws = proc._chain_setup(
            len(chain), batch, lambda Np, kstride: int(4e9 // ((3 if grad else 1) * kstride * proc.dtype.itemsize)), grad=grad)
        self.factor = (self.Xd, self.N, self.d, self.ws['K'], self.kstride, self.ws['W'], self.ws['a'])    # as the device takes it
        self._bufs = [self.Xd]

    def alloc(self, rows, cols):
        self._bufs.append(self.proc.device.alloc(rows, cols, self.proc.dtype))
        return self._bufs[-1]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for buf in self._bufs:      # not left to the garbage collector: a sampler evaluates chain after chain
            buf.free()

    def __iter__(self):
        p, n_rows = self.proc, len(self.chain)
        for lo in range(0, n_rows, self.batch):
            hi = min(lo + self.batch, n_rows)
            B = hi - lo
            # the whole block at once on the host: values, programs (one template + the hyper values that differ per
            # row), warped observations and the mean -- O(B) NumPy passes, no per-row Python
            values, logjac = p._values_rows(self.chain[lo:hi])
            members = p._chain_members(p.f_kernel_noise, values, self.d, B)
            delta, det_m, bad = p._chain_delta_or_bad(values, self.X, self.y, B)
            st = p._chain_factor_block(members, delta, *self.factor)
            yield SimpleNamespace(lo=lo, hi=hi, B=B, values=values, logjac=logjac, members=members, delta=delta, det_m=det_m,
                                  bad=bad, st=st, ok=~bad & np.isfinite(st[:, 0]) & (st[:, 2] == 0))


class FactorLikelihood:
    """What every elliptical process with a density of the Cholesky factor's two scalars shares -- logp, its gradient and
    their forms over the rows of a chain: mixed into GaussianProcess and StudentTProcess, which supply `_density` and
    `_dlogp_scale`.  Each host formula below is written once, for a scalar / (N,) vector of one hyper-parameter vector or
    the (B,) / (B, N) arrays of a chain block alike (reductions over the last axis); only the device calls differ."""

    def _nu(self, values, B=None):
        """degrees of freedom of the density for one row of values, or (B,) for a chain block (None: it has none)"""
        if self.f_degree is None:
            return None
        return self.f_degree(values) if B is None else self.f_degree.rows(values, B)

    def _density(self, logdet, quad, det_m, N, nu):
        """the observed log-density from the factor's scalars -- logdet = sum log L_ii, quad = |L^-1 delta|^2 -- and the
        warp's log-Jacobian, as scalars or (B,) arrays, evaluated in the process dtype"""
        raise NotImplementedError

    def _dlogp_scale(self, nu, quad, N, nat, ok=None):
        """s in d logp / d quad = -s / 2, as a scalar or (B,) like its arguments (None: s = 1, the Gaussian density); a
        density with hypers of its own adds their gradient terms to `nat` here (rows with ok False: none)"""
        return None

    # ---- log marginal likelihood (gaussian.py:192-249, studentT.py:114-146; stochastic.py:300-313)
    def th_loglike(self, space, inputs, outputs, vector, params, prior=False, noise=False):
        values, _ = self._values(params)
        t = self.dtype.type
        c = self._factor(values, inputs, outputs)
        if not np.all(np.isfinite(c['delta'])):                     # cond1, gaussian.py:234
            return t(SENTINEL)
        if not np.all(np.isfinite(c['det_m'])):                     # cond2, :235
            return t(SENTINEL)
        st = self._solve(c, values, 'logp')
        # cond3 (:236): a factor from a scrubbed covariance (or the 1e-10*I fallback) is finite
        if not np.isfinite(st['logdet']) or st['nonfinite'] > 0:    # cond4, :237
            return t(SENTINEL)
        with np.errstate(all='ignore'):
            return t(self._density(st['logdet'], st['quad'], c['det_m'], c['N'], self._nu(values)))

    # ---- gradient of logp (stochastic.py:308-309; tensors.py:11-22, 224-260)
    def th_dlogp(self, space, inputs, outputs, vector, params, prior=False, noise=False):
        """tt_to_num(gradient(th_logp, free variables)): flat vector over the model's variables in
        creation order, in TRANSFORMED space (d/d log h = h * d/dh for the FlatExp hypers).
        The reference differentiates the Theano graph; the same chain rule in closed form is
            d loglike = 1/2 sum_ij (alpha alpha^T - K^-1)_ij dK_ij  +  alpha . dm  -  alpha . dT^-1(y)  +  d logdet
        with K the (possibly jittered) matrix that was factored -- CholeskyRobust.grad re-uses the
        jittered factor the same way -- and zero when logp takes its constant -1e30 branch.
        K^-1 and the kernel-parameter sums are computed on the device (g3_gp_dlogp)."""
        values, _ = self._values(params)
        nat = self._potential_gradient(values)
        if not prior:
            ll = self.th_loglike(space, inputs, outputs, vector, params)
            if np.isfinite(ll) and ll != self.dtype.type(SENTINEL):
                self._dloglike(values, inputs, outputs, nat)
        return self._flat_gradient(values, nat)

    def _dloglike(self, values, inputs, outputs, nat):
        """adds d loglike / d (natural-space hyper) into `nat`"""
        dev = self.device
        c = self._factor(values, inputs, outputs)
        ds = self._dist
        if ds is not None and not ds.get('grad'):
            # several GPUs: from the first gradient on, every evaluation of this process carries the identity as
            # right-hand-side rows (the rank's rows of L^-T, g3_dist_set_grad); an evaluation cached without them is redone
            ds['grad'] = True
            if ds['dgp'] is not None:
                ds['dgp'].set_grad(True)
            c['which'] = None
        st = self._solve(c, values, 'logp')
        N, d, Np = c['N'], c['d'], c['Np']
        # d logp / d beta = -s / 2 with beta = |L^-1 delta|^2: s = 1 for the Gaussian density; the
        # Student-t density supplies its own s (and its degrees-of-freedom term) through the hook
        s = self._dlogp_scale(self._nu(values), st['quad'], N, nat)
        s = 1.0 if s is None else float(s)
        if c.get('grad') is None and ds is not None:
            # K^-1 never exists in one place: gathered panels of L^-T, the rank's rows of K^-1, one all-reduce of the sums
            prog, gmap, slots, alpha = ds['dgp'].dlogp(self.f_kernel_noise.spec(values, d), c['Xd'], np.sqrt(s))
            c['grad'] = dict(prog=prog, gmap=gmap, slots=slots, alpha=np.sqrt(s) * alpha)
        if c.get('grad') is None:
            prog = self._prog(self.f_kernel_noise, values, d)
            gmap = dev.grad_layout(prog)
            Y, Kinv, alpha, _ = self._kinv_workspace(Np)
            ad = c['ad']
            if s != 1.0:      # G = s alpha alpha^T - K^-1: hand the device sqrt(s) a, it returns sqrt(s) alpha
                ad = dev.upload((dev.download(c['ad']) * np.sqrt(s)).astype(self.dtype))
            slots = dev.gp_dlogp(prog, gmap, c['Xd'], N, d, c['Kd'], c['Wd'], ad, Y, Kinv, alpha)
            c['grad'] = dict(prog=prog, gmap=gmap, slots=slots,
                             alpha=np.sqrt(s) * dev.download(alpha, 1, N)[0].astype(np.float64))
        g = c['grad']
        self._chain_rule(values, c['X'], c['y'], nat, g['prog'], g['gmap'], g['slots'], g['alpha'], d)

    def _zero_gradient(self, B=None):
        """a natural-space gradient of zeros: {name: v.shape} for one row of values, {name: (B, *v.shape)} for a chain block"""
        lead = () if B is None else (B,)
        return {v.name: np.zeros(lead + tuple(v.shape)) for v in self.model.vars}

    def _kinv_workspace(self, Np, kinv=True, vec=None):
        """(Y, Kinv, alpha, vec): the device buffers of dlogp, loo and dloo, kept with the factor workspace (same data set)
        and created at first need.  Y is scratch in all three and shared; kinv=False does not create Kinv and alpha; vec
        names the caller's own two-row vector ('loo': alpha, kdiag; 'dloo': kdiag, u)."""
        dev, ws = self.device, self._workspace
        if 'Y' not in ws:
            ws['Y'] = dev.alloc(Np, Np, self.dtype)
        if kinv and 'Kinv' not in ws:
            ws['Kinv'], ws['alpha'] = dev.alloc(Np, Np, self.dtype), dev.alloc(1, Np, self.dtype)
        if vec is not None and vec not in ws:
            ws[vec] = dev.alloc(2, Np, self.dtype)
        return ws['Y'], ws.get('Kinv'), ws.get('alpha'), ws.get(vec)

    def _potential_gradient(self, values, B=None):
        """the natural-space gradient every evaluation starts from: the L1 / L2 potentials' (hypers/__init__.py:97-109),
        zeros elsewhere -- {name: v.shape} for one row of values, {name: (B, *v.shape)} for a chain block"""
        nat = self._zero_gradient(B)
        for _, reg, c, sel in self.model.potentials:
            for h in sel:
                hv = np.asarray(values[h.name], dtype=np.float64)
                nat[h.name] = nat[h.name] + (-c * np.sign(hv) if reg == 'L1' else -2.0 * c * hv)
        return nat

    def _chain_rule(self, values, X, y, nat, prog, gmap, slots, alpha, d, ok=None):
        """host part of d loglike: route the device's per-leaf parameter sums (`slots`) to the model's variables and add
        the O(N) location / warping terms on alpha = s K^-1 delta.  slots (nslots,) and alpha (N,) for one row of values,
        (B, nslots) and (B, N) for a chain block; rows with ok False get no likelihood term"""
        by_name = {v.name: v for v in self.model.vars}
        lead = alpha.shape[:-1]
        if ok is not None:
            with np.errstate(all='ignore'):
                slots, alpha = np.where(ok[:, None], slots, 0.0), np.where(ok[:, None], alpha, 0.0)

        def add(name, g):            # g: lead for a scalar hyper, lead + (size,) otherwise
            nat[name] = nat[name] + (g if np.shape(g) == nat[name].shape else np.reshape(g, nat[name].shape))
        self._kernel_slots(nat, prog, gmap, slots, d)
        # location: alpha . d m / d hyper.  Over a chain block d m / d hyper is the same for every row for the means on the
        # path (linear in their hypers, JAC_CONSTANT); any other mean is asked row by row
        if not lead or getattr(self.f_location, 'JAC_CONSTANT', False):
            for h, J in self.f_location.grad(X, self._values_row(values, 0) if lead else values):
                if getattr(h, 'name', None) in by_name:
                    gj = alpha.dot(np.asarray(J, dtype=np.float64))            # lead + (size,)
                    add(h.name, gj if by_name[h.name].shape else gj.sum(axis=-1))
        else:
            for j in range(lead[0]):
                for h, J in self.f_location.grad(X, self._values_row(values, j)):
                    if getattr(h, 'name', None) in by_name:
                        gj = alpha[j].dot(np.asarray(J, dtype=np.float64))
                        nat[h.name][j] = nat[h.name][j] + (gj.reshape(by_name[h.name].shape) if by_name[h.name].shape else gj.sum())
        # warping: -alpha . d T^-1(y) / d hyper + d logdet / d hyper
        with np.errstate(all='ignore'):
            for h, dinv, dlogdet in (self.f_mapping.grad_rows(y, values, lead[0]) if lead else self.f_mapping.grad(y, values)):
                if getattr(h, 'name', None) in by_name:
                    g = -(alpha * np.asarray(dinv, dtype=np.float64)).sum(axis=-1) + np.asarray(dlogdet, dtype=np.float64)
                    add(h.name, g if ok is None else np.where(ok, g, 0.0))

    def _kernel_slots(self, nat, prog, gmap, slots, d):
        """the kernel-hyper part of the chain rule: add the device's per-leaf parameter sums -- slots (nslots,), or
        (B, nslots) for a chain block -- to the natural-space gradients of the HyperVars that fed them (the alpha slot of a
        dot leaf is its bias)"""
        from ..device import spec_leaves, LEAF_FIELDS as fields
        by_name = {v.name: v for v in self.model.vars}
        refs = spec_leaves(self.f_kernel_noise.spec(_Refs(), d))
        for l, lf in enumerate(refs):
            nd = prog.leaf[l].ndims
            for pname, idx in dict(var=1, **fields[lf[0]]).items():
                ref = lf[idx]
                if not isinstance(ref, _Ref) or ref.name not in by_name:
                    continue
                slot = getattr(gmap, pname)[l]
                if pname in ('var', 'alpha'):
                    g = slots[..., slot]
                else:
                    g = slots[..., slot:slot + nd]
                    g = g if by_name[ref.name].shape else g.sum(axis=-1)
                nat[ref.name] = nat[ref.name] + (g if np.shape(g) == nat[ref.name].shape else np.reshape(g, nat[ref.name].shape))

    def factor_vjp(self, params, Lbar, inputs=None, outputs=None):
        """Reverse mode through the factor for ANY function f of it: given Lbar = d f / d L at the Cholesky factor L of the
        observed (noisy, possibly jittered) covariance, the gradient of f with respect to the model's variables as dlogp
        returns one -- flat, in creation order, transformed space, tt_to_num'ed.  Lbar is an N x N array (its strict upper
        triangle is not read) or a callable L -> Lbar that is handed the downloaded factor.  The device pulls Lbar back to
        the covariance (g3_potrf_vjp: CholeskyRobust.grad, tensors.py:224-260) and the covariance adjoint to the kernel
        parameters (g3_gram_vjp: what tt.grad through Kernel.cov does); the jitter is a constant, as in dlogp.  Variables
        the covariance does not depend on (location, mapping, degrees of freedom) get 0: their part of f's gradient does
        not pass through L.  A `logp` on the same parameters before it is not repeated."""
        if self._dist is not None:
            raise _lib.G3Error('factor_vjp runs on one GPU')
        if inputs is None and not self.is_observed:
            raise _lib.G3Error('factor_vjp needs observations')
        params, _, inputs, outputs, _ = self._call_defaults(params, None, inputs, outputs, False, False)
        dev = self.device
        values, _ = self._values(params)
        c = self._factor(values, inputs, outputs)
        self._solve(c, values, 'logp')
        N, d = c['N'], c['d']
        if callable(Lbar):
            Lbar = Lbar(np.tril(dev.download(c['Kd'], N, N)))
        Lbar = np.asarray(Lbar, dtype=self.dtype)
        if Lbar.shape != (N, N):
            raise ValueError('Lbar of shape %s for a factor of shape %s' % (Lbar.shape, (N, N)))
        Bd, Kb = dev.upload(Lbar), dev.alloc(N, N, self.dtype)
        dev.potrf_vjp(c['Kd'], Bd, N, Kb)
        prog = self._prog(self.f_kernel_noise, values, d)
        gmap = dev.grad_layout(prog)
        slots = dev.gram_vjp(prog, gmap, c['Xd'], N, d, Kb)
        nat = self._zero_gradient()
        self._kernel_slots(nat, prog, gmap, slots, d)
        return self._flat_gradient(values, nat)

    def _flat_gradient(self, values, nat, B=None):
        """natural-space gradients -> flat vector in creation order, transformed space, tt_to_num'ed: (ndim,), or
        (B, ndim) for a chain block"""
        lead = () if B is None else (B,)
        flat = []
        for v in self.model.vars:
            g = np.asarray(nat[v.name], dtype=np.float64).reshape(lead + (-1,))
            if v.positive:
                g = g * np.asarray(values[v.name], dtype=np.float64).reshape(lead + (-1,))
            flat.append(g)
        flat = np.concatenate(flat, axis=-1) if flat else np.zeros(lead + (0,))
        return to_num(flat, np.float64).astype(self.dtype)

    def _chain_workspace(self, batch, Np, grad, pred=0):
        """device buffers of logp_chain / dlogp_chain / predict_chain, kept between calls (samplers and optimisers evaluate
        chain after chain on one data set; a GB-sized hipMalloc + hipFree per call costs more than the evaluation: 250 - 390 ms
        spikes against 7 ms).  One workspace serves all three: it only grows (more members, the two extra matrices of the
        gradient, the three `pred`-wide result vectors per member of a prediction) and is replaced when the padded size or
        the dtype changes."""
        ws = getattr(self, '_chain_ws', None)
        same = ws is not None and ws['Np'] == int(Np) and ws['dtype'] == self.dtype.str
        if same and ws['cap'] >= batch and (ws['grad'] or not grad):
            if ws['pred'] < pred:     # a wider query set: only the three result vectors grow, the matrices stay
                dev = self.device
                for k in ('mu', 'ss', 'kd'):
                    if ws[k] is not None:
                        ws['bufs'].remove(ws[k])
                        ws[k].free()
                    ws[k] = dev.alloc(ws['cap'], int(pred), self.dtype)
                    ws['bufs'].append(ws[k])
                ws['pred'] = int(pred)
            return ws
        cap, grad, pred = int(batch), bool(grad), int(pred)
        if ws is not None:
            if same:                 # grow, never shrink: logp_chain and dlogp_chain alternate inside one optimiser
                cap, grad, pred = max(cap, ws['cap']), grad or ws['grad'], max(pred, ws['pred'])
            for b in ws['bufs']:
                b.free()
        dev = self.device
        n3 = 3 if grad else 1
        mats = [dev.alloc(cap * (Np + _lib.G3_RHS_PAD), Np, self.dtype) for _ in range(n3)]
        W = dev.alloc(cap * Np, _lib.G3_PAD, self.dtype)
        vecs = [dev.alloc(cap, Np, self.dtype) for _ in range(2 if grad else 1)]
        outs = [dev.alloc(cap, pred, self.dtype) for _ in range(3)] if pred else [None] * 3
        ws = dict(Np=int(Np), dtype=self.dtype.str, cap=cap, grad=grad, pred=pred, K=mats[0], Y=mats[1] if grad else None,
                  Ki=mats[2] if grad else None, W=W, a=vecs[0], al=vecs[1] if grad else None, mu=outs[0], ss=outs[1],
                  kd=outs[2], bufs=mats + [W] + vecs + [o for o in outs if o is not None])
        self._chain_ws = ws
        return ws

    def _chain_setup(self, n_rows, batch, default_batch, inputs=None, outputs=None, grad=False, pred=0, observed=True):
        """what the block loops over a chain start from: (X, y, N, d, Np, kstride, batch, Xd, ws) with `batch` clamped to the
        rows and the library's limit (None: the caller's default_batch(Np, kstride) -- how many members fit differs per
        call), X uploaded once for the whole call and the workspace for `batch` members.  observed=False (a prior): no
        device side, Xd and ws are None."""
        X = self._x(self.inputs if inputs is None else inputs)
        y = np.asarray(self.outputs if outputs is None else outputs, dtype=self.dtype).reshape(-1)
        N, d = X.shape
        Np = _lib.roundup(N)
        kstride = (Np + _lib.G3_RHS_PAD) * Np
        if batch is None:
            batch = default_batch(Np, kstride)
        batch = max(1, min(int(batch), n_rows, _lib.G3_MAX_BATCH))
        if not observed:
            return X, y, N, d, Np, kstride, batch, None, None
        return X, y, N, d, Np, kstride, batch, self.device.upload(X), self._chain_workspace(batch, Np, grad, pred=pred)

    def _chain_members(self, kern, values_b, d, B):
        """the members of `kern` for B chain rows as (template, offsets, fields) -- one program plus the hyper values that
        differ per row (compile_spec_rows)"""
        return compile_spec_rows(kern.spec(values_b, d), kern.spec(self._values_row(values_b, 0), d), d, B)

    def _chain_delta_or_bad(self, values_b, X, y, B):
        """the logp / dlogp rows' (delta, logdet_dinv, bad): a row with a non-finite entry takes the constant -1e30 branch
        (gaussian.py:234-235); it is evaluated like the others on zeros, and its result replaced by the caller"""
        _, _, delta, det_m = self._delta(values_b, X, y, B)
        bad = ~(np.isfinite(delta).all(axis=1) & np.isfinite(det_m))
        if bad.any():
            delta = np.where(bad[:, None], self.dtype.type(0), delta)
        return delta, det_m, bad

    def _chain_factor_block(self, obs, delta, Xd, N, d, K, kstride, W, a):
        """ONE batched factorisation of a block's observation covariances (g3_gp_factor_batched_fields).  `delta` comes
        prepared by the caller, and not in one way: the logp / dlogp rows send a row with a non-finite entry as zeros and
        replace its result by the constant -1e30 branch (gaussian.py:234-237, no scrub), the predict / sample rows scrub as
        _factor / _solve('post') do for one row -- two behaviours of the reference, kept apart."""
        dev = self.device
        dd = dev.upload(np.ascontiguousarray(delta, dtype=self.dtype))
        try:
            return dev.gp_factor_batched_fields(obs[0], obs[1], obs[2], Xd, N, d, dd, K, kstride, W, a)
        finally:
            dd.free()         # a (B, N) buffer per block: not left to the garbage collector over a long chain

    def dlogp_chain(self, chain, batch=None):
        """one dlogp per row of a flat-parameter chain, shape (rows, ndim) -- what fixed_dlogp averages
        (stochastic.py:554-564: a loop of single gradients in the reference).  `batch` rows at a time
        share ONE Gram launch, ONE factorisation sweep (g3_gp_factor_batched_fields) and ONE K^-1 sweep with the
        members' alpha and kernel-parameter sums in launches that carry the member in grid.y
        (g3_gp_dlogp_batched_fields); the O(N) chain-rule pieces are array arithmetic over the rows on the host."""
        chain = np.atleast_2d(np.asarray(chain, dtype=np.float64))
        n_rows = len(chain)
        out = np.zeros((n_rows, self.active.ndim), dtype=self.dtype)
        if not self.is_observed or n_rows == 0:
            for i in range(n_rows):
                out[i] = self.dlogp(chain[i], array=True)
            return out
        dev = self.device
        with _ScoreChain(self, chain, batch, grad=True) as sc:
            N, ws, a = sc.N, sc.ws, sc.ws['a']
            for blk in sc:
                # K^-1, alpha and the kernel-parameter sums of every member in batched launches; the chain rule is array arithmetic
                B, values_b, ok = blk.B, blk.values, blk.ok
                gmap = dev.grad_layout(blk.members[0])
                nat = self._potential_gradient(values_b, B)
                s = self._dlogp_scale(self._nu(values_b, B), blk.st[:, 1], N, nat, ok)
                if s is not None:     # G = s alpha alpha^T - K^-1: the device gets sqrt(s) a and returns sqrt(s) alpha
                    with np.errstate(all='ignore'):
                        rs = np.where(ok, np.sqrt(s), 1.0)
                    dev.copy_in(a, (dev.download(a, B, sc.Np) * rs[:, None].astype(self.dtype)).astype(self.dtype))
                slots = dev.gp_dlogp_batched_fields(*blk.members, gmap, *sc.factor, ws['Y'], ws['Ki'], ws['al'])
                alphas = dev.download(ws['al'], B, N).astype(np.float64)
                if s is not None:
                    alphas = alphas * rs[:, None]
                self._chain_rule(values_b, sc.X, sc.y, nat, blk.members[0], gmap, slots, alphas, sc.d, ok)
                out[blk.lo:blk.hi] = self._flat_gradient(values_b, nat, B)
        return out

    # ---- many hyper-parameter vectors on the same observations (stochastic.py:515-520)
    def logp_chain(self, chain, prior=False, batch=None):
        """one logp per row of a flat-parameter chain.  The reference loops over the rows
        (stochastic.py:515-520; fixed_logp :526-532, "TODO: Vectorized"); here `batch` rows at a
        time go through ONE Gram launch and ONE factorisation sweep (g3_gp_factor_batched), which
        is what fills the GPU when a single N x N problem is too small to.  `batch` defaults to
        as many members as fit in 4 GB of covariance workspace."""
        chain = np.atleast_2d(np.asarray(chain, dtype=np.float64))
        n_rows = len(chain)
        t = self.dtype.type
        out = np.empty(n_rows, dtype=self.dtype)
        if prior or not self.is_observed or n_rows == 0:
            if n_rows:                      # the free variables' terms only (th_logp with prior=True): no device work
                out[:] = self._values_rows(chain)[1].astype(self.dtype)
            return out
        with _ScoreChain(self, chain, batch) as sc:
            for blk in sc:
                logjac, st = blk.logjac.astype(self.dtype), blk.st
                with np.errstate(all='ignore'):
                    dens = self._density(st[:, 0], st[:, 1], blk.det_m, sc.N, self._nu(blk.values, blk.B))
                    lp = logjac + np.asarray(dens, dtype=self.dtype)
                out[blk.lo:blk.hi] = np.where(blk.ok, lp, logjac + t(SENTINEL))
        return out


class GaussianProcess(FactorLikelihood, EllipticalProcess):
    def __init__(self, *args, **kwargs):
        if 'name' not in kwargs:
            kwargs['name'] = 'GP'
        super().__init__(*args, **kwargs)

    def _density(self, logdet, quad, det_m, N, nu=None):
        """-n/2 log 2 pi - quad / 2 - sum log L_ii + logdet_dinv (gaussian.py:208-232)"""
        t = self.dtype.type
        npi = t(-0.5) * t(N) * np.log(t(2.0 * np.pi))               # :218
        return npi + t(-0.5) * np.asarray(quad, dtype=self.dtype) - np.asarray(logdet, dtype=self.dtype) + det_m   # :219-232

    # ---- posterior prediction over a chain (models.py:489-519: a loop of single predictions in the reference)
    _CHAIN_PREDICT = True

    def _chain_predict_batched(self):
        """the batched block path serves the plain Gaussian process on one GPU: a warping needs its row form of the
        forward map and of the Gauss-Hermite moments, the Student-t process its per-row scale, a distributed process the
        multi-GPU driver -- those take the loop of single predictions"""
        from .hypers.mappings import Identity
        return bool(type(self)._CHAIN_PREDICT and self._dist is None and type(self.f_mapping) is Identity)

    def _chain_block_members(self, rows_b, kern, S, X, y, prior):
        """what one block of chain rows hands the batched entry points: the rows' values, the members of `kern` (the
        cross / prior kernel) as template + fields, the rows' location at the query points S and -- a posteriori -- the
        members of the observation kernel with the rows' delta = tt_to_num(mapping.inv(y)) - m(X) (elliptical.py:63),
        non-finite entries sent as 0, exactly as _factor / _solve('post') prepare it for one row"""
        B, d = len(rows_b), S.shape[1]
        values_b, _ = self._values_rows(rows_b)
        members = self._chain_members(kern, values_b, d, B)
        with np.errstate(all='ignore'):
            loc = np.asarray(self.f_location.rows(S, values_b, B), dtype=self.dtype)
        if prior:
            return values_b, members, loc, None, None
        obs = self._chain_members(self.f_kernel_noise, values_b, d, B)
        mapped, mu, _, _ = self._delta(values_b, X, y, B)
        with np.errstate(all='ignore'):
            delta = to_num(mapped, self.dtype) - mu
        delta = np.where(np.isfinite(delta), delta, 0).astype(self.dtype)
        return values_b, members, loc, obs, delta

    def _predict_chain_blocks(self, rows, space, inputs, outputs, switches, noise, prior, batch):
        """predict_chain for a plain Gaussian process: per block of `batch` rows ONE batched factorisation
        (g3_gp_factor_batched_fields) and ONE batched cross solve (g3_gp_cross_batched_fields: rectangular Gram with the
        member in the grid, block forward solve with the row sums fused, diag K(space) per member); the host side is array
        arithmetic over the rows, formula by formula what th_location / th_kernel_diag / quantiler do for one row."""
        from ..libs import DictObj
        dev = self.device
        t = self.dtype.type
        S = self._x(self.space if space is None else space)
        n_rows, M = len(rows), S.shape[0]
        Mp = _lib.roundup(M, _lib.G3_RHS_PAD)
        need_loc = switches['mean'] or switches['median'] or switches['quantiles']
        need_var = switches['var'] or switches['std'] or switches['quantiles']
        keys = self._predict_chain_keys(switches)
        out = DictObj((k, np.empty((n_rows, M), dtype=self.dtype)) for k in keys)

        def fit(Np, kstride):
            # per member: factor + right-hand-side block, block inverses, a, and the three result vectors; the cross-Gram
            # blocks live in the library's own workspace (at most 256 MB of it, g3_gp_cross_batched)
            per = (3 * Mp if prior else kstride + Np * _lib.G3_PAD + Np + 3 * Mp) * self.dtype.itemsize
            return int((4e9 - 2 ** 28) // per)
        Sd = dev.upload(S)
        X, y, N, d, Np, kstride, batch, Xd, ws = self._chain_setup(n_rows, batch, fit, inputs, outputs, pred=Mp, observed=not prior)
        kern_c = self.f_kernel_noise if noise else self.f_kernel         # elliptical.py:78-79
        if prior:
            Xd, K, W, a, mu, ss = Sd, None, None, None, None, None
            kd = dev.alloc(batch, Mp, self.dtype) if need_var else None
        else:
            K, W, a = ws['K'], ws['W'], ws['a']
            # the library writes the members' results roundup(M, 128) apart: views of that shape on the (wider) buffers
            mu, ss, kd = (dev.wrap(ws[k].ptr, batch, Mp, Mp, self.dtype, keep=ws[k]) for k in ('mu', 'ss', 'kd'))
        p_up, p_down = stats.norm.ppf(0.975), stats.norm.ppf(0.025)
        try:
            for lo in range(0, n_rows, batch):
                hi = min(lo + batch, n_rows)
                B = hi - lo
                _, (ctmpl, coffs, cfields), loc, obs, delta = self._chain_block_members(rows[lo:hi], kern_c, S, X, y, prior)
                if prior:
                    if need_var:
                        dev.gp_cross_batched_fields(ctmpl, coffs, cfields, Sd, M, Xd, M, d, None, 0, None, None, None, None, kd)
                else:
                    self._chain_factor_block(obs, delta, Xd, N, d, K, kstride, W, a)
                    dev.gp_cross_batched_fields(ctmpl, coffs, cfields, Sd, M, Xd, N, d, K, kstride, W, a,
                                                mu if need_loc else None, ss if need_var else None, kd if need_var else None)
                    if need_loc:
                        loc = loc + dev.download(mu, B, M)                                    # elliptical.py:81-84
                with np.errstate(all='ignore'):
                    if need_var:
                        dg = dev.download(kd, B, M)
                        if noise:   # tt_to_cov acts on the whole matrix; its effect on each row's diagonal
                            dg = to_num(dg, self.dtype)
                            m = dg.min(axis=1)
                            dg = np.where(~(m > 0)[:, None], dg + (t(np.float32(1e-6)) - m)[:, None], dg)
                        if not prior:
                            dg = dg - dev.download(ss, B, M)
                        dg = np.where(dg < 0, t(0), dg)                                       # tt_to_bounded(., 0) elliptical.py:94-97
                        sd = np.sqrt(dg)
                    for k in keys:
                        if k in ('mean', 'median'):
                            out[k][lo:hi] = loc
                        elif k == 'variance':
                            out[k][lo:hi] = dg
                        elif k == 'std':
                            out[k][lo:hi] = sd
                        else:       # quantiler: mapping(location + p * kernel_sd), th_mapping scrubs its result
                            r = loc + (p_up if k == 'quantile_up' else p_down) * sd
                            out[k][lo:hi] = to_num(r, self.dtype)
        finally:
            Sd.free()
            if Xd is not Sd:
                Xd.free()
            if prior and kd is not None:
                kd.free()
        return out

    def _sample_chain_blocks(self, rows, space, inputs, outputs, rand, noise, prior, batch):
        """sample_chain for a plain Gaussian process: per block of `batch` rows ONE batched factorisation and ONE
        g3_gp_draws_batched_fields (cross solve that keeps V, posterior covariances through the batched MFMA product, the
        jitter schedule per member on the device, the draws with the member in the grid); the host side is the rows'
        location and the mapping's scrub, as th_location / th_mapping do for one row.  Returns (draws (rows, M, samples),
        tries, fallback, jitter per row)."""
        dev = self.device
        S = self._x(self.space if space is None else space)
        n_rows, M = len(rows), S.shape[0]
        samples = rand.shape[2]
        out = np.empty((n_rows, M, samples), dtype=self.dtype)
        tries, fallback, jitter = np.zeros(n_rows, dtype=np.int32), np.zeros(n_rows, dtype=bool), np.zeros(n_rows)
        kern = self.f_kernel_noise if noise else self.f_kernel           # elliptical.py:70,74,78-79
        Sd = dev.upload(S)
        Xd = None
        if prior:
            X = y = None
            N, d, K, W, a, kstride = 0, S.shape[1], None, None, None, 0
            batch = max(1, min(int(batch or _lib.G3_MAX_BATCH), n_rows, _lib.G3_MAX_BATCH))
        else:
            # per member: factor + right-hand-side block, block inverses, a (V, C and Lp live in the library)
            X, y, N, d, Np, kstride, batch, Xd, ws = self._chain_setup(
                n_rows, batch, lambda Np, kstride: int((4e9 - 2 ** 28) // ((kstride + Np * _lib.G3_PAD + Np) * self.dtype.itemsize)),
                inputs, outputs)
            K, W, a = ws['K'], ws['W'], ws['a']
        try:
            for lo in range(0, n_rows, batch):
                hi = min(lo + batch, n_rows)
                _, (tmpl, offs, fields), loc, obs, delta = self._chain_block_members(rows[lo:hi], kern, S, X, y, prior)
                if not prior:
                    self._chain_factor_block(obs, delta, Xd, N, d, K, kstride, W, a)
                g, tries[lo:hi], fallback[lo:hi], jitter[lo:hi] = dev.gp_draws_batched_fields(
                    tmpl, offs, fields, Sd, M, Xd, N, d, K, kstride, W, a, noise, loc, rand[lo:hi])
                with np.errstate(all='ignore'):
                    out[lo:hi] = to_num(g, self.dtype)     # th_mapping scrubs its result
        finally:
            Sd.free()
            if Xd is not None:
                Xd.free()
        return out, tries, fallback, jitter

    def th_logpredictive(self, space, inputs, outputs, vector, params, prior=False, noise=False):
        loc, sd, values = self._loc_sd(space, inputs, outputs, params, prior, noise, sd_noise=True)
        return logp_cho_diag(vector, loc, sd, self.f_mapping, values, self.dtype)

    # ---- leave-one-out cross-validation from the factor (no counterpart in the reference: its scores / Experiment
    #      harness, models.py:449-469, refits per hold-out split)
    _LOO_HERMITE = None          # mean / variance of a plain process: mapping(loc) and sd^2 (elliptical.py:190-200)

    def _loo_guard(self, inputs=None, what='loo'):
        if self._dist is not None:
            raise _lib.G3Error(what + ' runs on one GPU')
        if inputs is None and not self.is_observed:
            raise _lib.G3Error(what + ' needs observations')

    def loo(self, params=None, inputs=None, outputs=None, mean=True, std=True, var=False, median=False, logpred=True):
        """Every observation predicted from all the others, from the Cholesky factor `logp` already paid for: a DictObj
        under predict's keys (mean, variance, std, median: length N) plus `logpredictive`, the sum over i of
        logpredictive(vector=[y_i], space=[x_i]) after observing everything but i.  With alpha = K^-1 delta and
        c_i = [K^-1]_ii of the factored (possibly jittered) noisy covariance the latent predictive of y_i is
        N(z_i - alpha_i / c_i, 1 / c_i); the device forms L^-T and both vectors (g3_gp_loo: N^3 / 3 flops, half of
        dlogp's K^-1), the host the O(N) rest (loo_assemble).  A `logp` on the same parameters before it is not repeated.
        Where th_loglike takes its constant branch, logpredictive is the -1e30 sentinel and the curves come from the
        scrubbed observations, as predict's do."""
        self._loo_guard(inputs)
        params, _, inputs, outputs, _ = self._call_defaults(params, None, inputs, outputs, False, False)
        dev = self.device
        values, _ = self._values(params)
        c = self._factor(values, inputs, outputs)
        const = not (np.all(np.isfinite(c['delta'])) and np.all(np.isfinite(c['det_m'])))     # gaussian.py:234-235
        st = self._solve(c, values, 'post' if const else 'logp')
        if c.get('loo') is None:
            N, Np = c['N'], c['Np']
            Y, _, _, vec = self._kinv_workspace(Np, kinv=False, vec='loo')      # (dlogp's Y: scratch in both)
            dev.gp_loo(N, c['Kd'], c['Wd'], c['ad'], Y, vec, dev.wrap(vec.offset(1), 1, Np, Np, self.dtype, keep=vec))
            c['loo'] = dev.download(vec, 2, N)
        alpha, kdiag = c['loo']
        out = loo_assemble(alpha, kdiag, c['z'], self.f_mapping, values, y=c['y'], dtype=self.dtype,
                           hermite=self._LOO_HERMITE, mean=mean, std=std, var=var, median=median, logpred=logpred)
        if logpred and (const or not np.isfinite(st['logdet']) or st['nonfinite'] > 0):           # gaussian.py:234-237
            out['logpredictive'] = self.dtype.type(SENTINEL)
        return out

    def cv(self, params=None, folds=5, inputs=None, outputs=None, mean=True, std=True, var=False, median=False, logpred=True):
        """Blocked / k-fold cross-validation from the Cholesky factor `logp` already paid for: every fold predicted from all
        the observations outside it, without a refit.  `folds`: an int k (k contiguous blocks, the blocked-CV default), a
        length-N array of integer labels (negative: in no fold) or a sequence of index arrays (parse_folds).  Returns a DictObj
        under loo's keys -- mean, variance, std, median of length N: each observation's marginal predictive given everything
        outside its fold, NaN in no fold; `logpredictive`, the sum of the held-out points' marginal log densities (what loo and
        th_logpredictive report) -- plus `logpredictive_joint`, the sum over folds of log p(y_I | rest), `folds`, the index
        arrays used, and `info`, the folds' pivot flags.  With A = K^-1 of the factored covariance and alpha = A delta the fold's
        latent predictive is N(z_I - A_II^-1 alpha_I, A_II^-1): the device forms K^-1 and factors every A_II in batched
        launches (g3_gp_cv: 2 N^3 / 3 + 2 sum_f s_f^3 / 3 flops), the host the O(N) rest (cv_assemble).  F = N folds of one point
        is loo; one fold of everything is the prior, its joint score loglike.  A `logp` on the same parameters before it is
        not repeated, and the result is kept per (factorisation, folds).  Where th_loglike takes its constant branch, and
        where a fold's factorisation reports a pivot, both scores are the -1e30 sentinel."""
        self._loo_guard(inputs, 'cv')
        params, _, inputs, outputs, _ = self._call_defaults(params, None, inputs, outputs, False, False)
        dev = self.device
        values, _ = self._values(params)
        c = self._factor(values, inputs, outputs)
        N, Np = c['N'], c['Np']
        fl = parse_folds(folds, N)
        idx = np.concatenate(fl).astype(np.int32) if fl else np.zeros(0, dtype=np.int32)
        ptr = np.concatenate([[0], np.cumsum([len(f) for f in fl])]).astype(np.int64)
        key = (idx.tobytes(), ptr.tobytes())
        const = not (np.all(np.isfinite(c['delta'])) and np.all(np.isfinite(c['det_m'])))     # gaussian.py:234-235
        st = self._solve(c, values, 'post' if const else 'logp')
        got = c.get('cv')
        if got is None or got['stats'] is not st or got['key'] != key:       # (kept with the factorisation it belongs to)
            Y, Kinv, alpha, vec = self._kinv_workspace(Np, vec='cv')        # (Y, Kinv and alpha: dlogp's, scratch in both)
            fold, info = dev.gp_cv(N, c['Kd'], c['Wd'], c['ad'], Y, Kinv, alpha, idx, ptr, vec,
                                   dev.wrap(vec.offset(1), 1, Np, Np, self.dtype, keep=vec))
            rv = dev.download(vec, 2, N)
            got = c['cv'] = dict(stats=st, key=key, resid=rv[0], pvar=rv[1], fold=fold, info=info)
        out = cv_assemble(got['resid'], got['pvar'], got['fold'], got['info'], fl, c['z'], self.f_mapping, values, c['y'],
                          dtype=self.dtype, hermite=self._LOO_HERMITE, mean=mean, std=std, var=var, median=median, logpred=logpred)
        if logpred and (const or not np.isfinite(st['logdet']) or st['nonfinite'] > 0):           # gaussian.py:234-237
            out['logpredictive'] = out['logpredictive_joint'] = self.dtype.type(SENTINEL)
        return out

    def loo_chain(self, chain, batch=None):
        """loo(...).logpredictive for every row of a flat-parameter chain, shape (rows,): a model-comparison score over a
        whole trace.  The block structure is logp_chain's -- `batch` rows share ONE Gram launch and ONE factorisation
        sweep -- followed by ONE g3_gp_loo_batched (N <= 256: one workgroup per member) and one download of the members'
        alpha and kdiag; the rest is array arithmetic over the rows (loo_assemble), which is what the call spends most of
        its time in at small N (profiles/loo.md).  Rows
        that logp_chain sends to its -1e30 sentinel get the sentinel.  A predictive score, not a posterior density: no
        prior and no Jacobian-of-transform terms."""
        self._loo_guard()
        chain = np.atleast_2d(np.asarray(chain, dtype=np.float64))
        n_rows = len(chain)
        t = self.dtype.type
        out = np.empty(n_rows, dtype=self.dtype)
        if n_rows == 0:
            return out
        dev = self.device
        with _ScoreChain(self, chain, batch) as sc:
            y, N, Np, ws = sc.y, sc.N, sc.Np, sc.ws
            vec = sc.alloc(2 * sc.batch, Np)                     # a block's alpha rows, then its kdiag rows: one download
            Y = sc.alloc(Np, Np) if Np > 2 * _lib.G3_PAD else None
            for blk in sc:
                B, values_b = blk.B, blk.values
                kd = dev.wrap(vec.offset(B), B, Np, Np, self.dtype, keep=vec)
                dev.gp_loo_batched(B, N, ws['K'], sc.kstride, ws['W'], ws['a'], Y, vec, kd)
                both = dev.download(dev.wrap(vec.ptr, 2 * B, Np, Np, self.dtype, keep=vec), 2 * B, N)
                with np.errstate(all='ignore'):
                    z = np.asarray(self.f_mapping.inv_rows(y, values_b, B), dtype=self.dtype)
                lp = loo_assemble(both[:B], both[B:], z, self.f_mapping, values_b, y=y, dtype=self.dtype)['logpredictive']
                out[blk.lo:blk.hi] = np.where(blk.ok, lp, t(SENTINEL))
        return out

    def dloo(self, params=None, inputs=None, outputs=None):
        """Gradient of loo(...).logpredictive with respect to the model's variables, as dlogp returns one: flat, in creation
        order, transformed space, tt_to_num'ed.  A predictive score: no prior, Jacobian or potential terms.  With A = K^-1 of
        the factored (possibly jittered, the jitter a constant) noisy covariance, alpha = A delta and c = diag A,
            d F = sum_ij W_ij dK_ij + u . dm - u . dT^-1(y) + d logdet,
            W = -A diag(q) A + 1/2 (u alpha^T + alpha u^T),  q = 1/2 (1 / c + alpha^2 / c^2),  u = A (alpha / c);
        the device forms K^-1, the weight and the kernel-parameter sums (g3_gp_dloo: about 1 2/3 N^3 flops), the host the O(N)
        location and warping terms -- dlogp's chain rule with u in the place of alpha.  Zeros where loo returns its -1e30
        sentinel.  A `logp` on the same parameters before it is not repeated; the K^-1 workspaces are dlogp's."""
        self._loo_guard(inputs)
        params, _, inputs, outputs, _ = self._call_defaults(params, None, inputs, outputs, False, False)
        dev = self.device
        values, _ = self._values(params)
        nat = self._zero_gradient()
        c = self._factor(values, inputs, outputs)
        if not (np.all(np.isfinite(c['delta'])) and np.all(np.isfinite(c['det_m']))):          # gaussian.py:234-235
            return self._flat_gradient(values, nat)
        st = self._solve(c, values, 'logp')
        if not np.isfinite(st['logdet']) or st['nonfinite'] > 0:                                # gaussian.py:237
            return self._flat_gradient(values, nat)
        N, d, Np = c['N'], c['d'], c['Np']
        g = c.get('dloo')
        if g is None or g['stats'] is not st:        # (kept with the factorisation it belongs to)
            prog = self._prog(self.f_kernel_noise, values, d)
            gmap = dev.grad_layout(prog)
            Y, Kinv, alpha, vec = self._kinv_workspace(Np, vec='dloo')       # (Y, Kinv and alpha: dlogp's, scratch in both)
            slots = dev.gp_dloo(prog, gmap, c['Xd'], N, d, c['Kd'], c['Wd'], c['ad'], Y, Kinv, alpha, vec,
                                dev.wrap(vec.offset(1), 1, Np, Np, self.dtype, keep=vec))
            g = c['dloo'] = dict(stats=st, prog=prog, gmap=gmap, slots=slots, u=dev.download(vec, 2, N)[1].astype(np.float64))
        self._chain_rule(values, c['X'], c['y'], nat, g['prog'], g['gmap'], g['slots'], g['u'], d)
        return self._flat_gradient(values, nat)

    def dloo_chain(self, chain, batch=None):
        """one dloo per row of a flat-parameter chain, shape (rows, ndim).  The block structure and the workspace are
        dlogp_chain's: `batch` rows share ONE Gram launch, ONE factorisation sweep and ONE K^-1 sweep, then the members'
        weights, products and kernel-parameter sums in launches that carry the member in the grid
        (g3_gp_dloo_batched_fields); the chain rule is array arithmetic over the rows.  Rows that loo_chain sends to its
        -1e30 sentinel get zeros."""
        self._loo_guard()
        chain = np.atleast_2d(np.asarray(chain, dtype=np.float64))
        n_rows = len(chain)
        out = np.zeros((n_rows, self.active.ndim), dtype=self.dtype)
        if n_rows == 0:
            return out
        dev = self.device
        with _ScoreChain(self, chain, batch, grad=True) as sc:
            Np, ws = sc.Np, sc.ws
            vec = sc.alloc(2 * sc.batch, Np)                     # a block's kdiag rows, then its u rows
            for blk in sc:
                B, tmpl = blk.B, blk.members[0]
                gmap = dev.grad_layout(tmpl)
                ud = dev.wrap(vec.offset(B), B, Np, Np, self.dtype, keep=vec)
                slots = dev.gp_dloo_batched_fields(*blk.members, gmap, *sc.factor, ws['Y'], ws['Ki'], ws['al'], vec, ud)
                nat = self._zero_gradient(B)
                u = dev.download(ud, B, sc.N).astype(np.float64)
                self._chain_rule(blk.values, sc.X, sc.y, nat, tmpl, gmap, slots, u, sc.d, blk.ok)
                out[blk.lo:blk.hi] = self._flat_gradient(blk.values, nat, B)
        return out

    # ---- quantiles and draws (gaussian.py:56-97)
    def quantiler(self, params=None, space=None, inputs=None, outputs=None, q=0.975, prior=False, noise=False,
                  simulations=None):
        p = stats.norm.ppf(q)
        gp_quantiler = (self.location(params, space, inputs, outputs, prior=prior, noise=noise)
                        + p * self.kernel_sd(params, space, inputs, outputs, prior=prior, noise=noise))
        return self.mapping(params, space, inputs, outputs=gp_quantiler)

    def sampler(self, params=None, space=None, inputs=None, outputs=None, samples=1, prior=False, noise=False,
                rand=None):
        """location + cholesky . randn, mapped (gaussian.py:89-97).  The M x M by M x S product
        runs in the MFMA GEMM.  `rand` (len(space) x samples) may be supplied for reproducibility;
        by default it is drawn with np.random.randn exactly as the reference does."""
        if space is None:
            space = self.space
        M = len(space)
        if rand is None:
            rand = np.random.randn(M, samples)
        rand = np.asarray(rand, dtype=self.dtype)
        loc = self.location(params, space, inputs, outputs, prior=prior, noise=noise)
        if self._dist is not None and not prior:
            # several GPUs: every rank must use the SAME normals (rank 0's are broadcast), the posterior covariance of
            # the f process is formed and factored by the driver (g3_dist_posterior_draws) from the cross solve that
            # `location` has just left in it
            if noise:
                raise _lib.G3Error('draws with the noise term are not available on a distributed process')
            ds = self._dist
            if ds['world'] > 1:
                box = [rand if ds['rank'] == 0 else None]
                ds['dist'].broadcast_object_list(box, src=0)
                rand = np.asarray(box[0], dtype=self.dtype)
            values, _ = self._values(params)
            S_ = self._x(space)
            g = ds['dgp'].draws(self.f_kernel.spec(values, S_.shape[1]), self.device.upload(S_), np.asarray(loc, dtype=np.float64), rand)
            return self.mapping(params, space, inputs, outputs=g.astype(self.dtype))
        Ld, _, _ = self._cholesky_dev(params, space, inputs, outputs, prior=prior, noise=noise)   # stays on the device
        g = self.device.gp_sample(Ld, M, loc, rand)                # loc + L Z, one call (g3_gp_sample)
        # the mapping is element-wise: one vectorised pass over the M x S draws instead of the
        # reference's per-sample loop (gaussian.py:97)
        return self.mapping(params, space, inputs, outputs=g)

    _methods = EllipticalProcess._methods + (('dlogp', 'th_dlogp'),)


class WarpedGaussianProcess(GaussianProcess):
    _CHAIN_PREDICT = False       # predict_chain takes the loop of single predictions
    _LOO_HERMITE = 10            # loo's mean / variance: the Gauss-Hermite moments of th_mean / th_variance

    def __init__(self, *args, **kwargs):
        if 'name' not in kwargs:
            kwargs['name'] = 'WGP'
        super().__init__(*args, **kwargs)

    def gauss_hermite(self, f, mu, sigma, n=10):
        """gaussian.py:162-174"""
        return gauss_hermite(f, mu, sigma, n, self.dtype)

    def th_mean(self, space, inputs, outputs, vector, params, prior=False, noise=False, n=10):
        loc, sd, values = self._loc_sd(space, inputs, outputs, params, prior, noise)
        return self.gauss_hermite(lambda v: self.f_mapping(v, values), loc, sd, n)       # gaussian.py:127-141

    def th_variance(self, space, inputs, outputs, vector, params, prior=False, noise=False, n=10):
        loc, sd, values = self._loc_sd(space, inputs, outputs, params, prior, noise)
        m = self.gauss_hermite(lambda v: self.f_mapping(v, values), loc, sd, n)
        return self.gauss_hermite(lambda v: self.f_mapping(v, values) ** 2, loc, sd, n) - m ** 2   # :143-157

    # th_covariance is undefined for the warped process (gaussian.py:159-160): not bound
    _methods = tuple(m for m in GaussianProcess._methods if m[0] != 'covariance')
