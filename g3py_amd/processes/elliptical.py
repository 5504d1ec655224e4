"""EllipticalProcess: prior / posterior location, covariance, Cholesky, diagonal and sd of a
GP (g3py/processes/elliptical.py:18-217) computed by libg3hip.

The reference recompiles and recomputes Gram + an O(N^3) LU solve for EVERY requested
statistic.  Here one Cholesky factor of K(X,X)+noise is built per
(params, inputs, outputs) triple by `g3_gp_factor` and kept on the device; every posterior
statistic is a cross-Gram + multi-right-hand-side triangular solve against it
(`g3_gp_cross`).  Equal to the reference's `solve(K, .)` in exact arithmetic.
"""
import numpy as np

from .. import _lib
from ..device import Device, compile_spec
from ..libs import DictObj
from ..libs.tensors import to_num
from .hypers import HyperVar
from .hypers.kernels import Kernel, KernelSum, KernelNoise
from .hypers.means import Mean
from .hypers.mappings import Mapping, Identity
from .stochastic import StochasticProcess

SENTINEL = np.float32(-1e30)     # gaussian.py:238-241


class EllipticalProcess(StochasticProcess):
    def __init__(self, space=None, location: Mean = None, kernel: Kernel = None, mapping: Mapping = None,
                 degree=None, noisy=True, var_noise=None, *args, **kwargs):
        self.f_location = location
        self.f_degree = degree
        self.f_mapping = Identity() if mapping is None else mapping
        self.f_kernel = kernel
        if noisy:   # elliptical.py:26-31
            self.f_kernel_noise = KernelSum(self.f_kernel, KernelNoise(name='Noise', var=var_noise))
        else:
            self.f_kernel_noise = self.f_kernel
        self._cache = None
        self._workspace = None
        self._dist = None
        self.append_stats = dict(appended=0, cross_appended=0, refit=0)    # which way each observe_more went
        kwargs['space'] = space
        super().__init__(*args, **kwargs)

    @property
    def device(self):
        if self._device is None:
            self._device = Device.default()
        return self._device

    # ---------------------------------------------------------------- several GPUs
    def distribute(self, dist, rank, world, nb=None, transport='rccl'):
        """Evaluate this process on `world` GPUs, one process per GPU (SPMD: every rank runs the same program on the same
        observations and calls the same methods in the same order).  The reference has no counterpart (its only
        parallelism is a process pool over chains, stochastic.py:773-783).  From here on logp / loglike and every
        statistic that comes from the posterior location and variance at `space` -- mean, median, variance, std,
        quantiles, logpredictive -- are computed by the multi-GPU driver inside libg3hip (g3_dist_*: row-block-cyclic
        covariance, library-owned RCCL communicators); each rank holds 1 / world of the covariance and gets the same
        numbers back; `sampler` draws from the f posterior through the driver too (rank 0's normals).  `dlogp` (and so
        `find_MAP`) works too: from the first gradient on, the factorisation carries the identity as right-hand-side rows
        and K^-1 is formed row block by row block where the rows live (g3_dist_gp_dlogp).  The M x M posterior covariance
        (`covariance`, `cholesky`, `predict(cov=True)`) is formed in row chunks and gathered on every rank
        (g3_dist_posterior_cov); `cross_mean` passes its cross kernel to the driver.  `dist`: an initialised torch.distributed (any backend; it
        only carries 256 bytes of communicator ids, or everything with transport='callbacks', the one-GPU rehearsal)."""
        self._dist = dict(dist=dist, rank=int(rank), world=int(world), nb=nb, transport=transport, dgp=None, shape=None,
                          grad=False)
        self._cache = None
        self._workspace = None
        return self

    def undistribute(self):
        """back to one GPU: destroys the multi-GPU driver of this process (collective: call it on every rank)"""
        if self._dist is not None and self._dist['dgp'] is not None:
            self._dist['dgp'].close()
        self._dist = None
        self._cache = None
        self._workspace = None
        return self

    def _dist_step(self, c, values, dl, space, cross_kernel=None):
        """one evaluation on all ranks: (stats, cross-solve results or None); cross_kernel: the kernel of the cross
        covariance K(space, X) when it is not the process's own (th_cross_mean, gaussian.py:99-112)"""
        from ..distributed import NativeDistributedGP
        ds, dev = self._dist, self.device
        N, d = c['N'], c['d']
        S = None if space is None else self._x(space)
        M = 0 if S is None else S.shape[0]
        shape = (N, d, M, self.dtype.str)
        if ds['dgp'] is None or ds['shape'] != shape:
            if ds['dgp'] is not None:
                ds['dgp'].close()
            nb = ds['nb'] or (1024 if ds['world'] <= 4 and N >= 16384 else 512 if N >= 4096 else 128)
            ds['dgp'] = NativeDistributedGP(dev, ds['dist'], ds['rank'], ds['world'], N, d, M, nb=nb, dtype=self.dtype,
                                            transport=ds['transport'])
            ds['shape'] = shape
            if ds.get('grad'):
                ds['dgp'].set_grad(True)
        dgp = ds['dgp']
        dvec = self._workspace['dvec']
        dev.copy_in(dvec, np.where(np.isfinite(dl), dl, 0).astype(self.dtype))
        Sd = dev.upload(S) if M > 0 else c['Xd']
        kc = cross_kernel if cross_kernel is not None else self.f_kernel
        dgp.step(self.f_kernel_noise.spec(values, d), kc.spec(values, d), c['Xd'], Sd, dvec)
        last = dgp.last
        st = dict(logdet=last['logdet'], quad=last['quad'], nonfinite=0 if np.isfinite(last['quad']) else 1,
                  tries=last['tries'], fallback=last['fallback'], info=last['info'])
        cross = None
        if M > 0:
            Mp = _lib.roundup(M, _lib.G3_RHS_PAD)
            cross = dict(kid=(False, id(cross_kernel) if cross_kernel is not None else None), S=S.copy(),
                         out=(None, np.asarray(last['mean'], dtype=self.dtype),
                                                               np.asarray(last['ss'], dtype=self.dtype), M, Mp))
        return st, cross

    def _check_hypers(self):
        """elliptical.py:35-52"""
        x = self._inputs
        self.f_location.check_dims(x)
        self.f_kernel_noise.check_dims(x)
        self.f_mapping.check_dims(x)
        self.f_location.check_hypers(self.name + '_')
        self.f_kernel_noise.check_hypers(self.name + '_')
        self.f_mapping.check_hypers(self.name + '_')
        self.f_location.check_potential()
        self.f_kernel_noise.check_potential()
        self.f_mapping.check_potential()
        if self.f_degree is not None:                     # elliptical.py:49-52
            self.f_degree.check_dims(None)
            self.f_degree.check_hypers(self.name + '_')
            self.f_degree.check_potential()

    def default_hypers(self):
        x, y = self.inputs, self.outputs
        r = {**self.f_location.default_hypers_dims(x, y), **self.f_kernel_noise.default_hypers_dims(x, y),
             **self.f_mapping.default_hypers_dims(x, y)}
        if self.f_degree is not None:
            r.update(self.f_degree.default_hypers_dims(x, y))
        return r

    # ---------------------------------------------------------------- helpers
    def _x(self, a):
        a = np.asarray(a, dtype=self.dtype)
        return a.reshape(len(a), 1) if a.ndim < 2 else np.ascontiguousarray(a)

    def _prog(self, kernel, values, d):
        return compile_spec(kernel.spec(values, d), d)

    def _delta(self, values, X, y, B=None):
        """(mapped, mu, delta, det_m) = (T^-1(y), m(X), T^-1(y) - m(X), log det dT^-1(y)) in the process dtype
        (elliptical.py:63; gaussian.py:208, 225) for one row of hyper values -- (N,), (N,), (N,), scalar -- or, with B, for
        the B rows of a chain block: (B, N) and (B,).  Nothing is scrubbed here: logp sends a non-finite row to its -1e30
        branch, the posterior works on tt_to_num(mapped); the caller picks."""
        m, loc = self.f_mapping, self.f_location
        with np.errstate(all='ignore'):
            if B is None:
                mapped, mu, det_m = m.inv(y, values), loc(X, values), m.logdet_dinv(y, values)
            else:
                mapped, mu, det_m = m.inv_rows(y, values, B), loc.rows(X, values, B), m.logdet_dinv_rows(y, values, B)
            mapped, mu = np.asarray(mapped, dtype=self.dtype), np.asarray(mu, dtype=self.dtype)
            return mapped, mu, mapped - mu, np.asarray(det_m, dtype=self.dtype)[()]

    def _factor(self, values, inputs, outputs):
        """L = cholesky_robust(tt_to_cov(K_noise(X, X))), a = L^-1 (T^-1(y) - m(X)) on the device
        (elliptical.py:63,68,71; gaussian.py:208-212, 251-260), cached across statistics."""
        X = self._x(inputs)
        y = np.asarray(outputs, dtype=self.dtype).reshape(-1)
        key = (tuple((k, np.asarray(v).tobytes()) for k, v in sorted(values.items())), X.shape)
        c = self._cache
        if c is not None and c['key'] == key and np.array_equal(c['X'], X) and np.array_equal(c['y'], y):
            return c
        dev = self.device
        N, d = X.shape
        mapped, mu, delta, det_m = self._delta(values, X, y)
        mapped_num = to_num(mapped, self.dtype)      # tt_to_num(mapping.inv(outputs)) is what the posterior uses (elliptical.py:63)
        Np = _lib.roundup(N)
        # device workspace: re-used while the observations stay the same (optimisers and samplers call
        # logp / dlogp thousands of times on one data set -- hipMalloc and the upload of X would
        # otherwise dominate small problems)
        ws = self._workspace
        if ws is None or ws['shape'] != X.shape or not np.array_equal(ws['X'], X):
            if self._dist is not None:      # several GPUs: the covariance lives in the driver, 1 / world of it per rank
                ws = dict(shape=X.shape, X=X.copy(), Xd=dev.upload(X), Kd=None, ad=None, Wd=None, dvec=dev.alloc(1, N, self.dtype))
            else:
                ws = dict(shape=X.shape, X=X.copy(), Xd=dev.upload(X),
                          Kd=dev.alloc(Np + _lib.G3_RHS_PAD, Np, self.dtype),   # + the right-hand-side block that carries delta
                          ad=dev.alloc(1, Np, self.dtype), Wd=dev.alloc_inverses(Np, self.dtype),
                          dvec=dev.alloc(1, N, self.dtype))
            self._workspace = ws
        Xd, Kd, ad, Wd = ws['Xd'], ws['Kd'], ws['ad'], ws['Wd']
        c = dict(key=key, X=X.copy(), y=y.copy(), N=N, d=d, Np=Np, Xd=Xd, Kd=Kd, Wd=Wd, ad=ad, mu=mu, det_m=det_m,
                 delta=delta, delta_post=mapped_num - mu, z=mapped_num, stats=None, which=None)
        c['same_delta'] = bool(np.array_equal(c['delta'], c['delta_post']))
        self._cache = c
        return c

    def _solve(self, c, values, which):
        """run g3_gp_factor with delta (logp) or the scrubbed delta (posterior)"""
        if c['which'] == which or (c['which'] is not None and c['same_delta']):
            return c['stats']
        dev = self.device
        dl = c['delta'] if which == 'logp' else c['delta_post']
        finite = np.all(np.isfinite(dl))
        if self._dist is not None:
            # one multi-GPU evaluation gives the factor's scalars AND the cross solve at the process's own space
            sp = getattr(self, 'space', None)         # (a process without a space holds the reference's 2-point dummy)
            if sp is not None and self._x(sp).shape[1] != c['d']:
                sp = None
            st, cross = self._dist_step(c, values, dl, sp)
            st['delta_finite'] = bool(finite)
            c['stats'], c['which'], c['grad'], c['cross'], c['loo'], c['cv'] = st, which, None, cross, None, None
            c['dx'] = None
            return st
        dvec = self._workspace['dvec']
        dev.copy_in(dvec, np.where(np.isfinite(dl), dl, 0).astype(self.dtype))
        prog = self._prog(self.f_kernel_noise, values, c['d'])
        st = dev.gp_factor(prog, c['Xd'], c['N'], c['d'], dvec, c['Kd'], c['Wd'], c['ad'])
        st['delta_finite'] = bool(finite)
        c['stats'], c['which'] = st, which
        c['grad'] = None            # K^-1 / alpha pieces of th_dlogp belong to this factorisation
        c['cross'] = None           # so does the last cross solve
        c['loo'] = None             # and the leave-one-out vectors
        c['dx'] = None              # and predict_dx's L^-T and alpha
        c['cv'] = None              # and the leave-fold-out ones
        return st

    # ---------------------------------------------------------------- new observations without a refit
    _NP_SCRATCH = ('Y', 'Kinv', 'alpha', 'loo', 'cv', 'dloo', 'dxY', 'dxvec')    # workspace buffers sized by the padded N

    def observe_more(self, inputs, outputs, params=None):
        """Append observations: afterwards the process is what observed(all inputs, all outputs) would have made it, up to
        rounding (the reference has no counterpart: it refits).  When the factor cached for these hyper-parameter values
        (params=None: the current ones) and the observations so far was solved without jitter, fallback or pivot failure, on
        one GPU, it is extended in place -- a lower Cholesky factor is built from its leading principal submatrices, so only
        the block rows from rounddown(N, 128) on are computed (g3_gp_append), and a cached cross solve at the last space is
        extended by the new columns (g3_gp_cross_append).  A following logp / predict / dlogp / loo on the same parameters
        finds the factor.  Everywhere else -- no such factor, a jittered one, a diagonal the reference's tt_to_cov would
        have lifted, a failed pivot among the new rows, several GPUs -- the data are extended, the cache is dropped and
        the next call factors everything through the usual path.  `append_stats` counts which way each call went.  From the
        first call on, the workspace carries slack and grows geometrically."""
        Xn = self._x(inputs)
        yn = np.asarray(outputs, dtype=self.dtype).reshape(-1)
        if len(Xn) != len(yn):
            raise _lib.G3Error('observe_more: %d inputs for %d outputs' % (len(Xn), len(yn)))
        if len(Xn) == 0:
            return
        if not self.is_observed:
            self.observed(Xn, yn)
            self._cache = None
            self.append_stats['refit'] += 1
            return
        X0, y0 = self._x(self._inputs), np.asarray(self._outputs, dtype=self.dtype).reshape(-1)
        if Xn.shape[1] != X0.shape[1]:
            raise _lib.G3Error('observe_more: inputs with %d columns, the process has %d' % (Xn.shape[1], X0.shape[1]))
        X1, y1 = np.concatenate([X0, Xn]), np.concatenate([y0, yn])
        values, _ = self._values(self.params if params is None else self.filter_params(params))
        c = self._cache
        key = tuple((k, np.asarray(v).tobytes()) for k, v in sorted(values.items()))
        st = c['stats'] if c is not None else None
        fast = (self._dist is None and st is not None and c['which'] is not None and c['key'] == (key, X0.shape)
                and st['tries'] == 0 and not st['fallback'] and st['info'] == 0
                and np.array_equal(c['X'], X0) and np.array_equal(c['y'], y0))
        self.observed(X1, y1)
        if fast:
            try:
                fast = self._append(c, values, key, Xn, yn, X1, y1)
            except Exception:
                self._cache = self._workspace = None
                raise
        if not fast:
            self._cache = None
            self.append_stats['refit'] += 1

    def _reserve(self, c, N1):
        """the factor workspace with room for N1 observations: capacity grows by >= 1.5 (a multiple of 128, the leading
        dimension), what the factor of the whole blocks below n0 consists of is moved on the device; c's and the
        workspace's buffers become views of N1 rows"""
        dev, ws, t = self.device, self._workspace, self.dtype
        back = ws.setdefault('back', {k: ws[k] for k in ('Kd', 'Wd', 'ad', 'Xd', 'dvec')})
        N0, d, P = c['N'], c['d'], _lib.G3_PAD
        n0, Np1 = N0 // P * P, _lib.roundup(N1)
        old = []
        cap = back['Kd'].ld
        if Np1 > cap or back['Wd'].rows < Np1 or back['ad'].ld < Np1:
            cap = _lib.append_capacity(cap, Np1)
            new = dict(Kd=dev.alloc(cap + _lib.G3_RHS_PAD, cap, t), Wd=dev.alloc_inverses(cap, t), ad=dev.alloc(1, cap, t))
            if n0 > 0:
                dev.copy2d(new['Kd'], back['Kd'], n0, n0)
                dev.copy2d(new['Wd'], back['Wd'], n0, P)
                dev.copy2d(new['ad'], back['ad'], 1, n0)
            old += [back[k] for k in new]
            back.update(new)
        if back['Xd'].rows < N1:
            capx = _lib.append_capacity(back['Xd'].rows, N1)
            Xd = dev.alloc(capx, d, t)
            dev.copy2d(Xd, back['Xd'], N0, d)
            old += [back['Xd'], back['dvec']]
            back['Xd'], back['dvec'] = Xd, dev.alloc(1, capx, t)
        views = dict(Kd=dev.wrap(back['Kd'].ptr, Np1 + _lib.G3_RHS_PAD, Np1, back['Kd'].ld, t, keep=back['Kd']),
                     Wd=dev.wrap(back['Wd'].ptr, Np1, P, P, t, keep=back['Wd']),
                     ad=dev.wrap(back['ad'].ptr, 1, Np1, back['ad'].ld, t, keep=back['ad']),
                     Xd=dev.wrap(back['Xd'].ptr, N1, d, back['Xd'].ld, t, keep=back['Xd']),
                     dvec=dev.wrap(back['dvec'].ptr, 1, N1, back['dvec'].ld, t, keep=back['dvec']))
        ws.update(views)
        return views, old

    def _append(self, c, values, key, Xn, yn, X1, y1):
        """the fast path of observe_more on the cached factor c; False: declined, the caller refits"""
        dev, ws, t = self.device, self._workspace, self.dtype
        N0, d, Np0 = c['N'], c['d'], c['Np']
        N1, Np1 = len(X1), _lib.roundup(len(X1))
        n0 = N0 // _lib.G3_PAD * _lib.G3_PAD
        # the right-hand side of the new points alone: mapping and location are pointwise (elliptical.py:63)
        mapped, mu, delta, det_m = self._delta(values, Xn, yn)
        mapped_num = to_num(mapped, t)
        delta1 = np.concatenate([c['delta'], delta])
        post1 = np.concatenate([c['delta_post'], mapped_num - mu])
        dl = delta1 if c['which'] == 'logp' else post1
        v, old = self._reserve(c, N1)
        dev.copy_in(dev.wrap(v['Xd'].offset(N0), N1 - N0, d, v['Xd'].ld, t, keep=v['Xd']), Xn)
        dev.copy_in(v['dvec'], np.where(np.isfinite(dl), dl, 0).astype(t))
        prog = self._prog(self.f_kernel_noise, values, d)
        st = dev.gp_append(prog, v['Xd'], N0, N1, d, v['dvec'], v['Kd'], v['Wd'], v['ad'])
        for b in old:
            b.free()
        if st.pop('refused') or st['info'] != 0:
            self._workspace = None
            return False
        st['delta_finite'] = bool(np.all(np.isfinite(dl)))
        if Np1 != Np0:
            for k in self._NP_SCRATCH:
                if k in ws:
                    ws.pop(k).free()
        ws['shape'], ws['X'] = X1.shape, X1.copy()
        cross = c.get('cross')
        c.update(key=(key, X1.shape), X=ws['X'].copy(), y=y1.copy(), N=N1, Np=Np1, delta=delta1, delta_post=post1,
                 z=np.concatenate([c['z'], mapped_num]), mu=np.concatenate([c['mu'], mu]),
                 det_m=np.asarray(c['det_m'] + det_m, dtype=t)[()], stats=st, grad=None, loo=None, cv=None, dx=None, cross=None,
                 same_delta=bool(np.array_equal(delta1, post1)), **{k: v[k] for k in ('Xd', 'Kd', 'Wd', 'ad')})
        self.append_stats['appended'] += 1
        if cross is not None and cross['out'][0] is not None:
            # the cross solve at the last space: its columns below n0 stand, the new ones are solved against the corner
            V, _, _, M, Mp = cross['out']
            if V.ld < Np1:
                V2 = dev.alloc(Mp, _lib.append_capacity(V.ld, Np1), t)
                if n0 > 0:
                    dev.copy2d(V2, V, Mp, n0)
                V, dead = V2, V
            else:
                dead = None
            noise, _ = cross['kid']
            kern = cross['kernel_ref'] if cross.get('kernel_ref') is not None else (self.f_kernel_noise if noise else self.f_kernel)
            mud, ssd = dev.alloc(1, Mp, t), dev.alloc(1, Mp, t)
            dev.gp_cross_append(self._prog(kern, values, d), dev.upload(cross['S']), M, c['Xd'], N0, N1, d, c['Kd'], c['Wd'], c['ad'],
                                V, mud, ssd)
            cross['out'] = (V, dev.download(mud, 1, M)[0], dev.download(ssd, 1, M)[0], M, Mp)
            if dead is not None:
                dead.free()
            c['cross'] = cross
            self.append_stats['cross_appended'] += 1
        return True

    def _cross(self, c, values, space, noise, kernel=None):
        """V = K(space, X) L^-T, mu = V a, ss = |V_i|^2 (elliptical.py:78-91)"""
        dev = self.device
        S = self._x(space)
        M = S.shape[0]
        Mp = _lib.roundup(M, _lib.G3_RHS_PAD)
        # predict() asks for mean, variance, quantiles ... one after the other (the reference compiles and runs one
        # function per statistic, each with its own solves, elliptical.py:81-91): the N^2 M cross solve is shared
        # between them while factor, right-hand side, space and kernel stay the same
        kid = (bool(noise), id(kernel) if kernel is not None else None)
        cc = c.get('cross')
        if self._dist is not None:
            # the Noise term contributes nothing to a cross block (kernels.py:367-371): one cross solve serves both flags
            kd = id(kernel) if kernel is not None else None
            if cc is None or cc['kid'][1] != kd or cc['S'].shape != S.shape or not np.array_equal(cc['S'], S):
                dl = c['delta'] if c['which'] == 'logp' else c['delta_post']
                st, cc = self._dist_step(c, values, dl, S, cross_kernel=kernel)   # another space / cross kernel: one more evaluation
                cc['kernel_ref'] = kernel          # keeps the object alive: its id() cannot be handed to another kernel
                c['stats'], c['cross'] = dict(st, delta_finite=c['stats']['delta_finite']), cc
            return cc['out']
        if cc is not None and cc['kid'] == kid and cc['S'].shape == S.shape and np.array_equal(cc['S'], S):
            return cc['out']
        Sd = dev.upload(S)
        V = dev.alloc(Mp, c['Np'], self.dtype)
        mu = dev.alloc(1, Mp, self.dtype)
        ss = dev.alloc(1, Mp, self.dtype)
        kern = kernel if kernel is not None else (self.f_kernel_noise if noise else self.f_kernel)
        dev.gp_cross(self._prog(kern, values, c['d']), Sd, M, c['Xd'], c['N'], c['d'], c['Kd'], c['Wd'], c['ad'], V, mu, ss)
        out = (V, dev.download(mu, 1, M)[0], dev.download(ss, 1, M)[0], M, Mp)
        c['cross'] = dict(kid=kid, S=S.copy(), out=out, kernel_ref=kernel)   # (the reference pins id(kernel))
        return out

    def _prior_gram(self, values, space, noise, pad=False):
        """prior_kernel_space = tt_to_cov(K_noise(space)) / prior_kernel_f_space = K_f(space)
        (elliptical.py:70,74) as a device matrix"""
        dev = self.device
        S = self._x(space)
        M, d = S.shape
        Mp = _lib.roundup(M, _lib.G3_RHS_PAD) if pad else M
        Sd = dev.upload(S)
        K = dev.alloc(Mp, Mp, self.dtype)
        kern = self.f_kernel_noise if noise else self.f_kernel
        dev.gram(self._prog(kern, values, d), Sd, None, d, K, Mp, Mp, _lib.G3_GRAM_SCRUB if noise else 0)
        if noise:
            dev.cov_lift(K, M)
        return K, M, Mp

    def _prior_diag(self, values, space, noise):
        dev = self.device
        S = self._x(space)
        M, d = S.shape
        Sd = dev.upload(S)
        out = dev.alloc(1, M, self.dtype)
        kern = self.f_kernel_noise if noise else self.f_kernel
        dev.gram_diag(self._prog(kern, values, d), Sd, d, out)
        dg = dev.download(out, 1, M)[0]
        if noise:   # tt_to_cov acts on the whole matrix; its effect on the diagonal:
            dg = to_num(dg, self.dtype)
            m = dg.min()
            if not m > 0:
                dg = dg + (self.dtype.type(np.float32(1e-6)) - m)
        return dg

    # ---------------------------------------------------------------- statistics (th_* of the reference)
    def th_define_process(self):
        pass   # the symbolic graph of elliptical.py:60-107 is replaced by the methods below

    def th_freedom(self, space, inputs, outputs, vector, params, prior=False, noise=False):
        """prior degrees of freedom, plus the number of observations a posteriori (elliptical.py:109-113)"""
        if self.f_degree is None:
            return None
        values, _ = self._values(params)
        nu = self.f_degree(values)
        return self.dtype.type(nu if prior else nu + len(np.asarray(inputs)))

    def th_logp(self, space, inputs, outputs, vector, params, prior=False, noise=False):
        """sum of the free variables' log-densities (Flat: 0; FlatExp: the log-transform Jacobian
        term; potentials) plus the observed term unless prior (stochastic.py:300-306)"""
        _, logjac = self._values(params)
        t = self.dtype.type
        if prior:
            return t(logjac)
        return t(logjac + self.th_loglike(space, inputs, outputs, vector, params))

    def th_mapping_inv(self, space, inputs, outputs, vector, params, prior=False, noise=False):
        values, _ = self._values(params)
        with np.errstate(all='ignore'):
            r = np.asarray(self.f_mapping.inv(np.asarray(outputs, dtype=self.dtype), values))
        return to_num(r, self.dtype)

    def th_mapping(self, space, inputs, outputs, vector, params, prior=False, noise=False):
        values, _ = self._values(params)
        with np.errstate(all='ignore'):
            r = np.asarray(self.f_mapping(np.asarray(outputs, dtype=self.dtype), values))
        return to_num(r, self.dtype)

    def th_location(self, space, inputs, outputs, vector, params, prior=False, noise=False):
        values, _ = self._values(params)
        S = self._x(space)
        loc = self.f_location(S, values)
        if prior:
            return loc                                                    # elliptical.py:122-123
        c = self._factor(values, inputs, outputs)
        self._solve(c, values, 'post')
        _, mu, _, _, _ = self._cross(c, values, space, noise)
        return loc + mu                                                   # elliptical.py:81-84

    def th_cross_mean(self, space, inputs, outputs, vector, params, prior=False, noise=False, cross_kernel=None):
        """location of one process given another through a cross kernel (gaussian.py:99-112)"""
        values, _ = self._values(params)
        loc = self.f_location(self._x(space), values)
        if prior:
            return loc
        c = self._factor(values, inputs, outputs)
        self._solve(c, values, 'post')
        _, mu, _, _, _ = self._cross(c, values, space, False, kernel=cross_kernel)
        return loc + mu

    def _kernel_dev(self, space, inputs, outputs, params, prior, noise):
        """prior / posterior covariance of `space` as a DEVICE matrix: (K, M, rows of K)"""
        values, _ = self._values(params)
        dev = self.device
        if prior:
            K, M, Mp = self._prior_gram(values, space, noise)
            return K, M, Mp
        c = self._factor(values, inputs, outputs)
        self._solve(c, values, c['which'] or 'post')
        if self._dist is not None:
            # several GPUs: V = K(space, X) L^-T lives in the driver's right-hand-side rows; every rank forms the rows of
            # its chunks, the M x M matrix is gathered on all of them (g3_dist_posterior_cov)
            _, _, _, M, Mp = self._cross(c, values, space, noise)        # the driver's last evaluation is at this space
            K = dev.alloc(Mp, Mp, self.dtype)
            kern = self.f_kernel_noise if noise else self.f_kernel
            self._dist['dgp'].posterior_cov(kern.spec(values, c['d']), dev.upload(self._x(space)), K)
            return K, M, Mp
        V, _, _, M, Mp = self._cross(c, values, space, noise)
        K, _, _ = self._prior_gram(values, space, noise, pad=True)
        dev.gemm_nt(K, V, V, Mp, Mp, c['Np'], alpha=-1.0, beta=1.0)        # elliptical.py:86-91
        return K, M, Mp

    def th_kernel(self, space, inputs, outputs, vector, params, prior=False, noise=False):
        K, M, _ = self._kernel_dev(space, inputs, outputs, params, prior, noise)
        return self.device.download(K, M, M)

    def th_cholesky_dev(self, space, inputs, outputs, vector, params, prior=False, noise=False):
        """cholesky_robust of the prior / posterior covariance, kept on the device: (L zero-padded to
        a multiple of 128, M, padded size) -- what the samplers multiply the normal draws with"""
        dev = self.device
        K, M, _ = self._kernel_dev(space, inputs, outputs, params, prior, noise)
        Mp = _lib.roundup(M, _lib.G3_RHS_PAD)
        Ld = dev.alloc(Mp, Mp, self.dtype, zero=True)
        dev.potrf_robust(K, Ld, M)                                        # elliptical.py:72,76,88,92
        return Ld, M, Mp

    def th_cholesky(self, space, inputs, outputs, vector, params, prior=False, noise=False):
        Ld, M, _ = self.th_cholesky_dev(space, inputs, outputs, vector, params, prior=prior, noise=noise)
        return self.device.download(Ld, M, M)

    def th_kernel_diag(self, space, inputs, outputs, vector, params, prior=False, noise=False):
        values, _ = self._values(params)
        dg = self._prior_diag(values, space, noise)
        if not prior:
            c = self._factor(values, inputs, outputs)
            self._solve(c, values, c['which'] or 'post')
            _, _, ss, _, _ = self._cross(c, values, space, noise)
            dg = dg - ss
        return np.where(dg < 0, self.dtype.type(0), dg)                   # tt_to_bounded(., 0) elliptical.py:94-97

    def th_kernel_sd(self, space, inputs, outputs, vector, params, prior=False, noise=False):
        return np.sqrt(self.th_kernel_diag(space, inputs, outputs, vector, params, prior=prior, noise=noise))

    def th_cholesky_diag(self, space, inputs, outputs, vector, params, prior=False, noise=False):
        return np.diag(self.th_kernel_sd(space, inputs, outputs, vector, params, prior=prior, noise=noise))

    def _loc_sd(self, space, inputs, outputs, params, prior, noise, sd_noise=None):
        """location and sd from ONE cross solve (the reference runs two compiled functions)"""
        values, _ = self._values(params)
        S = self._x(space)
        loc = self.f_location(S, values)
        sd_noise = noise if sd_noise is None else sd_noise
        dg = self._prior_diag(values, space, sd_noise)
        if not prior:
            c = self._factor(values, inputs, outputs)
            self._solve(c, values, 'post')
            _, mu, ss, _, _ = self._cross(c, values, space, noise)
            loc = loc + mu
            dg = dg - ss
        dg = np.where(dg < 0, self.dtype.type(0), dg)
        return loc, np.sqrt(dg), values

    # ---- gradients with respect to the query inputs (in the reference: tt.grad(..., space) through elliptical.py:81-97)
    def predict_dx(self, params=None, space=None, inputs=None, outputs=None, location=True, kernel_diag=True, kernel_sd=False,
                   prior=False, noise=False):
        """Gradients with respect to `space` of what `location`, `kernel_diag` and `kernel_sd` return for the same arguments:
        a DictObj of (M, d) arrays under those three keys.  These are latent quantities; with the Identity mapping they are the
        gradients of predict's mean, variance and std.  With alpha = K^-1 delta and w_i = K^-1 k(X, x_i) of the factored
        (possibly jittered) covariance,
            d location / d x_i = d m / d x_i + sum_j alpha_j d1 k(x_i, x_j)
            d diag / d x_i     = d k(x, x) / d x |x_i - 2 sum_j w_ij d1 k(x_i, x_j)
        d1 being the gradient with respect to the kernel's first argument (g3_gp_cross_dx, g3_gram_diag_dx).  kernel_diag is
        clipped at 0, and its gradient is 0 where it clips; kernel_sd's is d diag / (2 sd), 0 where sd == 0; the lift tt_to_cov
        applies to a non-positive prior diagonal with noise=True counts as a constant.  prior=True needs no factor; an
        unobserved process falls back to the prior, as every method does.  A `predict` at the same space before it shares
        the cross solve, and L^-T and alpha are kept with the factor: after the first call on a factor a call costs the
        2 N^2 M product W = V L^-1 plus one pass over the M x N pairs.  Out of scope: a chain of hyper-parameter vectors,
        the Student-t scaling of a TProcess, and the mapped statistics (mean, variance, quantiles) through a mapping other
        than Identity."""
        if self._dist is not None:
            raise _lib.G3Error('predict_dx runs on one GPU')
        params, space, inputs, outputs, prior = self._call_defaults(params, space, inputs, outputs, prior, False)
        values, _ = self._values(params)
        dev, t = self.device, self.dtype
        S = self._x(space)
        M, d = S.shape
        want_diag = kernel_diag or kernel_sd
        kern = self.f_kernel_noise if noise else self.f_kernel
        prog = self._prog(kern, values, d)
        Sd = dev.upload(S)
        dloc = np.asarray(self.f_location.dx(S, values), dtype=t) if location else None
        ddiag = dg = None
        if want_diag:
            dk = dev.alloc(M, d, t)
            dev.gram_diag_dx(prog, Sd, M, d, dk)
            ddiag = dev.download(dk)
            dg = self._prior_diag(values, space, noise)
        if not prior:
            c = self._factor(values, inputs, outputs)
            self._solve(c, values, 'post')
            V, _, ss, _, Mp = self._cross(c, values, space, noise)
            N, Np = c['N'], c['Np']
            ws = self._workspace
            if c.get('dx') is None:
                # a buffer of its own: dlogp and dloo overwrite the shared scratch ws['Y']
                if 'dxY' not in ws:
                    ws['dxY'], ws['dxvec'] = dev.alloc(Np, Np, t), dev.alloc(2, Np, t)
                vec = ws['dxvec']
                dev.gp_loo(N, c['Kd'], c['Wd'], c['ad'], ws['dxY'], vec, dev.wrap(vec.offset(1), 1, Np, Np, t, keep=vec))
                c['dx'] = (ws['dxY'], vec)
            Y, alpha = c['dx']
            dmu = dev.alloc(M, d, t) if location else None
            dss = dev.alloc(M, d, t) if want_diag else None
            Wm = dev.alloc(Mp, Np, t) if want_diag else None
            dev.gp_cross_dx(prog, Sd, M, c['Xd'], N, d, alpha, V if want_diag else None, Y if want_diag else None, Wm, dmu, dss)
            if location:
                dloc = dloc + dev.download(dmu)
            if want_diag:
                ddiag = ddiag - dev.download(dss)
                dg = dg - ss
        out = DictObj()
        if location:
            out['location'] = dloc
        if want_diag:
            ddiag = np.where((dg < 0)[:, None], t.type(0), ddiag)            # tt_to_bounded(., 0) elliptical.py:94-97
            if kernel_diag:
                out['kernel_diag'] = ddiag
            if kernel_sd:
                sd = np.sqrt(np.where(dg < 0, t.type(0), dg))
                with np.errstate(all='ignore'):
                    out['kernel_sd'] = np.where((sd > 0)[:, None], ddiag / (2 * sd)[:, None], t.type(0))
        return out

    def th_median(self, space, inputs, outputs, vector, params, prior=False, noise=False):
        values, _ = self._values(params)
        return self.f_mapping(self.th_location(space, inputs, outputs, vector, params, prior, noise), values)

    def th_mean(self, space, inputs, outputs, vector, params, prior=False, noise=False):
        values, _ = self._values(params)
        return self.f_mapping(self.th_location(space, inputs, outputs, vector, params, prior, noise), values)

    def th_variance(self, space, inputs, outputs, vector, params, prior=False, noise=False):
        return self.th_kernel_diag(space, inputs, outputs, vector, params, prior=prior, noise=noise)

    def th_std(self, space, inputs, outputs, vector, params, prior=False, noise=False):
        return np.sqrt(self.th_variance(space, inputs, outputs, vector, params, prior=prior, noise=noise))

    def th_covariance(self, space, inputs, outputs, vector, params, prior=False, noise=False):
        return self.th_kernel(space, inputs, outputs, vector, params, prior=prior, noise=noise)

    # ---- errors of the predictive mean against a supplied vector (stochastic.py:315-326)
    def th_error_l1(self, space, inputs, outputs, vector, params, prior=False, noise=False):
        mean = self.th_mean(space, inputs, outputs, vector, params, prior=prior, noise=noise)
        return np.mean(np.abs(np.asarray(vector, dtype=self.dtype) - mean))

    def th_error_l2(self, space, inputs, outputs, vector, params, prior=False, noise=False):
        mean = self.th_mean(space, inputs, outputs, vector, params, prior=prior, noise=noise)
        return np.mean((np.asarray(vector, dtype=self.dtype) - mean) ** 2)

    def th_error_mse(self, space, inputs, outputs, vector, params, prior=False, noise=False):
        d = np.abs(np.asarray(vector, dtype=self.dtype) - np.asarray(outputs, dtype=self.dtype))
        return np.mean(d) ** 2 + np.var(d)

    _methods = (('mean', 'th_mean'), ('median', 'th_median'), ('variance', 'th_variance'), ('std', 'th_std'),
                ('covariance', 'th_covariance'), ('logpredictive', 'th_logpredictive'), ('logp', 'th_logp'),
                ('loglike', 'th_loglike'), ('mapping', 'th_mapping'), ('mapping_inv', 'th_mapping_inv'),
                ('location', 'th_location'), ('kernel', 'th_kernel'), ('cholesky', 'th_cholesky'),
                ('kernel_diag', 'th_kernel_diag'), ('kernel_sd', 'th_kernel_sd'),
                ('cholesky_diag', 'th_cholesky_diag'), ('cross_mean', 'th_cross_mean'), ('freedom', 'th_freedom'),
                ('error_l1', 'th_error_l1'), ('error_l2', 'th_error_l2'), ('error_mse', 'th_error_mse'),
                ('_cholesky_dev', 'th_cholesky_dev'))
