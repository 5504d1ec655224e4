"""StochasticProcess: the user-facing API, parameter conventions and compiled-method dispatch
of g3py/processes/stochastic.py:20-105, 150-201, 300-313, 385-430, 444-513, rebuilt on the
HIP path.  Optimisers, MCMC drivers, plotting and pickling are out of scope.
"""
import types

import numpy as np

from ..libs import DictObj, clone
from ..libs.tensors import makefn
from .hypers import Model


class GraphicalModel:
    """The slice of g3py/bayesian/models.py:56-182 the path depends on: the variable registry,
    default / current parameters and the dict <-> flat-array bijection (models.py:143-155)."""
    active = None

    def __init__(self, name='GM'):
        self.name = name
        self.model = Model(name)
        self.components = DictObj()
        self.current_params = None
        self.fix_vars()

    def add_component(self, component):
        self.components[component.name] = component

    def compile_components(self, precompile=False):
        pass

    # ---- bijection (pm.DictToArrayBijection over vars in creation order)
    @property
    def ndim(self):
        return self.model.ndim

    def dict_to_array(self, params):
        return np.concatenate([np.asarray(params[v.key], dtype=np.float64).reshape(-1)
                               for v in self.model.vars]) if self.model.vars else np.zeros(0)

    def array_to_dict(self, array):
        array = np.asarray(array, dtype=np.float64).reshape(-1)
        r, o = DictObj(), 0
        for v in self.model.vars:
            r[v.key] = array[o:o + v.size].reshape(v.shape)
            o += v.size
        return r

    class _Bijection:
        def __init__(self, gm):
            self.map = gm.dict_to_array
            self.rmap = gm.array_to_dict

    @property
    def bijection(self):
        return GraphicalModel._Bijection(self)

    # ---- fixed chains (models.py:270-296): some variables are pinned to the rows of a chain / datatrace,
    #      the others are the ones an optimiser or sampler moves
    def fix_vars(self, datatrace=None, keys=None):
        """`datatrace`: 2-D array or DataFrame whose first `ndim` columns are flat parameter vectors;
        `keys`: the names (transformed keys or natural names) of the variables that stay fixed"""
        if datatrace is None or keys is None:
            self.fixed_keys, self.fixed_datatrace, self.fixed_chain, self.fixed_dims = [], None, None, []
            return
        self.fixed_keys = list(keys)
        self.fixed_datatrace = datatrace.copy()
        values = getattr(self.fixed_datatrace, 'values', self.fixed_datatrace)
        self.fixed_chain = np.array(np.asarray(values)[:, :self.ndim], dtype=np.float64)
        dims, o = [], 0
        for v in self.model.vars:
            if v.key in self.fixed_keys or v.name in self.fixed_keys:
                dims += list(range(o, o + v.size))
            o += v.size
        self.fixed_dims = sorted(dims)

    @property
    def sampling_dims(self):
        return sorted(set(range(self.ndim)) - set(self.fixed_dims))

    def sampling_params(self, params):
        """the entries an optimiser / sampler moves, from a dict or a flat vector"""
        flat = self.dict_to_array(params) if isinstance(params, dict) else np.asarray(params)
        return flat[self.sampling_dims]

    def dict_from_sampling_array(self, params):
        """inverse of sampling_params: the moved entries spliced into the current parameter vector"""
        flat = np.asarray(params, dtype=np.float64)
        if self.fixed_datatrace is not None:
            full = self.dict_to_array(self.params)
            full[self.sampling_dims] = flat
            flat = full
        return self.array_to_dict(flat)

    # ---- parameters
    def set_params(self, params=None):
        self.current_params = None if params is None else DictObj(params)

    @property
    def params(self):
        """a copy of the parameters set with set_params, else the defaults"""
        return self.params_default if self.current_params is None else clone(self.current_params)

    @property
    def params_test(self):
        return DictObj(self.model.test_point)

    @property
    def params_default(self):
        """models.py:174-182 + transformed_hypers (:46-53): defaults in transformed space"""
        out = self.params_test
        mine = set(self.model.vars)
        for component in self.components.values():
            for var, natural in component.default_hypers().items():
                if var not in mine:
                    continue
                value = np.asarray(natural, dtype=np.float64)
                if var.positive:
                    with np.errstate(all='ignore'):
                        value = np.log(value)
                out[var.key] = value.reshape(var.shape)
        return out

    def transform_params(self, params, to_dict=True, to_transformed=True, complete=False):
        """natural <-> transformed names and values (models.py:232-260)"""
        if not isinstance(params, dict):
            params = self.array_to_dict(params)
        r = DictObj(self.params) if (complete or not to_dict) else DictObj()
        by_name = {v.name: v for v in self.model.vars}
        by_key = {v.key: v for v in self.model.vars}
        for k, val in params.items():
            if to_transformed and k in by_name and by_name[k].positive:
                r[by_name[k].key] = np.log(val)
            elif (not to_transformed) and k in by_key and by_key[k].positive:
                r[by_key[k].name] = np.exp(val)
            else:
                r[k] = val
        return r if to_dict else self.dict_to_array(r)


class StochasticProcess:
    """stochastic.py:20-105 (construction), :150-201 (space/observations), :385-430
    (method dispatch), :444-513 (predict)."""

    def __init__(self, space=None, order=None, inputs=None, outputs=None, hidden=None, index=None,
                 name='SP', distribution=None, active=False, precompile=False, file=None, load=True,
                 compile_logp=True, dtype=np.float64, device=None, *args, **kwargs):
        self.makefn = makefn
        self.nspace = self._columns_of(space)
        self.name = name
        self.dtype = np.dtype(dtype)
        self._device = device
        # until set_space / observed supply data every array is the reference's 2-point dummy (:46-56)
        pair = np.array([0.0, 1.0], dtype=self.dtype)
        grid = np.tile(pair[:, None], (1, self.nspace))
        self._order, self._index, self._outputs = pair.copy(), pair.copy(), pair.copy()
        self._space, self._inputs = grid.copy(), grid.copy()
        self.is_observed, self.np_hidden, self.distribution = False, None, distribution
        self.active = self._graph_for(active)
        self.active.add_component(self)
        self.compiles = DictObj()
        self.precompile = precompile
        self.file = file   # accepted for signature compatibility; pickling is out of scope
        with self.model:
            self._check_hypers()
            self.th_define_process()
            self.active.compile_components()
        self.set_space(space=space, hidden=hidden, order=order, inputs=inputs, outputs=outputs, index=index)
        self._compile_methods(compile_logp)
        if hidden is None:
            self.hidden = hidden

    @staticmethod
    def _columns_of(space):
        """number of input columns: from an array's second axis, or given directly as an int"""
        if space is None:
            return 1
        shape = getattr(space, 'shape', None)
        if shape is None:
            return int(space)
        return shape[1] if len(shape) > 1 else 1

    def _graph_for(self, active):
        """True: the shared model of all active=True processes; False: a private one; else the given one"""
        if active is True:
            if GraphicalModel.active is None:
                GraphicalModel.active = GraphicalModel('GM_' + self.name)
            return GraphicalModel.active
        return GraphicalModel('GM_' + self.name) if active is False else active

    # ---- parameters
    def set_params(self, *args, **kwargs):
        return self.active.set_params(*args, **kwargs)

    def transform_params(self, *args, **kwargs):
        return self.active.transform_params(*args, **kwargs)

    @property
    def model(self):
        return self.active.model

    @property
    def params(self):
        return self.active.params

    @property
    def params_default(self):
        return self.active.params_default

    @property
    def params_test(self):
        return self.active.params_test

    def filter_params(self, params):
        return {k: params[k] for k in self.model.test_point}   # models.py:471-473

    # ---- space and observations (boundary: stochastic.py:150-201, 219-259 -- copy on set)
    # how each array handed to set_space is normalised: True = matrix (a vector becomes one column),
    # False = vector (a matrix is flattened to its first axis)
    _ARRAY_RANK2 = (('space', True), ('hidden', False), ('order', False), ('inputs', True),
                    ('outputs', False), ('index', False))
    # a vector that, when not supplied for a one-dimensional space, mirrors a matrix; and the
    # matrix whose length it must match otherwise (it falls back to 0..n-1)
    _MIRRORS = (('order', 'space'), ('index', 'inputs'))

    def set_space(self, space=None, hidden=None, order=None, inputs=None, outputs=None, index=None):
        given = dict(space=space, hidden=hidden, order=order, inputs=inputs, outputs=outputs, index=index)
        for name, rank2 in self._ARRAY_RANK2:
            a = given[name]
            if a is None:
                continue
            a = np.asarray(a)
            n = len(a)
            if rank2 and a.ndim < 2:
                a = a.reshape(n, 1)
            elif not rank2 and a.ndim > 1:
                a = a.reshape(n)
            setattr(self, name, a)
        for vec, mat in self._MIRRORS:
            m = getattr(self, mat)
            if given[vec] is None and self.nspace == 1:
                setattr(self, vec, m.reshape(len(m)))
            if len(getattr(self, vec)) != len(m):
                setattr(self, vec, np.arange(len(m)))

    def observed(self, inputs=None, outputs=None, order=None, index=None, hidden=None):
        self.set_space(inputs=inputs, outputs=outputs, order=order, index=index, hidden=hidden)
        self.is_observed = not (inputs is None and outputs is None)

    def _get(self, name):
        return getattr(self, '_' + name).copy()

    def _set(self, name, value):
        setattr(self, '_' + name, np.array(value, dtype=self.dtype, copy=True))

    space = property(lambda s: s._get('space'), lambda s, v: s._set('space', v))
    inputs = property(lambda s: s._get('inputs'), lambda s, v: s._set('inputs', v))
    outputs = property(lambda s: s._get('outputs'), lambda s, v: s._set('outputs', v))
    order = property(lambda s: s._get('order'), lambda s, v: s._set('order', v))
    index = property(lambda s: s._get('index'), lambda s, v: s._set('index', v))

    @property
    def hidden(self):
        return self.np_hidden

    @hidden.setter
    def hidden(self, value):
        self.np_hidden = value

    def _natural(self, raw, lead):
        """the one body of _values (lead = ()) and _values_rows (lead = (B,)): natural-space values by hyper name from
        raw(v), the transformed-space value of variable v shaped lead + v.shape, and the terms every process adds to logp
        besides the observed density, shaped lead -- the log-Jacobian of the FlatExp variables (hypers/__init__.py:199-200)
        and the L1 / L2 potentials registered by check_potential (hypers/__init__.py:94-109), which enter th_logp like
        pm.Potential terms (stochastic.py:305).  Reductions run over a variable's own entries, per row."""
        values, logjac = {}, np.zeros(lead)
        with np.errstate(over='ignore'):
            for v in self.model.vars:
                p = raw(v)
                if v.positive:
                    p = np.exp(p)
                    logjac = logjac + np.where(p > 1e-6, 0.0, -np.inf).reshape(lead + (-1,)).sum(axis=-1)
                values[v.name] = p
        for _, reg, c, sel in self.model.potentials:
            if reg in ('L1', 'L2'):
                tot = np.zeros(lead)
                for h in sel:
                    hv = np.asarray(values[h.name]).reshape(lead + (-1,))
                    tot = tot + (np.abs(hv).sum(axis=-1) if reg == 'L1' else (hv ** 2).sum(axis=-1))
                logjac = logjac + c * -tot
        return values, logjac

    def _values(self, params):
        """transformed-space params dict -> (natural-space values by hyper name, extra logp terms as a float): _natural
        for one hyper-parameter vector, remembered per params object.  Shared by the elliptical and the transport
        processes."""
        memo = getattr(self, '_values_memo', None)
        if memo is not None and memo[0] is params:          # th_logp -> th_loglike -> ... share one params object
            return memo[1], memo[2]
        values, logjac = self._natural(lambda v: np.asarray(params[v.key], dtype=np.float64), ())
        self._values_memo = (params, values, float(logjac))
        return values, float(logjac)

    def _values_rows(self, chain):
        """_natural for every row of a flat-parameter chain at once: {hyper name: Rows (B, *shape)} and the (B,) extra
        logp terms"""
        from ..device import Rows
        chain = np.asarray(chain, dtype=np.float64)
        B = len(chain)
        at = np.cumsum([0] + [v.size for v in self.model.vars])
        cols = {v.name: slice(at[i], at[i + 1]) for i, v in enumerate(self.model.vars)}
        values, logjac = self._natural(lambda v: chain[:, cols[v.name]].reshape((B,) + tuple(v.shape)), (B,))
        return {k: np.ascontiguousarray(p).view(Rows) for k, p in values.items()}, logjac

    @staticmethod
    def _values_row(values_rows, j):
        """row j of _values_rows as the plain dict _values returns"""
        return {k: np.asarray(v)[j] for k, v in values_rows.items()}

    # ---- to be provided by subclasses
    def default_hypers(self):
        return {}

    def _check_hypers(self):
        pass

    def th_define_process(self):
        pass

    def sampler(self, samples=1, prior=False, noise=False):
        pass

    def quantiler(self, q=0.975, prior=False, noise=False, simulations=None):
        pass

    # names of the statistics a subclass implements as  fn(ctx, prior, noise, **kw)
    _methods = ()

    def _compile_methods(self, compile_logp=True):
        """bind every statistic as a lazily 'compiled' method (stochastic.py:328-380)"""
        if self.compiles is None:
            self.compiles = DictObj()
        for public, th_name in self._methods:
            setattr(self, public, types.MethodType(self._method_name(th_name), self))
        if compile_logp:
            # the reference force-compiles logp on the 2-point dummy data here; our kernels are
            # already compiled, so only the registry entries are created
            for prior in (False, True):
                self._compiled('th_logp', prior, False, True, (), {})

    def _compiled(self, method, prior, noise, array, args, kwargs):
        # registry key, e.g. posterior_logp, prior_kernel_sd_noise (boundary: stochastic.py:404-415)
        name = ''.join(['prior' if prior else 'posterior', method.replace('th', ''), '_noise' if noise else '',
                        str(args) if args else '', str(kwargs) if kwargs else ''])
        if name not in self.compiles:
            impl = getattr(self, method)

            def fn(space, inputs, outputs, vector, params, _impl=impl):
                return _impl(space, inputs, outputs, vector, params, prior=prior, noise=noise, *args, **kwargs)
            th_vars = [self.name + '_space_th', self.name + '_inputs_th', self.name + '_outputs_th',
                       self.name + '_vector_th'] + [v.key for v in self.model.vars]
            self.compiles[name] = self.makefn(th_vars, fn, givens=[('space', 'space_th'), ('inputs', 'inputs_th'),
                                                                    ('outputs', 'outputs_th')],
                                              bijection=None, precompile=self.precompile)
        if not array:
            return self.compiles[name]
        flat = 'array_' + name               # same function behind the flat-vector -> dict bijection
        if flat not in self.compiles:
            self.compiles[flat] = self.compiles[name].clone(self.active.bijection.rmap)
        return self.compiles[flat]

    def _call_defaults(self, params, space, inputs, outputs, prior, array):
        """fill in what a caller left out (boundary: stochastic.py:387-402): current parameters (as a
        flat vector when array=True; a supplied dict is cut down to the model's variables), the
        stored space / observations, and the prior when nothing has been observed"""
        if params is None:
            params = self.active.dict_to_array(self.params) if array else self.params
        elif not array:
            params = self.filter_params(params)
        unobserved_call = inputs is None and not self.is_observed
        stored = (self.space, self.inputs, self.outputs)
        space, inputs, outputs = (s if a is None else a for a, s in zip((space, inputs, outputs), stored))
        return params, space, inputs, outputs, (True if unobserved_call else prior)

    @staticmethod
    def _method_name(method=None):
        """public statistic bound to an instance: signature (params, space, inputs, outputs, vector,
        prior, noise, array) as in the reference; resolves defaults, then runs the registry entry"""
        def statistic(self, params=None, space=None, inputs=None, outputs=None, vector=[], prior=False,
                      noise=False, array=False, *args, **kwargs):
            params, space, inputs, outputs, prior = self._call_defaults(params, space, inputs, outputs, prior, array)
            kwargs.pop('simulations', None)   # accepted and unused, as in the reference's th_* methods
            fn = self._compiled(method, prior, noise, array, args, kwargs)
            return fn(params, space, inputs, outputs, vector)
        statistic.__name__ = str(method)
        return statistic

    @property
    def executed(self):
        return {k: v.executed for k, v in self.compiles.items()}

    # ---- predict (boundary: stochastic.py:444-513 -- switches and returned keys)
    # (switch, returned key, method, extra keyword arguments, noise override)
    _PREDICT_TABLE = (
        ('mean', 'mean', 'mean', {}, None),
        ('var', 'variance', 'variance', {}, None),
        ('std', 'std', 'std', {}, None),
        ('cov', 'covariance', 'covariance', {}, None),
        ('median', 'median', 'median', {}, None),
        ('quantiles', 'quantile_up', 'quantiler', {'q': 0.975}, None),
        ('quantiles', 'quantile_down', 'quantiler', {'q': 0.025}, None),
        ('quantiles_noise', 'noise_std', 'std', {}, True),
        ('quantiles_noise', 'noise_up', 'quantiler', {'q': 0.975}, True),
        ('quantiles_noise', 'noise_down', 'quantiler', {'q': 0.025}, True),
    )

    def predict(self, params=None, space=None, inputs=None, outputs=None, mean=True, std=True, var=False,
                cov=False, median=False, quantiles=False, quantiles_noise=False, samples=0, distribution=False,
                prior=False, noise=False, simulations=None):
        params = self.params if params is None else params
        prior = prior or not self.is_observed
        space = self.space if space is None else space
        inputs = self.inputs if inputs is None else inputs
        outputs = self.outputs if outputs is None else outputs
        where = (params, space, inputs, outputs)
        if type(simulations) is int:    # the reference draws them here and then ignores them downstream
            self.sampler(*where, prior=prior, noise=noise, samples=simulations)
        switches = dict(mean=mean, var=var, std=std, cov=cov, median=median, quantiles=quantiles,
                        quantiles_noise=quantiles_noise)
        values = DictObj()
        for switch, key, method, extra, noise_override in self._PREDICT_TABLE:
            if switches[switch]:
                values[key] = getattr(self, method)(*where, prior=prior,
                                                    noise=noise if noise_override is None else noise_override, **extra)
        if samples > 0:
            values['samples'] = self.sampler(*where, samples=samples, prior=prior, noise=noise)
        if distribution:
            def logpredictive(x, _where=where, _prior=prior):
                return self.logpredictive(*_where, vector=x, prior=_prior, noise=True)
            values['logpredictive'] = logpredictive
        return values

    def sample(self, params=None, space=None, inputs=None, outputs=None, samples=1, prior=False, noise=False):
        """draws only (boundary: models.py:443-446)"""
        return self.predict(params=params, space=space, inputs=inputs, outputs=outputs, mean=False, std=False,
                            samples=samples, prior=prior, noise=noise)['samples']

    def scores(self, params=None, space=None, hidden=None, inputs=None, outputs=None, logp=False, logpred=False,
               bias=True, variance=False, median=False, *args, loo=False, **kwargs):
        """scoring harness over mean / variance / median / logpredictive against the hidden truth
        (boundary: models.py:449-469 -- the keys `_l1`, `_l2`, `_mse`, `_rmse`, `_median_l1`,
        `_median_l2`, `_logp`, `_loglike`, `_logprior`, `_nlpd`).  loo=True (keyword only; no counterpart in the reference) adds the
        leave-one-out scores of the OBSERVATIONS from the factor logp already paid for (GaussianProcess.loo): `_loo_nlpd`
        = -logpredictive / N, `_loo_l1` and `_loo_l2`, the mean absolute and squared error of the leave-one-out mean.  cv=folds
        (keyword only, taken from **kwargs so that the signature stays what callers introspect; what GaussianProcess.cv takes as
        `folds`) adds the same three for blocked / k-fold cross-validation
        over the observations held out by some fold: `_cv_nlpd` = -logpredictive / n_held, `_cv_l1` and `_cv_l2`"""
        truth = self.hidden if hidden is None else hidden
        pred = self.predict(params=params, space=space, inputs=inputs, outputs=outputs, mean=True, var=variance,
                            median=median, distribution=logpred)

        def err(which, power):
            return np.mean(np.abs(pred[which] - truth) ** power)
        out = DictObj()
        if bias:
            out.update(_l1=err('mean', 1), _l2=err('mean', 2))
        if variance:
            mse = np.mean((pred.mean - truth) ** 2 + pred.variance)
            out.update(_mse=mse, _rmse=np.sqrt(mse))
        if median:
            out.update(_median_l1=err('median', 1), _median_l2=err('median', 2))
        if logp:
            out.update(_logp=self.logp(params), _loglike=self.loglike(params), _logprior=self.logp(params, prior=True))
        if logpred:
            out['_nlpd'] = -pred.logpredictive(truth) / len(truth)
        if loo:
            if not hasattr(self, 'loo'):
                from .._lib import G3Error
                raise G3Error('leave-one-out scores are not available for %s' % type(self).__name__)
            held = self.loo(params=params, inputs=inputs, outputs=outputs, mean=True, std=False, logpred=True)
            seen = np.asarray(self.outputs if outputs is None else outputs, dtype=self.dtype).reshape(-1)
            out.update(_loo_nlpd=-held.logpredictive / len(seen), _loo_l1=np.mean(np.abs(held.mean - seen)),
                       _loo_l2=np.mean((held.mean - seen) ** 2))
        cv = kwargs.pop('cv', None)
        if cv is not None:
            if not hasattr(self, 'cv'):
                from .._lib import G3Error
                raise G3Error('cross-validation scores are not available for %s' % type(self).__name__)
            held = self.cv(params=params, folds=cv, inputs=inputs, outputs=outputs, mean=True, std=False, logpred=True)
            seen = np.asarray(self.outputs if outputs is None else outputs, dtype=self.dtype).reshape(-1)
            out_of = np.concatenate(held.folds)
            miss = held.mean[out_of] - seen[out_of]
            out.update(_cv_nlpd=-held.logpredictive / len(out_of), _cv_l1=np.mean(np.abs(miss)), _cv_l2=np.mean(miss ** 2))
        return out

    def logp_chain(self, chain, prior=False):
        """stochastic.py:515-520: one logp per row of a flat-parameter chain"""
        return np.array([self.logp(row, array=True, prior=prior) for row in chain], dtype=np.float64)

    # ---- predictions over the rows of a chain (models.py:489-519: a loop of single predictions over an MCMC trace)
    def _chain_rows(self, chain):
        """a 2-D array of flat parameter vectors, or anything with `.values` of that shape (a DataFrame trace)"""
        rows = np.atleast_2d(np.asarray(getattr(chain, 'values', chain), dtype=np.float64))
        return rows[:, :self.active.ndim]

    def _predict_chain_keys(self, switches):
        return [key for switch, key, _, _, _ in self._PREDICT_TABLE if switches.get(switch)]

    def _predict_chain_loop(self, rows, space, inputs, outputs, switches, noise, prior):
        """one `predict` per row, stacked: the route of every process without a batched form of its prediction"""
        out = DictObj()
        for i, row in enumerate(rows):
            pred = self.predict(self.active.array_to_dict(row), space, inputs, outputs, prior=prior, noise=noise, **switches)
            for k, v in pred.items():
                v = np.asarray(v)
                if k not in out:
                    out[k] = np.empty((len(rows),) + v.shape, dtype=v.dtype)
                out[k][i] = v
        if not len(rows):
            M = len(self.space if space is None else space)
            for k in self._predict_chain_keys(switches):
                out[k] = np.empty((0, M), dtype=self.dtype)
        return out

    def _chain_predict_batched(self):
        """True when the process evaluates a block of chain rows in batched launches (GaussianProcess)"""
        return False

    def predict_chain(self, chain, space=None, inputs=None, outputs=None, mean=True, std=True, var=False, median=False,
                      quantiles=False, noise=False, prior=False, batch=None):
        """`predict` for every row of a flat-parameter chain: a DictObj of (rows, M) arrays under predict's keys (mean,
        variance, std, median, quantile_up, quantile_down), row i equal to predict(array_to_dict(chain[i]), ...).  The
        reference loops (models.py:489-519); a GaussianProcess factors and solves `batch` rows at a time in batched
        launches (g3_gp_factor_batched_fields + g3_gp_cross_batched_fields), every other process takes the loop."""
        rows = self._chain_rows(chain)
        switches = dict(mean=mean, std=std, var=var, median=median, quantiles=quantiles)
        prior = prior or not self.is_observed
        if len(rows) and self._chain_predict_batched():
            return self._predict_chain_blocks(rows, space, inputs, outputs, switches, noise, prior, batch)
        return self._predict_chain_loop(rows, space, inputs, outputs, switches, noise, prior)

    def average(self, chain, space=None, inputs=None, outputs=None, mean=True, std=True, var=False, median=False,
                quantiles=False, noise=False, prior=False, batch=None, mixture=False):
        """models.py:489-519 without its `scores`: the arithmetic mean over the rows of a chain (2-D array or anything with
        `.values`) of every curve predict_chain returns.  mixture=True adds the moments of the equal-weight mixture of the
        rows' predictive distributions: mixture_mean = mean of the means, mixture_variance = mean of the variances + the
        (population) variance of the means."""
        pred = self.predict_chain(chain, space, inputs, outputs, mean=mean or mixture, std=std, var=var or mixture,
                                  median=median, quantiles=quantiles, noise=noise, prior=prior, batch=batch)
        wanted = self._predict_chain_keys(dict(mean=mean, std=std, var=var, median=median, quantiles=quantiles))
        out = DictObj()
        for k in wanted:
            out[k] = np.mean(pred[k], axis=0)
        if mixture:
            out['mixture_mean'] = np.mean(pred['mean'], axis=0)
            out['mixture_variance'] = np.mean(pred['variance'], axis=0) + np.var(pred['mean'], axis=0)
        return out

    # ---- draws over the rows of a chain (models.py:521-543: `particles`, a loop of single sampler calls over an MCMC trace)
    def sample_chain(self, chain, space=None, inputs=None, outputs=None, samples=1, prior=False, noise=False, rand=None,
                     batch=None, return_info=False):
        """`sampler` for every row of a flat-parameter chain: (rows, M, samples), row i equal to
        sampler(array_to_dict(chain[i]), ..., samples=samples, rand=rand[i]).  `rand` is (rows, M, samples); by default
        np.random.randn(rows, M, samples), which takes from the global stream what the loop's successive randn(M, samples)
        calls take.  A GaussianProcess draws `batch` rows at a time in batched launches (g3_gp_factor_batched_fields +
        g3_gp_draws_batched_fields), every other process takes the loop.  return_info=True adds a DictObj of per-row
        `tries`, `fallback`, `jitter` of the robust factorisation of the rows' covariances (None where the loop ran)."""
        rows = self._chain_rows(chain)
        prior = prior or not self.is_observed
        space = self.space if space is None else space
        n_rows, M, samples = len(rows), len(space), int(samples)
        if rand is not None:
            rand = np.asarray(rand, dtype=self.dtype)
            if rand.shape != (n_rows, M, samples):
                raise ValueError('rand must have shape (rows, len(space), samples) = %r, got %r'
                                 % ((n_rows, M, samples), rand.shape))
        info = DictObj(tries=None, fallback=None, jitter=None)
        if n_rows and self._chain_predict_batched():
            if rand is None:
                rand = np.asarray(np.random.randn(n_rows, M, samples), dtype=self.dtype)
            out, info['tries'], info['fallback'], info['jitter'] = self._sample_chain_blocks(
                rows, space, inputs, outputs, rand, noise, prior, batch)
        else:
            out = np.empty((n_rows, M, samples), dtype=self.dtype)
            for i, row in enumerate(rows):          # rand None: every sampler call draws its own, in the loop's order
                out[i] = self.sampler(self.active.array_to_dict(row), space, inputs, outputs, samples=samples, prior=prior,
                                      noise=noise, rand=None if rand is None else rand[i])
        return (out, info) if return_info else out

    def particles(self, chain, nsamples=None, *, space=None, inputs=None, outputs=None, samples=1, prior=False, noise=False,
                  rand=None, batch=None):
        """models.py:521-543: one set of `samples` joint draws per row of a chain (2-D array or anything with `.values`),
        cycling over the rows until `nsamples` sets are taken (default: one per row), concatenated along axis 1 to
        (M, nsamples * samples) -- the fully Bayesian predictive: hyper-parameter and function uncertainty together.
        `rand`: (nsamples, M, samples) normals, one slice per set."""
        rows = self._chain_rows(chain)
        nsamples = len(rows) if nsamples is None else int(nsamples)
        M = len(self.space if space is None else space)
        if nsamples < 0 or (nsamples and not len(rows)):
            raise ValueError('particles: %d draws asked of a chain of %d rows' % (nsamples, len(rows)))
        if rand is not None and np.shape(rand) != (nsamples, M, int(samples)):
            raise ValueError('rand must have shape (nsamples, len(space), samples) = %r, got %r'
                             % ((nsamples, M, int(samples)), np.shape(rand)))
        if not nsamples:
            return np.empty((M, 0), dtype=self.dtype)
        picked = rows[np.arange(nsamples) % len(rows)]
        draws = self.sample_chain(picked, space=space, inputs=inputs, outputs=outputs, samples=samples, prior=prior, noise=noise,
                                  rand=rand, batch=batch)
        return np.concatenate(list(draws), axis=1)

    # ---- averages over a fixed chain (stochastic.py:522-564): the rows of active.fixed_chain with
    #      the sampling dimensions overwritten by `sampling_params`
    def _fixed_rows(self, sampling_params):
        if self.active.fixed_chain is None:
            raise ValueError('no fixed chain: call active.fix_vars(datatrace, keys) first')
        self.active.fixed_chain[:, self.active.sampling_dims] = sampling_params
        return self.active.fixed_chain

    def fixed_logp(self, sampling_params, return_array=False):
        r = self.logp_chain(self._fixed_rows(sampling_params))          # one batched sweep where available
        return r if return_array else np.mean(r)

    def fixed_logprior(self, sampling_params, return_array=False):
        r = self.logp_chain(self._fixed_rows(sampling_params), prior=True)
        return r if return_array else np.mean(r)

    def fixed_loglike(self, sampling_params, return_array=False):
        rows = self._fixed_rows(sampling_params)
        r = self.logp_chain(rows) - self.logp_chain(rows, prior=True)
        return r if return_array else np.mean(r)

    def fixed_dlogp(self, sampling_params, return_array=False):
        rows = self._fixed_rows(sampling_params)
        if hasattr(self, 'dlogp_chain'):      # one batched factor + K^-1 sweep where the process provides it
            r = np.asarray(self.dlogp_chain(rows))[:, self.active.sampling_dims]
        else:
            r = np.array([self.dlogp(p, array=True)[self.active.sampling_dims] for p in rows])
        return r if return_array else np.mean(r, axis=0)
