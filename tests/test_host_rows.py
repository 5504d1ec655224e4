"""The host-side formulas of g3py_amd/processes/ -- mappings, means, Freedom, _values, the densities and the chain rule
of dlogp -- against tests/golden/host_rows.npz, which oracle/gen_host_rows.py recorded from the commit that still held
every formula twice (a one-row form and a hand-vectorised `*_rows` form).  Each formula is now written once and serves
both; it must give what BOTH recorded forms gave, byte for byte wherever the arithmetic is element-wise or a sum over the
last axis.  No device."""
import numpy as np
import pytest

from oracle import gen_host_rows as gen

N, B = gen.N, gen.B
TAGS = [pytest.param(tag, dtype, id=tag) for tag, dtype in gen.DTYPES]


@pytest.fixture(scope='module')
def fx():
    return gen.load()


@pytest.fixture(scope='module')
def inp():
    return gen.inputs()


def same(got, want, what):
    got = np.asarray(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_array_equal(got, want, err_msg=str(what))          # (NaNs in the same places count as equal)


def within(got, want, bound, what):
    """|got - want| <= bound element-wise; where the recorded value is not finite, the same non-finite value"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    fin = np.isfinite(want)
    np.testing.assert_array_equal(got[~fin], want[~fin], err_msg=str(what))
    bound = np.broadcast_to(bound, want.shape)
    assert np.all(np.abs(got - want)[fin] <= bound[fin]), (what, np.abs(got - want)[fin].max(), bound[fin].min())


def grads_one(m, y, vr):
    per = [m.grad(y, gen.row(vr, j)) for j in range(B)]
    return [(np.stack([np.broadcast_to(p[i][1], y.shape) for p in per]), np.array([p[i][2] for p in per]))
            for i in range(len(per[0]))]


@pytest.mark.parametrize('tag, dtype', TAGS)
def test_mappings_give_both_recorded_forms(fx, inp, tag, dtype):
    """every built-in mapping: `__call__`, `inv`, `logdet_dinv`, `grad` row by row, and `inv_rows`, `logdet_dinv_rows`,
    `grad_rows` (and `__call__` on Rows values) over B = 7 rows, each against the recorded one-row AND the recorded rows
    form.  BoxCoxLinear has rows on both sides of its power < 1e-5 switch and a negative `shifted` entry (NaN in the log
    branch), LogShifted a row with shift > min(y)."""
    y, x = inp['y'].astype(dtype), inp['x'].astype(dtype)
    with np.errstate(all='ignore'):
        for name, (m, vr) in gen.mapping_cases().items():
            assert m.BROADCASTS
            k = '%s/map/%s/' % (tag, name)
            same(np.broadcast_to(m(x, vr), (B, N)), fx[k + 'call_one'], k + 'call on Rows')
            same(np.stack([np.broadcast_to(m(x, gen.row(vr, j)), (N,)) for j in range(B)]), fx[k + 'call_one'], k + 'call')
            inv_one = np.stack([np.asarray(m.inv(y, gen.row(vr, j)), dtype=dtype) for j in range(B)])
            det_one = np.array([m.logdet_dinv(y, gen.row(vr, j)) for j in range(B)], dtype=dtype)
            g_one, g_rows = grads_one(m, y, vr), m.grad_rows(y, vr, B)
            assert len(g_rows) == len(g_one) == len(m.hypers)
            for form in ('one', 'rows'):
                same(inv_one, fx[k + 'inv_' + form], k + 'inv / ' + form)
                same(m.inv_rows(y, vr, B), fx[k + 'inv_' + form], k + 'inv_rows / ' + form)
                same(det_one, fx[k + 'logdet_' + form], k + 'logdet_dinv / ' + form)
                same(m.logdet_dinv_rows(y, vr, B), fx[k + 'logdet_' + form], k + 'logdet_dinv_rows / ' + form)
                for i in range(len(g_rows)):
                    want = fx[k + 'grad_%s/%d/dinv' % (form, i)], fx[k + 'grad_%s/%d/dlogdet' % (form, i)]
                    for got, label in ((g_one[i], 'grad'), (g_rows[i][1:], 'grad_rows')):
                        same(got[0], want[0], (k, label, form, i, 'dinv'))
                        same(got[1], want[1], (k, label, form, i, 'dlogdet'))


@pytest.mark.parametrize('tag, dtype', TAGS)
def test_means_and_freedom_give_both_recorded_forms(fx, inp, tag, dtype):
    """every built-in mean on 3 columns (Linear with a per-column coeff): `__call__` row by row and `rows`, both against
    the recorded loop and the recorded rows form; `grad` against the recorded Jacobians; Freedom() and Freedom.rows.
    Linear's three-term dot product was recorded from np.dot (one row) and np.matmul (rows) and is np.matmul in both now:
    the record's two forms agree byte for byte, and so does this on the BLAS builds tried, but NumPy promises that of no
    two routines -- if only `Linear` fails here on another BLAS, compare within 2 * 3 * eps * |x| . |coeff| first."""
    X = inp['X'].astype(dtype)
    for name, (m, vr) in gen.mean_cases().items():
        assert m.BROADCASTS and m.JAC_CONSTANT
        k = '%s/mean/%s/' % (tag, name)
        one = np.stack([m(X, gen.row(vr, j)) for j in range(B)])
        for want in (fx[k + 'call_one'], fx[k + 'rows']):
            same(one, want, k + 'call')
            same(m.rows(X, vr, B), want, k + 'rows')
        per = [m.grad(X, gen.row(vr, j)) for j in range(B)]
        for i in range(len(per[0])):
            same(np.stack([p[i][1] for p in per]), fx[k + 'grad_one/%d' % i], k + 'grad')
    f, fr = gen.freedom_case()
    for want in (fx[tag + '/freedom/one'], fx[tag + '/freedom/rows']):
        same(np.array([f(gen.row(fr, j)) for j in range(B)]), want, 'Freedom()')
        same(f.rows(fr, B), want, 'Freedom.rows')


def test_values_give_both_recorded_forms(fx):
    """_values and _values_rows on the three processes of test_chain_rows_packing_equals_row_by_row: the natural-space
    values and the extra logp terms (the -inf Jacobian term of the underflowing row, the L2 potential)"""
    for i, (gp, chain) in enumerate(gen.packing_cases()):
        k = 'values/%d/' % i
        same(chain, fx[k + 'chain'], 'the chain itself')
        vb, lj = gp._values_rows(chain)
        per = []
        for j in range(B):
            gp._values_memo = None
            per.append(gp._values(gp.active.array_to_dict(chain[j])))
        assert np.isneginf(fx[k + 'logjac_one'][2])
        for form in ('one', 'rows'):
            same(lj, fx[k + 'logjac_' + form], k + 'logjac rows / ' + form)
            same(np.array([q[1] for q in per]), fx[k + 'logjac_' + form], k + 'logjac one / ' + form)
            for name in vb:
                same(vb[name], fx[k + form + '/' + name], (k, name, form))
                same(np.stack([np.asarray(q[0][name]) for q in per]), fx[k + form + '/' + name], (k, name, form))
        params = gp.active.array_to_dict(chain[0])
        assert gp._values(params)[0] is gp._values(params)[0]              # the memo on the params object


@pytest.mark.parametrize('tag, dtype', TAGS)
def test_diagonal_density_one_body(fx, inp, tag, dtype):
    """logp_cho_diag and loo_assemble (one and two dimensions) on a Box-Cox warp, rows with a NaN sd or a NaN delta on the
    sentinel.  The rows form and every curve are byte-equal to the record.  The ONE-ROW log density summed its squares
    with BLAS (lcho.dot(lcho)) where the rows form, and now the one body, sums over the last axis: two N-term sums of the
    same products, each within N eps sum(lcho^2) of the exact sum, so they differ by at most 2 N eps (1/2 sum lcho^2) in
    the quadratic term, plus one rounding (eps |r|) in each of the three additions that follow it."""
    from g3py_amd.processes.gaussian import logp_cho_diag, loo_assemble, SENTINEL
    from g3py_amd.libs.tensors import to_num
    t = np.dtype(dtype).type
    eps = np.finfo(dtype).eps
    y, alpha, kdiag = inp['y'].astype(dtype), inp['alpha'].astype(dtype), inp['kdiag'].astype(dtype)
    m, vr = gen.mapping_cases()['BoxCoxLinear']
    with np.errstate(all='ignore'):
        z = np.asarray(m.inv_rows(y, vr, B), dtype=dtype)
        zs = to_num(z, dtype)
        loc, sd = z - alpha / kdiag, t(1) / np.sqrt(kdiag)
        quad = 0.5 * ((((z - loc) / sd).astype(np.float64)) ** 2).sum(axis=1)
    k = tag + '/diag/'
    rows = loo_assemble(alpha, kdiag, z, m, vr, y=y, dtype=dtype)['logpredictive']
    same(rows, fx[k + 'loo_rows/logpredictive'], 'loo_assemble, two dimensions')
    sentinel = fx[k + 'logp_cho_diag_one'] == t(SENTINEL)
    assert 1 <= sentinel.sum() < B and np.array_equal(sentinel, rows == t(SENTINEL))
    bound = np.where(sentinel, 0.0, 2 * N * eps * quad + 3 * eps * np.abs(fx[k + 'logp_cho_diag_one'].astype(np.float64)))
    one = np.array([logp_cho_diag(y, loc[j], sd[j], m, gen.row(vr, j), dtype) for j in range(B)])
    assert one.dtype == np.dtype(dtype)
    within(one, fx[k + 'logp_cho_diag_one'], bound, 'logp_cho_diag')
    same(one, rows, 'one row against B rows, current code')
    for hermite in (None, 10):
        per = [loo_assemble(alpha[j], kdiag[j], zs[j], m, gen.row(vr, j), y=y, dtype=dtype, hermite=hermite, var=True, median=True)
               for j in range(B)]
        for key in ('mean', 'variance', 'std', 'median'):
            same(np.stack([p[key] for p in per]), fx[k + 'loo_one/%s/%s' % (hermite, key)], ('loo_assemble', hermite, key))
        lp = fx[k + 'loo_one/%s/logpredictive' % hermite]
        within(np.array([p['logpredictive'] for p in per]), lp, np.where(lp == t(SENTINEL), 0.0, 2 * N * eps * np.nan_to_num(quad)
                                                                         + 3 * eps * np.abs(lp.astype(np.float64))), 'loo one row')


@pytest.mark.parametrize('tag, dtype', TAGS)
def test_factor_densities_one_body(fx, inp, tag, dtype):
    """the Gaussian and the Student-t density of the factor's scalars (logdet, quad, det_m): `_density` on (B,) arrays
    against the recorded _chain_density, and on scalars row by row against the recorded arithmetic of th_loglike; the
    Student-t rows sit on both sides of nu = 1e6 and on it"""
    cases = gen.gradient_cases(dtype)
    st, det_m = inp['st'], inp['det_m'].astype(dtype)
    f, fr = gen.freedom_case()
    nu = np.asarray(f.rows(fr, B))
    assert (nu < 1e6).any() and (nu == 1e6).any() and (nu > 1e6).any()
    with np.errstate(all='ignore'):
        for name, p, nus in (('gauss', cases['wgp'][0], [None] * B), ('student', cases['tp'][0], nu)):
            k = '%s/density/%s/' % (tag, name)
            rows = np.asarray(p._density(st[:, 0], st[:, 1], det_m, N, None if name == 'gauss' else nu))
            one = np.array([p._density(st[j, 0], st[j, 1], det_m[j], N, nus[j]) for j in range(B)])
            assert rows.dtype == one.dtype == np.dtype(dtype)
            for got in (rows, one):
                same(got, fx[k + 'rows'], k + 'rows')
                same(got, fx[k + 'one'], k + 'one')


def nat_of(fx, key, names, j=None):
    return {n: (fx[key + '/' + n] if j is None else fx[key + '/' + n][j]) for n in names}


@pytest.mark.parametrize('tag, dtype', TAGS)
@pytest.mark.parametrize('which', ['wgp', 'tp'])
def test_gradient_stages_one_body(fx, inp, tag, dtype, which):
    """dlogp's host side stage by stage -- _potential_gradient, _dlogp_scale, _chain_rule, _flat_gradient -- on a
    WGP(BoxCoxLinear, Linear, SE + RQ, L2 potential) and a StudentTProcess with synthetic device results (slots, alpha,
    quad; two rows not ok): each stage starts from the recorded input of that stage and is compared with the recorded
    one-row form (row by row) and the recorded rows form.  Byte-equal, except the alpha . J terms of the location and
    warping hypers: a one-row and a B-row call may take different BLAS routes (and the one-row warping term was a BLAS
    dot, now a last-axis sum), so those get the forward error bound of an N-term dot product, taken twice:
    2 N eps(dtype) sum_i |alpha_i| |J_i|."""
    p, chain, X, y = gen.gradient_cases(dtype)[which]
    k = '%s/grad/%s/' % (tag, which)
    same(chain, fx[k + 'chain'], 'the chain itself')
    st, ok, alphas, slots = inp['st'], inp['ok'], inp['alpha'], fx[k + 'slots']
    d = X.shape[1]
    vb, _ = p._values_rows(chain)
    prog, gmap, nslots = gen.program(p, p._values_row(vb, 0), d)
    assert slots.shape == (B, nslots) and not ok.all()
    names = [v.name for v in p.model.vars]
    eps = np.finfo(dtype).eps
    # what the bound needs: |alpha| . |J| per hyper, from the Jacobians tested above
    bound = {n: 0.0 for n in names}
    a_ok = np.abs(np.where(ok[:, None], alphas, 0.0))
    for h, J in p.f_location.grad(X, p._values_row(vb, 0)):
        b = a_ok.dot(np.abs(np.asarray(J, dtype=np.float64)))
        bound[h.name] = 2 * N * eps * (b if h.shape else b.sum(axis=1))
    with np.errstate(all='ignore'):
        for h, dinv, _ in p.f_mapping.grad_rows(y, vb, B):
            bound[h.name] = 2 * N * eps * (a_ok * np.abs(np.asarray(dinv, dtype=np.float64))).sum(axis=1)
    loose = {n for n in names if np.any(np.asarray(bound[n]) > 0)}
    assert loose == {h.name for h in list(p.f_location.hypers) + list(p.f_mapping.hypers)}

    def compare(nat, want_key, j=None, stage=''):
        for n in names:
            want = fx[want_key + '/' + n] if j is None else fx[want_key + '/' + n][j]
            if stage == 'rule' and n in loose:
                bd = np.asarray(bound[n]) if j is None else np.asarray(bound[n])[j]
                within(nat[n], want, np.reshape(bd, np.shape(want)), (want_key, n, j))
            else:
                same(nat[n], want, (want_key, n, j))

    # ---- the B rows at once
    nat = p._potential_gradient(vb, B)
    compare(nat, k + 'pot_rows')
    nat = nat_of(fx, k + 'pot_rows', names)
    s = p._dlogp_scale(p._nu(vb, B), st[:, 1], N, nat, ok)
    same(np.ones(B) if s is None else s, fx[k + 's_rows'], 's rows')
    assert (s is None) == (which == 'wgp')
    compare(nat, k + 'scale_rows')
    nat = nat_of(fx, k + 'scale_rows', names)
    p._chain_rule(vb, X, y, nat, prog, gmap, slots, alphas, d, ok)
    compare(nat, k + 'rule_rows', stage='rule')
    same(p._flat_gradient(vb, nat_of(fx, k + 'rule_rows', names), B), fx[k + 'flat_rows'], 'flat rows')
    # ---- row by row, as th_dlogp / _dloglike do: the likelihood terms only where logp is not the sentinel
    for j in range(B):
        vj = p._values_row(vb, j)
        nat = p._potential_gradient(vj)
        compare(nat, k + 'pot_one', j)
        compare(nat, k + 'pot_rows', j)
        if ok[j]:
            nat = nat_of(fx, k + 'pot_one', names, j)
            s = p._dlogp_scale(p._nu(vj), st[j, 1], N, nat)
            for form in ('one', 'rows'):
                same(1.0 if s is None else s, fx[k + 's_' + form][j], 's one row')
                compare(nat, k + 'scale_' + form, j)
            nat = nat_of(fx, k + 'scale_one', names, j)
            with np.errstate(all='ignore'):
                p._chain_rule(vj, X, y, nat, prog, gmap, slots[j], alphas[j], d)
            compare(nat, k + 'rule_one', j, stage='rule')
            compare(nat, k + 'rule_rows', j, stage='rule')
        for form in ('one', 'rows'):
            same(p._flat_gradient(vj, nat_of(fx, k + 'rule_' + form, names, j)), fx[k + 'flat_' + form][j], ('flat', form, j))


@pytest.mark.parametrize('tag, dtype', TAGS)
def test_one_row_equals_rows_on_the_current_code(inp, tag, dtype):
    """row j of every `*_rows` result against the one-row call on row j, byte for byte, all built-in mappings and means;
    BoxCoxLinear's power is exactly 0.5 and 2.0 on two rows, where NumPy would take sqrt / square for a scalar exponent
    and pow for an array of them (mappings._power hands it an array in both forms)"""
    y, x, X = inp['y'].astype(dtype), inp['x'].astype(dtype), inp['X'].astype(dtype)
    cases = gen.mapping_cases(special_powers=True)
    power = np.asarray(cases['BoxCoxLinear'][1]['P_BoxCoxLinear_power'])
    assert power[1] == 0.5 and power[4] == 2.0
    with np.errstate(all='ignore'):
        for name, (m, vr) in cases.items():
            same(np.broadcast_to(m(x, vr), (B, N)), np.stack([np.broadcast_to(m(x, gen.row(vr, j)), (N,)) for j in range(B)]), name)
            same(m.inv_rows(y, vr, B), np.stack([np.asarray(m.inv(y, gen.row(vr, j)), dtype=dtype) for j in range(B)]), name)
            same(m.logdet_dinv_rows(y, vr, B), np.array([m.logdet_dinv(y, gen.row(vr, j)) for j in range(B)], dtype=dtype), name)
            for (h, dinv, dlogdet), (dinv1, dlogdet1) in zip(m.grad_rows(y, vr, B), grads_one(m, y, vr)):
                same(dinv, dinv1, (name, h, 'dinv'))
                same(dlogdet, dlogdet1, (name, h, 'dlogdet'))
    for name, (m, vr) in gen.mean_cases().items():
        same(m.rows(X, vr, B), np.stack([m(X, gen.row(vr, j)) for j in range(B)]), name)


@pytest.mark.parametrize('tag, dtype', TAGS)
def test_row_forms_over_several_row_blocks(tag, dtype):
    """the `*_rows` forms evaluate a mapping's formula on blocks of rows (hypers.row_blocks: 8192 // N rows each); with
    N = 3000 observations the B = 7 rows fall into blocks of 2, 2, 2 and 1, and every row still equals its one-row call"""
    from g3py_amd.processes.hypers import row_blocks
    n = 3000
    y = np.random.default_rng(5).uniform(0.5, 3.0, n).astype(dtype)
    y[3] = 0.2
    cases = gen.mapping_cases(special_powers=True)
    assert [hi - lo for lo, hi, _ in row_blocks(cases['BoxCoxLinear'][1], B, n)] == [2, 2, 2, 1]
    with np.errstate(all='ignore'):
        for name, (m, vr) in cases.items():
            same(m.inv_rows(y, vr, B), np.stack([np.asarray(m.inv(y, gen.row(vr, j)), dtype=dtype) for j in range(B)]), name)
            same(m.logdet_dinv_rows(y, vr, B), np.array([m.logdet_dinv(y, gen.row(vr, j)) for j in range(B)], dtype=dtype), name)
            for (h, dinv, dlogdet), (dinv1, dlogdet1) in zip(m.grad_rows(y, vr, B), grads_one(m, y, vr)):
                same(dinv, dinv1, (name, h, 'dinv'))
                same(dlogdet, dlogdet1, (name, h, 'dlogdet'))


def constant_slot_cases():
    """mappings, means and a Freedom with some slots given as constants (Hypers.__init__ takes them, value_of returns them):
    the constant has no row axis, so an expression may get its (B, ...) shape from the free slots alone"""
    import g3py_amd as g3
    from g3py_amd.processes.hypers import Freedom, Model
    rng = np.random.default_rng(9)
    X = gen.inputs()['X']
    power = np.array([1e-6, 0.5, 1.0, 3e-6, 2.0, 0.8, 2.5])
    shift = np.array([0.5, -0.3, 1.0, -0.3, 0.0, 2.0, 0.7])
    scale = np.exp(0.3 * rng.standard_normal(B))
    with Model('host_rows_constants'):
        maps = [(g3.BoxCoxLinear(name='BCa', shift=1.0, scale=1.0), {'P_BCa_power': power}),
                (g3.BoxCoxLinear(name='BCb', shift=-0.3, scale=1.3), {'P_BCb_power': power}),
                (g3.BoxCoxLinear(name='BCc', power=0.5), {'P_BCc_shift': shift, 'P_BCc_scale': scale}),
                (g3.BoxCoxLinear(name='BCd', scale=0.8, power=3e-6), {'P_BCd_shift': shift}),
                (g3.LinearMapping(name='LMa', shift=0.2), {'P_LMa_scale': scale}),
                (g3.LinearMapping(name='LMb', scale=1.7), {'P_LMb_shift': shift}),
                (g3.ArcsinhLinear(name='ASa', scale=1.5), {'P_ASa_shift': shift}),
                (g3.ArcsinhLinear(name='ASb', shift=0.4), {'P_ASb_scale': scale}),
                (g3.LogShifted(name='LSa', shift=-0.5), {})]
        means = [(g3.Linear(X, name='La', constant=0.3), {'P_La_Coeff': rng.standard_normal((B, X.shape[1]))}),
                 (g3.Linear(X, name='Lb', coeff=np.array([0.5, -1.0, 2.0])), {'P_Lb_Constant': rng.standard_normal(B)}),
                 (g3.Linear(X, name='Lc', constant=-1.0, coeff=0.25), {}),
                 (g3.Bias(X, name='Ba', bias=0.6), {})]
        free = [(Freedom(name='Fa', degree=5.0), {}), (Freedom(name='Fb'), {'P_Fb_degree': np.array([1.5, 10.0, 1e3, 1e6, 2e6, 3.0, 7.0])})]
        for h, v in maps + means + free:
            h.check_dims(None)
            h.check_hypers('P_')
            assert set(v) == {s.name for s in h.hypers if hasattr(s, 'name')}, (h.name, h.hypers)
    rows = lambda cases: [(h, {k: gen.as_rows(a) for k, a in v.items()}) for h, v in cases]
    return rows(maps), rows(means), rows(free)


@pytest.mark.parametrize('tag, dtype', TAGS)
def test_one_row_equals_rows_with_slots_given_as_constants(inp, tag, dtype):
    """the comparison above where some (or all) of a function's slots are constants, not free hypers -- for example
    BoxCoxLinear(shift=1.0, scale=1.0) with only its power free, at exactly 0.5 and 2.0 and below 1e-5 among the rows:
    `*_rows`, `rows` and Freedom.rows give (B, ...) results whose row j is the one-row call on row j, byte for byte"""
    y, x, X = inp['y'].astype(dtype), inp['x'].astype(dtype), inp['X'].astype(dtype)
    maps, means, free = constant_slot_cases()
    with np.errstate(all='ignore'):
        for m, vr in maps:
            assert m.BROADCASTS and len(vr) < len(m.SLOTS)
            same(np.broadcast_to(m(x, vr), (B, N)), np.stack([np.broadcast_to(m(x, gen.row(vr, j)), (N,)) for j in range(B)]), m.name)
            same(m.inv_rows(y, vr, B), np.stack([np.asarray(m.inv(y, gen.row(vr, j)), dtype=dtype) for j in range(B)]), m.name)
            same(m.logdet_dinv_rows(y, vr, B), np.array([m.logdet_dinv(y, gen.row(vr, j)) for j in range(B)], dtype=dtype), m.name)
            g_rows = m.grad_rows(y, vr, B)
            assert len(g_rows) == len(m.SLOTS)
            for (h, dinv, dlogdet), (dinv1, dlogdet1) in zip(g_rows, grads_one(m, y, vr)):
                same(dinv, dinv1, (m.name, h, 'dinv'))
                same(dlogdet, dlogdet1, (m.name, h, 'dlogdet'))
    for m, vr in means:
        same(m.rows(X, vr, B), np.stack([m(X, gen.row(vr, j)) for j in range(B)]), m.name)
    for f, vr in free:
        same(f.rows(vr, B), np.array([f(gen.row(vr, j)) for j in range(B)]), f.name)


def test_user_defined_one_row_classes_take_the_row_loop(inp):
    """a Mapping and a Mean that implement only the one-row methods (plain value_of, scalar branches) and have not
    declared BROADCASTS still serve inv_rows / logdet_dinv_rows / grad_rows / rows: row by row, with a loop's values"""
    from g3py_amd.processes.hypers import Model, Slot, value_of
    from g3py_amd.processes.hypers.mappings import Mapping
    from g3py_amd.processes.hypers.means import Mean

    class Cubic(Mapping):
        SLOTS = (Slot('scale', True, '_scale'),)

        def inv(self, y, values=None):
            s = float(value_of(self.scale, values))
            return y ** 3 * s if s > 1 else y ** 3 / s

        def logdet_dinv(self, y, values=None):
            s = float(value_of(self.scale, values))
            return float(np.sum(np.log(3 * y ** 2)) + (1 if s > 1 else -1) * len(y) * np.log(s))

        def grad(self, y, values=None):
            s = float(value_of(self.scale, values))
            return [(self.scale, y ** 3 if s > 1 else -y ** 3 / s ** 2, (1 if s > 1 else -1) * len(y) / s)]

    class Bump(Mean):
        SLOTS = (Slot('centre', False, '_centre'),)

        def eval(self, x, values):
            return np.exp(-(x[:, 0] - float(value_of(self.centre, values))) ** 2)

    y, X = inp['y'], inp['X']
    with Model('user_defined'):
        m, mu = Cubic(name='Cubic'), Bump(X, name='Bump')
        m.check_hypers('P_')
        mu.check_hypers('P_')
    assert not m.BROADCASTS and not mu.BROADCASTS and not mu.JAC_CONSTANT
    vr = {'P_Cubic_scale': gen.as_rows([0.5, 2.0, 1.5, 0.9, 3.0, 0.2, 1.1]), 'P_Bump_centre': gen.as_rows(np.linspace(0, 5, B))}
    same(m.inv_rows(y, vr, B), np.stack([m.inv(y, gen.row(vr, j)) for j in range(B)]), 'inv_rows')
    same(m.logdet_dinv_rows(y, vr, B), np.array([m.logdet_dinv(y, gen.row(vr, j)) for j in range(B)]), 'logdet_dinv_rows')
    (h, dinv, dlogdet), = m.grad_rows(y, vr, B)
    assert h is m.scale
    same(dinv, np.stack([m.grad(y, gen.row(vr, j))[0][1] for j in range(B)]), 'grad_rows dinv')
    same(dlogdet, np.array([m.grad(y, gen.row(vr, j))[0][2] for j in range(B)]), 'grad_rows dlogdet')
    same(mu.rows(X, vr, B), np.stack([mu(X, gen.row(vr, j)) for j in range(B)]), 'Mean.rows')
