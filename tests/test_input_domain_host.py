"""The conditions tests/test_gpu_input_domain.py rests on, checked without a GPU (inputs, truth and tolerance live in
tests/input_domain.py):

  * U + c is exact in the working type for every case, so the extended-precision covariance of U is the exact
    covariance of X = U + c;
  * the yardstick -- the reference's direct formula in the working type on X -- stays within
    64 eps (1 + 2 pi sum_k f_k span_k) max|truth| of that truth: it is not loose, its error follows the SPAN of the inputs
    and not their distance from the origin;
  * the tolerance separates the defect from a correct kernel: a NumPy emulation of per-tile [cos, sin] tables of
    theta = 2 pi f x in the working type misses it at every offset case; the same tables of theta = 2 pi f (x - x0),
    x0 the first column point of the tile, stay within it for a bare COS leaf; tables of theta modulo 2 pi from the exact
    product f x, which is what the kernels build, stay within it for every case and kernel tried."""
import numpy as np
import pytest

import input_domain as idm


@pytest.mark.parametrize('case', sorted(idm.CASES))
def test_offsets_are_exact_in_the_working_type(case):
    assert idm.offsets_exact(case)
    U, Us, X, Xs = idm.inputs(case)
    T, d, grid, span, c = idm.CASES[case]
    assert X.shape == (idm.N, d) and Xs.shape == (idm.M, d) and X.dtype == T
    assert U.min() >= 0 and U.max() < span and np.array_equal(U / grid, np.round(U / grid))


@pytest.mark.parametrize('case', sorted(idm.CASES))
def test_the_direct_formula_in_the_working_type_is_a_tight_yardstick(case):
    for name in idm.kernels(case):
        for cross in (False, True):
            ye, bound = idm.yard_err(case, name, cross), idm.yard_bound(case, name, cross)
            print('%-12s %-20s %-5s |yard - truth| %.3e  bound %.3e  tol %.3e' %
                  (case, name, 'cross' if cross else 'sym', ye, bound, idm.tol(case, name, cross)))
            assert ye <= bound, (case, name, cross, ye, bound)


@pytest.mark.parametrize('local', [False, True], ids=['COS', 'SE*COS'])
@pytest.mark.parametrize('cross', [False, True], ids=['sym', 'cross'])
@pytest.mark.parametrize('case', sorted(idm.CASES))
def test_the_tolerance_separates_the_ways_to_form_theta(case, cross, local):
    """per-tile [cos, sin] tables emulated in the working type, for the bare COS leaf and for the locally periodic SE * COS:
    theta as a plain product of x misses the tolerance at every offset case; measured from a point of the tile it stays
    within it for the bare COS leaf, whose own direct formula is as wrong at large distances -- but not for SE * COS on the
    time series, whose large entries sit on close pairs while the tile spans 64 periods; taken modulo 2 pi from the exact
    product it stays within the tolerance everywhere"""
    tr, ye, tol = idm.probe_truth(case, cross, local)
    e = {m: float(np.abs(idm.table_emulation(case, m, cross, local).astype(np.longdouble) - tr).max())
         for m in ('origin', 'tile', 'exact')}
    print('%-12s %-6s %-5s direct %.3e  table: origin %.3e  tile %.3e  exact %.3e  tol %.3e' %
          (case, 'SE*COS' if local else 'COS', 'cross' if cross else 'sym', ye, e['origin'], e['tile'], e['exact'], tol))
    assert e['exact'] <= tol, (case, e, tol)
    if case in idm.OFFSET_CASES:
        assert e['origin'] > tol, (case, e, tol)
    years = idm.case_d(case) == 1
    if not local:
        assert e['tile'] <= tol, (case, e, tol)
        if not years and case not in idm.OFFSET_CASES:
            assert e['origin'] <= tol, (case, e, tol)
    elif years:
        assert e['tile'] > tol, (case, e, tol)
