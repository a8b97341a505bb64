"""LSX_DPOPS_COL after a statistical equilibrium or an implicit step is, bit for bit, the maximum over the column's solved
systems of |1 - n_old / n_new| (NaN dropped) formed in float64 from the populations before and after the call: a division and
a subtraction that round once each, on the device as in numpy.  The kernels take that maximum with one atomic per run of a
wave's lanes that hold the same column (lsx_solve_flag.h: column_max), so the shapes put into one wave: a single short column
(1 x 3), columns of 5 depths (twelve runs and a cut one), of 13 (runs that straddle waves), 82 depths (one or two runs), beside
a refused system in the middle of a run, a frozen column between two active ones, and both register and LDS kernels."""
import numpy as np
import pytest

import se_cases
import td_cases
from lightspinner_amd import _capi
from lightspinner_amd.problem import Engine
from se_cases import probe_problem

pytestmark = pytest.mark.gpu


def expected(n_old, n_new, skip=()):
    """[ncol]: max over levels and depths of |1 - n_old / n_new|, NaN dropped, the systems (col, level slice, depth) of skip left out"""
    with np.errstate(all='ignore'):
        ch = np.abs(1.0 - n_old / n_new)
    for c, lv, k in skip:
        ch[c, lv, k] = 0.0
    return np.fmax.reduce(np.fmax.reduce(np.where(np.isnan(ch), 0.0, ch), axis=2), axis=1)


def probes(nls, Ns, nc, seed):
    prob, block, atoms = probe_problem(list(nls), Ns, nc)
    for q, a in enumerate(atoms):
        se_cases.family_inputs(('rate_scale', 'ties')[q % 2], prob, block, a, seed=seed + q)
    return prob, block, atoms


@pytest.mark.parametrize('options', [None, 'se_lds=1'])
@pytest.mark.parametrize('shape', [(3, 1), (5, 37), (13, 5), (82, 3)])
def test_monitor_is_the_maximum_over_the_columns_systems(hip_lib, shape, options):
    Ns, nc = shape
    prob, block, _ = probes([6, 9, 2], Ns, nc, seed=40 + Ns)
    e, G, n_old, n_new, dPcol, dP = se_cases.run(hip_lib, prob, block, options=options)
    e.close()
    want = expected(n_old, n_new)
    assert np.all(want > 0.0)
    assert np.array_equal(dPcol.view(np.uint64), want.view(np.uint64))
    assert dP == want.max()


def test_a_refused_system_in_the_middle_of_a_run_and_a_frozen_column(hip_lib):
    Ns, nc = 13, 5
    prob, block, (a, b) = probes([5, 8], Ns, nc, seed=500)
    Ca = se_cases.rates_of(prob, block.C, a).copy()
    Ca[2, :, :, 7] = 0.0
    se_cases.put(prob, block, a, C=Ca)
    active = np.ones(nc, dtype=bool)
    active[3] = False
    e = Engine(prob, nc, lib=hip_lib)
    e.set_columns(0, block)
    e.set_active_columns(active)
    e.formal_sol_gamma()
    n_old = e.get(_capi.LSX_N)
    se_cases.expect_singular(e, 'sync', 2, 7, a)
    n_new, dPcol = e.get(_capi.LSX_N), e.get(_capi.LSX_DPOPS_COL)
    e.close()
    lv = slice(prob.lev_off[a], prob.lev_off[a] + 5)
    assert np.array_equal(n_new[2, lv, 7].view(np.uint64), n_old[2, lv, 7].view(np.uint64))
    assert np.array_equal(n_new[3].view(np.uint64), n_old[3].view(np.uint64))
    want = expected(n_old, n_new, skip=[(2, lv, 7)])
    assert want[3] == 0.0 and np.all(want[[0, 1, 2, 4]] > 0.0)
    assert np.array_equal(dPcol.view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize('Nl', [3, 9])
def test_monitor_of_the_implicit_step(hip_lib, Nl):
    Ns, nc = td_cases.SHAPES[1]
    prob, block, (a,) = probe_problem([Nl], Ns, nc)
    dt = td_cases.column_dt(nc)
    prev_a, _ = td_cases.family_inputs('rate_scale', prob, block, a, 700 + Nl, dt)
    n_prev = td_cases.full_n_prev(prob, block, a, prev_a)
    G, n_old, n_new, dPcol = td_cases.HipRunner(hip_lib)(prob, block, dt, n_prev)
    want = expected(n_old, n_new)
    assert np.all(want > 0.0) and np.array_equal(dPcol.view(np.uint64), want.view(np.uint64))
