"""The HIP kernels against the reference's OWN loop on every made-up topology (tests/topology_cases.py), through the fixture
tests/golden/topologies_*.npz (tests/golden/make_topology_golden.py: the unmodified formal_sol_gamma_matrices / stat_equil,
rh_method.py:565-745, on the arrays the library is given).  The whole batch of a case runs on the GPU; its golden columns (the first
and the last: the ragged last group of the ray-serial wavefronts) are compared with the fixture under the bars of
tests/topology_reference.py, the ones tests/test_topologies_reference_host.py holds the oracle to.  The fixture is all that is read.

Batches of >= 32 columns run on both sweep mappings where the shape has ray-serial kernels (one launch per tile class), smaller
ones through the fused launch.  Only the linear rule: the reference has no parabolic rule, which stays HIP against the oracle
(tests/test_toy_topologies.py, tests/test_instances_gpu.py)."""
import numpy as np
import pytest

import instance_cases as ic
import topology_cases as tc
import topology_reference as tr
from test_instances_gpu import classes_run
from lightspinner_amd import _capi
from lightspinner_amd.problem import Engine

pytestmark = pytest.mark.gpu


def _ncol(name):
    kind, arg = tc.TABLE[name]
    return arg.get('ncol', 3) if kind == 'toy' else arg[1] if kind == 'inst' else arg


def _has_ray_serial(name):
    """the ray-serial kernels exist for five rays and a wavelength-independent scattering coefficient (lsx_set_sweep_policy refuses
    the mapping for any other shape: asserted below)"""
    kind, arg = tc.TABLE[name]
    return kind != 'toy' or (arg.get('Nrays', 3) == 5 and not arg.get('sca_per_lambda', False))


RUNS = [(name, policy) for name in tc.NAMES
        for policy in ((('ray-per-lane', 'ray-serial') if _has_ray_serial(name) else ('ray-per-lane',)) if _ncol(name) >= 32 else ('auto',))]


@pytest.mark.parametrize('name,policy', RUNS, ids=['%s-%s' % r for r in RUNS])
def test_hip_meets_the_reference(hip_lib, oracle_lib, name, policy):
    """formal solutions 1-4 with a statistical equilibrium behind the 3rd and the 4th"""
    c = tr.case(name)
    ncol = c.block.ncol
    assert ncol == _ncol(name)
    bars = tr.oracle_bars(oracle_lib, name)
    e = Engine(c.prob, ncol, lib=hip_lib, sweep_policy=policy)
    e.set_columns(0, c.block)
    if not _has_ray_serial(name):
        with pytest.raises(_capi.LsxError):
            e.set_sweep_policy('ray-serial')
    snaps = tr.run(e, np.asarray(c.cols))
    table, fused = classes_run(hip_lib, e)
    e.close()
    ratios = tr.check_sequence('HIP, %s' % policy, c, bars, snaps)
    print('%s %s: deviation / bar  %s' % (name, policy, '  '.join('%s %.3g' % kv for kv in ratios.items())))
    # ---- what ran: per-class launches for >= 32 columns, the fused launch below; the instances the ledger lists the case for
    serial = {k for k, (_, rs) in table.items() if rs}
    if policy == 'auto':
        assert fused == tr.NCALLS and not serial, (fused, table)
    else:
        assert fused == 0
        assert all(launches == tr.NCALLS for launches, _ in table.values()), table
        if policy == 'ray-serial':
            assert serial == {k for k in table if 0 <= k[0] <= 2}, (serial, table)      # every class with at most two per-ray slots
        else:
            assert not serial
    if tc.family(name) == 'inst':
        for key in ic.EXPECT[name[len('inst-'):]]:
            assert key in table and table[key][0] == tr.NCALLS, (key, table)


@pytest.mark.parametrize('name', tc.NAMES)
def test_rates_meet_the_reference(hip_lib, oracle_lib, name):
    """Engine.radiative_rates after ONE formal solution: one call from zero with J-dagger = J of call 1 and the starting populations --
    the reference's t.Rij / t.Rji of call 2, zeroed in front of it (the reference never zeroes them).  Rji_ref is the reference's
    rh_method.py:692.  Ray groups of 1, 2, 3, 4, 5, 7 and 8 rays on topologies with cross terms"""
    c = tr.case(name)
    e = Engine(c.prob, c.block.ncol, lib=hip_lib)
    e.set_columns(0, c.block)
    e.formal_sol_gamma()
    J = e.get(tr.J_)[c.cols]
    r = e.radiative_rates()
    e.close()
    assert r.Rij.shape == (c.block.ncol, c.prob.Ntrans, c.prob.Nspace)
    runs = tr.oracle_rates_bars(oracle_lib, c, J)
    ratio, own = tr.check_rates('HIP', c, runs, r.Rij[c.cols], r.Rji_ref[c.cols])
    print('%s rates: deviation / bound %.3g (the oracle against the reference: %.3g of its bar)' % (name, ratio, own))
