"""The depth-scale conversion without a GPU: the fixture's own bookkeeping, the formulas of lsx_scales_dev.h compiled for the CPU
(liblsx_scales_host.so) against the reference inside the bar of tests/scales_cases.py -- fed the reference's chi_c, which isolates
the integration, and through the host equation of state and opacity, which covers the whole chain --, the rule for tau = 1 against
numpy.interp bit for bit, the stand-alone sanitizer program, and the argument checks that need no device."""
import os
import subprocess

import numpy as np
import pytest

from conftest import golden

import background_cases as bc
import scales_cases as sc


@pytest.fixture(scope='module')
def host():
    return sc.HostLib()


def test_fixture_bookkeeping():
    d = sc.fixture()
    assert os.path.getsize(golden('scales_falc.npz')) < (1 << 20)
    names = sc.cases()
    assert len(names) == len(set(names)) == 3 + 6 * 3 + 6 * 3 + 1
    assert float(d['weight_per_H']) == sc.tables().weight_per_H
    assert {sc.Case(n).N for n in names} == {2, 4, 12, 33, 40, 82, 325}
    for n in names:
        c = sc.Case(n)
        assert c.T.min() >= 2500.0
        for q in sc.QUANTITIES:
            assert c.ref[q].shape == (3, c.N) and np.all(np.isfinite(c.ref[q])), (n, q)
        assert np.all(np.diff(c.ref['tau_ref'], axis=1) > 0), n
        assert np.all(np.diff(c.ref['height'], axis=1) < 0) and np.all(np.diff(c.ref['cmass'], axis=1) > 0), n
        if c.scale == sc.GEO:
            raw = 0.5 * c.ref['chi_c'][:, 0] * (c.ds[0] - c.ds[1])
            assert np.all(np.abs(raw - 1.0) >= 1e-3), (n, raw)
    # the three scales of a column describe the same column
    f = {s: sc.Case('falc_' + s) for s in ('cm', 'geo', 'tau')}
    assert np.array_equal(f['geo'].ds, f['cm'].ref['height'][0]) and np.array_equal(f['tau'].ds, f['cm'].ref['tau_ref'][0])
    # what the reference does at the edges (the cases exist for these)
    c = sc.Case('s0_40_cm')          # never reaches tau = 1: hTau1 = height[-1]
    assert c.ref['tau_ref'][0][-1] < 2e-5 and c.ref['height'][0][-1] == 0.0
    c = sc.Case('s70_82_cm')         # starts above tau = 1: hTau1 = height[0]
    assert c.ref['tau_ref'][0][0] > 2.4 and c.ref['height'][0][0] == 0.0
    for n, tau in (('s80_82_geo', [0, 6.98]), ('s78_82_geo', [0, 3.75, 8.94, 15.92])):      # tau[0] > 1 -> 0
        got = sc.Case(n).ref['tau_ref'][0]
        assert got[0] == 0.0 and np.allclose(got, tau, rtol=2e-3), (n, got)
    assert 4e-10 < sc.Case('falc_geo').ref['tau_ref'][0][0] < 6e-10


@pytest.mark.parametrize('name', sc.cases())
def test_host_integration_given_the_reference_opacity(host, name):
    c = sc.Case(name)
    rc, h, cm, tau = host.integrate(c.scale, float(sc.fixture()['weight_per_H']), c.ds, c.T, c.nH, c.ne, sc.gravity(), c.ref['chi_c'][0])
    assert rc == 0, host.error()
    sc.check_case(c, h[0], cm[0], tau[0], None, tag='given chi_c: ')


@pytest.mark.parametrize('name', sc.cases())
def test_host_whole_chain(host, name):
    c = sc.Case(name)
    rc, h, cm, tau, chi = host.convert(sc.tables(), c.scale, c.ds, c.T, c.nH, c.ne, sc.gravity())
    assert rc == 0, host.error()
    sc.check_case(c, h[0], cm[0], tau[0], chi[0], tag='whole chain: ')


def test_tau1_rule_is_numpy_interp_bit_for_bit(host):
    rng = np.random.default_rng(20261018)
    n_inside = 0
    for trial in range(3000):
        n = int(rng.integers(2, 101))
        tau = np.cumsum(rng.uniform(1e-3, 1.0, n)) * rng.choice([1e-3, 0.05, 0.3, 1.0, 4.0]) + rng.choice([0.0, 0.5, 1.5])
        kind = trial % 5
        if kind == 1:                       # 1.0 is a grid point
            j = int(rng.integers(0, n))
            tau = tau * (1.0 / tau[j])
            tau[j] = 1.0
        elif kind == 2:                     # 1.0 below the first point
            tau = tau + 1.0
        elif kind == 3:                     # 1.0 above the last point
            tau = tau / (tau[-1] * (1.0 + rng.uniform(1e-9, 1.0)))
        assert np.all(np.diff(tau) > 0)
        h = -np.cumsum(rng.uniform(1.0, 1e5, n)) + rng.uniform(0, 1e6)
        want = np.interp(1.0, tau, h)
        got = host.tau1(tau, h)
        assert got == want, (trial, n, got, want)
        n_inside += bool(tau[0] < 1.0 < tau[-1])
    assert n_inside > 500
    assert host.tau1(np.array([0.5, 1.0]), np.array([2.0, 1.0])) == 1.0            # 1 >= tau[-1]
    assert host.tau1(np.array([1.0, 2.0]), np.array([2.0, 1.0])) == 2.0            # tau[0] == 1


def test_formulas_under_asan_ubsan(tmp_path):
    """FALC and two perturbed columns on every scale, every combination of outputs, in a stand-alone program"""
    d = sc.fixture()
    b = bc.fixture()
    subprocess.check_call(['make', '-s', '-C', sc.CSRC, 'scalessan'])
    cols = [sc.Case(n) for n in ('falc_cm', 'p2_cm', 'p5_cm')]
    dump = tmp_path / 'scales.bin'
    with open(dump, 'wb') as f:
        np.array([b['tpf'].shape[0], 28, len(cols), 82], dtype=np.int32).tofile(f)
        b['tpf'].tofile(f)
        b['nstage'].astype(np.int32).tofile(f)
        for a in (b['pf'], b['eion'], b['abund'], b['amass'], np.array([float(d['weight_per_H']), sc.gravity()]),
                  np.array([c.ds for c in cols]), np.array([c.T for c in cols]), np.array([c.nH for c in cols]), np.array([c.ne for c in cols])):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:halt_on_error=1', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')
    out = subprocess.run([os.path.join(sc.CSRC, 'lsx_scales_san'), str(dump)], capture_output=True, text=True, timeout=600, env=env)
    tail = out.stdout[-1500:] + '\n' + out.stderr[-3000:]
    assert out.returncode == 0, tail
    assert 'SCALES SANITIZED RUN COMPLETE' in out.stdout, tail


def test_argument_checks(host):
    c = sc.Case('falc_cm')
    g, N = sc.gravity(), c.N
    EINVAL = 1
    ok = lambda *a: host.check(*a)
    assert ok(sc.CM, N, c.ds, c.T, c.nH, None, g) == 0
    assert ok(sc.TAU, N, c.ref['tau_ref'][0], c.T, c.nH, None, g) == 0
    assert ok(sc.GEO, N, c.ref['height'][0], c.T, c.nH, c.ne, g) == 0
    assert ok(3, N, c.ds, c.T, c.nH, None, g) == EINVAL and 'scale' in host.error()
    assert ok(-1, N, c.ds, c.T, c.nH, None, g) == EINVAL
    assert ok(sc.CM, 1, c.ds, c.T, c.nH, None, g) == EINVAL and 'Nspace < 2' in host.error()
    assert ok(sc.GEO, N, c.ref['height'][0], c.T, c.nH, None, g) == EINVAL           # the geometric scale reads ne
    for bad_g in (0.0, -1.0, np.nan, np.inf):
        assert ok(sc.GEO, N, c.ref['height'][0], c.T, c.nH, c.ne, bad_g) == EINVAL
        assert ok(sc.CM, N, c.ds, c.T, c.nH, None, bad_g) == 0                        # ... and gravity; the others do not
    for bad in (0.0, -1.0, np.nan, np.inf):
        for which in range(3):
            arrs = [c.T.copy(), c.nH.copy(), c.ne.copy()]
            arrs[which][40] = bad
            assert ok(sc.GEO, N, c.ref['height'][0], *arrs, g) == EINVAL, (bad, which)
            assert ok(sc.CM, N, c.ds, *arrs, g) == (0 if which == 2 else EINVAL), (bad, which)      # ne is not read
    T = c.T.copy()
    T[3] = 2400.0
    assert ok(sc.CM, N, c.ds, T, c.nH, None, g) == EINVAL and '2500' in host.error()
    T[3] = 2500.0
    assert ok(sc.CM, N, c.ds, T, c.nH, None, g) == 0
    # strictly monotonic depth scales: ascending and positive, or descending
    for scale, ds, ne in ((sc.CM, c.ds, None), (sc.TAU, c.ref['tau_ref'][0], None), (sc.GEO, c.ref['height'][0], c.ne)):
        for k, mode in ((10, 'equal'), (81, 'swap'), (0, 'nan')):
            x = ds.copy()
            if mode == 'equal':
                x[k] = x[k - 1]
            elif mode == 'swap':
                x[k], x[k - 1] = x[k - 1], x[k]
            else:
                x[k] = np.nan
            assert ok(scale, N, x, c.T, c.nH, ne, g) == EINVAL, (scale, mode)
            assert 'depth_scale' in host.error()
        if scale != sc.GEO:
            x = ds.copy()
            x[0] = 0.0
            assert ok(scale, N, x, c.T, c.nH, ne, g) == EINVAL
    # a second column is checked on its own: the first depth of a column is not compared with the last of the one before
    two = lambda a: np.array([a, a])
    assert ok(sc.CM, N, two(c.ds), two(c.T), two(c.nH), None, g) == 0
    assert ok(sc.GEO, N, two(c.ref['height'][0]), two(c.T), two(c.nH), two(c.ne), g) == 0
    rc, *_ = host.integrate(sc.CM, 1.0, c.ds[::-1].copy(), c.T, c.nH, None, g, c.ref['chi_c'][0])
    assert rc == EINVAL
