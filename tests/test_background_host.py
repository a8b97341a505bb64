"""The background's formulas on the CPU (no GPU needed): the fixture's own bookkeeping, the Kurucz table parser, and
lsx_background_dev.h -- the header the HIP kernels are made of -- compiled with g++ -ffp-contract=off (liblsx_bg_host.so) against
the reference's numbers on every point of tests/golden/background_eos.npz, inside the bar of tests/background_cases.py.
The same code runs once more as a stand-alone program under -fsanitize=address,undefined (nothing is loaded into python)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import background_cases as bc
from conftest import golden

pytestmark = pytest.mark.skipif(shutil.which('g++') is None, reason='no host compiler')


@pytest.fixture(scope='module')
def host():
    return bc.HostLib()


@pytest.fixture(scope='module')
def host_eos(host):
    """the host build on every point of the fixture, once"""
    d = bc.fixture()
    out = {}
    for name in ('falc', 'rf', 'grid'):
        out[name] = host.eos(bc.tables(), d[name + '_temperature'], d[name + '_nHTot'])
    return out


def test_fixture_bookkeeping():
    d = bc.fixture()
    assert os.path.getsize(golden('background_eos.npz')) < (1 << 20)
    assert d['falc_temperature'].shape == (82,) and d['rf_temperature'].shape == (164,) and d['grid_temperature'].shape == (66,)
    falc = np.load(golden('falc_ca.npz'))
    assert np.array_equal(d['falc_temperature'], falc['temperature']) and np.array_equal(d['falc_nHTot'], falc['nHTot'])
    assert np.array_equal(d['rf_temperature'], np.concatenate([falc['temperature'] + 25.0, falc['temperature'] - 25.0]))
    for name in ('falc', 'rf', 'grid'):
        assert np.all(d[name + '_margin'] >= 1e-5), name                      # no stop test near a flip: the tests leave no point out
        assert np.all(d[name + '_nstop'] > d[name + '_npepg']) and np.all(d[name + '_npepg'] > 0)
        for key in ('pgas', 'pe', 'partials'):
            assert np.all(np.isfinite(d['%s_%s' % (name, key)])) and np.all(d['%s_%s_env' % (name, key)] >= 0)
    assert d['nstage'].shape == (28,) and d['pf'].shape == (28, 6, d['tpf'].shape[0]) and d['abund'].shape == (99,)
    assert d['grid_chi'].shape == (66, d['grid_wavelength'].shape[0]) and d['grid_wavelength'].shape[0] > 100
    for f in ('falc_ca.npz', 'falc_cah.npz', 'falc_all.npz'):                 # the FALC envelope covers the three committed grids
        assert np.all(np.isin(np.load(golden(f))['wavelength'], d['falc_env_wavelength']))
    assert d['falc_chi_env16'].shape == (d['falc_env_wavelength'].shape[0], 82) and d['falc_chi_env16'].dtype == np.float16
    assert d['rf_chi_env16'].shape == (164, 287)
    # the issue's measured envelope of the reference on FALC: at worst 2.3e-13 for chi
    assert 1e-13 < bc.rel_env(d['falc_chi_env16']).max() < 1e-12


def test_from_kurucz_xdr_bit_for_bit():
    ref = os.environ.get('LIGHTSPINNER_REF', '')
    path = os.path.join(ref, 'Data', 'pf_Kurucz.input')
    if not ref or not os.path.exists(path):
        pytest.skip('the reference\'s data file is not here (LIGHTSPINNER_REF)')
    d = bc.fixture()
    t = bc.EosTables.from_kurucz_xdr(path, d['abund'], d['amass'], float(d['weight_per_H']), nelem=28)
    for key in ('tpf', 'nstage', 'pf', 'eion'):
        assert np.array_equal(getattr(t, key), d[key]), key
    full = bc.EosTables.from_kurucz_xdr(path, d['abund'], d['amass'], float(d['weight_per_H']))
    assert full.nelem == 99 and np.array_equal(full.pf[:28], d['pf'])


def test_derived_scalars(host):
    d = bc.fixture()
    mine = host.derived(bc.tables())
    for x, key in zip(mine, ('ref_avw', 'ref_ab_others', 'ref_rho_from_H')):
        assert abs(x - float(d[key])) <= 99 * bc.U * abs(float(d[key])), (key, x, float(d[key]))


@pytest.mark.parametrize('name', ['falc', 'rf', 'grid'])
def test_host_eos_inside_the_bar(host_eos, name):
    d = bc.fixture()
    rc, pg, pe, part, st = host_eos[name]
    assert rc == 0
    assert np.array_equal(st, d[name + '_npepg'])              # the same number of pe_pg evaluations, point by point
    bc.inside(pg, d[name + '_pgas'], d[name + '_pgas_env'], name + ' pgas')
    bc.inside(pe, d[name + '_pe'], d[name + '_pe_env'], name + ' pe')
    bc.inside(part, d[name + '_partials'], d[name + '_partials_env'], name + ' partials')


def test_host_opacity_branch_grid(host, host_eos):
    d = bc.fixture()
    _, pg, pe, part, _ = host_eos['grid']
    chi, _ = host.opacity(d['grid_temperature'], pg, pe, part, d['grid_wavelength'])
    bc.inside(chi, d['grid_chi'], d['grid_chi_env'], 'grid chi (edges)')


@pytest.mark.parametrize('name', ['falc_ca.npz', 'falc_cah.npz', 'falc_all.npz'])
def test_host_opacity_falc(host, host_eos, name):
    g = np.load(golden(name))
    _, pg, pe, part, _ = host_eos['falc']
    chi, eta = host.opacity(g['temperature'], pg, pe, part, g['wavelength'])
    env = bc.falc_env_for(g['wavelength']) * np.abs(g['bg_chi'])
    bc.inside(chi.T, g['bg_chi'], env, name + ' chi')
    bc.inside(eta.T, g['bg_eta'], env * bc.planck(g['temperature'][None, :], g['wavelength'][:, None]), name + ' eta')


def test_host_opacity_response_points(host, host_eos):
    d = bc.fixture()
    rf = np.load(golden('rf_ca_inputs.npz'))
    _, pg, pe, part, _ = host_eos['rf']
    chi, eta = host.opacity(d['rf_temperature'], pg, pe, part, d['rf_env_wavelength'])
    ref_chi = np.array([rf['k%d%s_bg_chi' % (k, s)] for s in 'pm' for k in range(82)])
    ref_eta = np.array([rf['k%d%s_bg_eta' % (k, s)] for s in 'pm' for k in range(82)])
    env = bc.rel_env(d['rf_chi_env16']) * np.abs(ref_chi)
    bc.inside(chi, ref_chi, env, 'rf chi')
    bc.inside(eta, ref_eta, env * bc.planck(d['rf_temperature'][:, None], d['rf_env_wavelength'][None, :]), 'rf eta')


def test_iter_cap_flags_every_point(host):
    d = bc.fixture()
    for name in ('falc', 'grid'):
        rc, _, _, _, st = host.eos(bc.tables(iter_cap=3), d[name + '_temperature'], d[name + '_nHTot'])
        assert rc == 6 and np.all(st < 0), (name, rc, st)           # LSX_ENOCONV, a negative status everywhere
    assert b'point 0' in host.dll.lsx_bg_host_error()


def test_formulas_under_asan_ubsan(tmp_path):
    """the branch grid and the FALC points, the edge wavelengths and some far outside every table, in a stand-alone program"""
    d = bc.fixture()
    subprocess.check_call(['make', '-s', '-C', bc.CSRC, 'bgsan'])
    T = np.concatenate([d['grid_temperature'], d['falc_temperature'], [400.0, 1.0e6]])
    nH = np.concatenate([d['grid_nHTot'], d['falc_nHTot'], [d['falc_nHTot'].max(), d['falc_nHTot'].min()]])
    wl = np.unique(np.concatenate([d['grid_wavelength'], [0.5, 5.0, 1.0e5, 1.0e7]]))
    dump = tmp_path / 'bg.dump'
    with open(dump, 'wb') as f:
        np.array([d['tpf'].shape[0], 28, T.shape[0], wl.shape[0]], dtype=np.int32).tofile(f)
        d['tpf'].tofile(f)
        d['nstage'].astype(np.int32).tofile(f)
        for a in (d['pf'], d['eion'], d['abund'], d['amass'], np.array([float(d['weight_per_H'])]), T, nH, wl):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:halt_on_error=1', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')
    out = subprocess.run([os.path.join(bc.CSRC, 'lsx_bg_san'), str(dump)], capture_output=True, text=True, timeout=600, env=env)
    tail = out.stdout[-1500:] + '\n' + out.stderr[-3000:]
    assert out.returncode == 0, tail
    assert 'BG SANITIZED RUN COMPLETE' in out.stdout, tail
    assert 'AddressSanitizer' not in out.stderr and 'runtime error' not in out.stderr, tail
