"""Native set-up of columns (Engine.setup_columns) and the fixture-free response function (response.native_response_function) on the
device, pinned at the 164 + 1 columns of the FALC CaII temperature response function, whose inputs the unmodified reference
recorded (tests/golden/rf_ca_inputs.npz) and whose converged runs it recorded too (rf_ca_outputs.npz).

4. the inputs of all 165 columns, made by setup_columns in one engine, against the reference's at the perturbed depth (the set-up
   chain's bars, tests/setup_cases.py; the background's, tests/background_cases.py) and bit-equal to the base column elsewhere;
5. the driver at ks = (0, 40, 81) bit-equal to a twin that is handed the read-back arrays through set_columns, and that twin's run
   inside the computed bars of tests/envelope.py against the oracle on the same arrays;
6. all 82 depths against the reference's converged runs: every iteration count exactly, n and I inside the converged-run bar 1e-6;
7. the other parameters (vturb, ne, nHTot, vlos), each perturbed column bit-equal to the same atmosphere set up and iterated alone.

Measured on MI355X: see DESIGN.md, "The native set-up: how it is pinned"."""
import numpy as np
import pytest

import background_cases as bc
import eqpops_cases as ec
import envelope
import scales_cases as scc
import setup_cases as sc
from conftest import golden, relerr
from test_response_every_depth import _Recorder, _rf_excess, load_rf_outputs, SE_FROM, TOL
from lightspinner_amd import ColumnBlock, Engine, _capi, atomdata, drivers, fixtures, native, response

pytestmark = pytest.mark.gpu

NS = 82
EPS = sc.EPS


def make_setup(problem_file='falc_ca.npz'):
    """-> (prob, raw, NativeSetup, ColumnModel of FALC on its column-mass scale), all from committed fixtures"""
    d = ec._npz('setup_falc.npz')
    prob, block, raw = fixtures.load_problem_npz(golden(problem_file))
    s = scc.fixture()
    assert np.array_equal(s['falc_cm_temperature'], raw['temperature']) and np.array_equal(s['falc_cm_nHTot'], raw['nHTot'])
    setup = native.NativeSetup(atomdata.from_fixture(d, atoms=[1]), atomdata.from_fixture(d, atoms=[0]).atoms[0], [float(d['m1_abundance'])],
                               bc.tables(), float(s['logG']))
    model = native.ColumnModel('column_mass', s['falc_cm_depth_scale'], raw['temperature'], raw['ne'], raw['nHTot'], raw['vturb'])
    return prob, raw, setup, model


@pytest.fixture(scope='module')
def falc():
    return make_setup()


@pytest.fixture(scope='module')
def inputs(hip_lib, falc):
    """the 165 columns (base, then k0+, k0-, k1+, ...) set up natively in ONE engine, and everything read back"""
    prob, raw, setup, model = falc
    batch = native.perturbed(model.validated(NS), 'temperature', 50.0, range(NS))
    eng = Engine(prob, 165, lib=hip_lib)
    eng.setup_columns(0, model, setup)
    eng.setup_columns(1, batch, setup)
    got = {w: eng.get(w) for w in (_capi.LSX_NSTAR, _capi.LSX_N, _capi.LSX_C, _capi.LSX_VBROAD, _capi.LSX_ADAMP, _capi.LSX_PHI, _capi.LSX_WPHI)}
    T = np.concatenate([model.validated(NS).temperature, batch.temperature])
    tile = lambda a: np.tile(np.asarray(a, dtype=np.float64), (165, 1))
    chi, eta, sca = eng.background(setup.tables, T, tile(raw['nHTot']), tile(raw['ne']))
    scales = eng.convert_scales(setup.tables, 'column_mass', tile(model.depth_scale), T, tile(raw['nHTot']), logG=setup.logG)
    eng.close()
    return dict(got=got, T=T, chi=chi, eta=eta, sca=sca, height=scales.height, nTotal=(setup.abundances[0] * tile(raw['nHTot']))[:, None])


def _col(k, tag):
    return 1 + 2 * k + (0 if tag == 'p' else 1)


# ---- 4. the inputs of all 165 columns -------------------------------------------------------------------------------------------------
def test_inputs_of_all_165_columns(falc, inputs):
    prob, raw, setup, model = falc
    rf, g = ec._npz('rf_ca_inputs.npz'), inputs['got']
    atom = setup.atomic_data.atoms[0]
    lines = [kr for kr, t in enumerate(prob.trans) if t.is_line]
    led = sc.Ledger('native set-up, 164 columns')
    # the base column against the problem file (the reference's FALC)
    T0 = raw['temperature']
    led.check('base nStar', g[_capi.LSX_NSTAR][0], raw['a0_nStar'], sc.nstar_bar(atom.E_SI, T0))
    led.check('base vBroad', g[_capi.LSX_VBROAD][0, 0], raw['a0_vBroad'], 4 * EPS)
    led.check('base aDamp', g[_capi.LSX_ADAMP][0], np.array([raw['t%d_aDamp' % kr] for kr in lines]), 32 * EPS)
    _, B = sc.rates_and_bars(atom, T0, raw['ne'], raw['a0_nStar'])
    sc.check_rates(led, 'base C', g[_capi.LSX_C][0].reshape(6, 6, NS), raw['a0_C'], B)
    block = fixtures.load_problem_npz(golden('falc_ca.npz'))[1]
    assert relerr(g[_capi.LSX_PHI][0], block.phi[0]) < 3e-13 and relerr(g[_capi.LSX_WPHI][0], block.wphi[0]) < 1e-13
    assert np.array_equal(g[_capi.LSX_N], g[_capi.LSX_NSTAR])
    env0 = bc.falc_env_for(raw['wavelength']) * np.abs(raw['bg_chi'])
    bc.inside(inputs['chi'][0], raw['bg_chi'], env0, 'base chi')
    bc.inside(inputs['eta'][0], raw['bg_eta'], env0 * bc.planck(T0[None, :], raw['wavelength'][:, None]), 'base eta')
    d = bc.fixture()
    phi_dev = wphi_dev = 0.0
    off = np.concatenate([[0], np.cumsum([prob.trans[kr].Nlambda for kr in lines])])
    for k in range(NS):
        others = np.arange(NS) != k
        for s, tag in enumerate('pm'):
            c, pre = _col(k, tag), 'k%d%s_' % (k, tag)
            assert inputs['T'][c, k] == float(rf[pre + 'temperature'])
            # every other depth: the base column's bits
            for w, a in g.items():
                assert np.array_equal(a[c][..., others], a[0][..., others]), (pre, w)
            for w in ('chi', 'eta'):
                assert np.array_equal(inputs[w][c][:, others], inputs[w][0][:, others]), (pre, w)
            assert np.array_equal(inputs['sca'][c], inputs['sca'][0])
            # depth k: the reference's
            Tk = np.array([float(rf[pre + 'temperature'])])
            led.check('nStar', g[_capi.LSX_NSTAR][c][:, k], rf[pre + 'a0_nStar'], sc.nstar_bar(atom.E_SI, Tk)[:, 0])
            led.check('vBroad', g[_capi.LSX_VBROAD][c][0, k], rf[pre + 'a0_vBroad'], 4 * EPS)
            led.check('aDamp', g[_capi.LSX_ADAMP][c][:, k], np.array([rf['%st%d_aDamp' % (pre, kr)] for kr in lines]), 32 * EPS)
            _, B = sc.rates_and_bars(atom, Tk, raw['ne'][k:k + 1], rf[pre + 'a0_nStar'][:, None])
            sc.check_rates(led, 'C', g[_capi.LSX_C][c][:, k].reshape(6, 6, 1), rf[pre + 'a0_C'][:, :, None], B)
            ref_phi = np.concatenate([rf['%st%d_phi' % (pre, kr)] for kr in lines])
            assert ref_phi.shape == (off[-1],)
            phi_dev = max(phi_dev, relerr(g[_capi.LSX_PHI][c][:, k], ref_phi))
            wphi_dev = max(wphi_dev, relerr(g[_capi.LSX_WPHI][c][:, k], np.array([rf['%st%d_wphi' % (pre, kr)] for kr in lines])))
            q = s * NS + k                                   # the background fixture's order of the 164 points
            assert d['rf_temperature'][q] == Tk[0]
            env = bc.rel_env(d['rf_chi_env16'][q]) * np.abs(rf[pre + 'bg_chi'])
            bc.inside(inputs['chi'][c][:, k], rf[pre + 'bg_chi'], env, pre + 'chi')
            bc.inside(inputs['eta'][c][:, k], rf[pre + 'bg_eta'], env * bc.planck(Tk[0], raw['wavelength']), pre + 'eta')
    print('phi: largest relative deviation %.3g (bar 3e-13), wphi %.3g (bar 1e-13)' % (phi_dev, wphi_dev))
    assert phi_dev < 3e-13 and wphi_dev < 1e-13
    led.report()
    # heights: a temperature perturbation moves them by hTau1 alone -- the steps are the base column's
    h = inputs['height']
    s = scc.fixture()
    scc.inside(h[0], s['falc_cm_height'], 'base height', height_shifted=True)
    step0 = np.diff(h[0])
    dev = np.abs(np.diff(h[1:], axis=1) - step0)
    bar = scc.BASE * (np.abs(h[1:, 1:]) + np.abs(h[1:, :-1]) + 2 * np.abs(h[1:, :1]))           # the scales bar on each of the two heights
    print('height steps against the base column: largest deviation %.3g m, %.3g of the bar; %s'
          % (dev.max(), float(np.max(dev / bar)), 'bit-equal' if not dev.any() else 'not bit-equal'))
    assert np.all(dev <= bar)


# ---- 5. the driver, ks = (0, 40, 81) ---------------------------------------------------------------------------------------------------
def _twin_blocks(prob, inputs, cols, n_start):
    g = inputs['got']
    pick = lambda a: np.ascontiguousarray(a[cols])
    return ColumnBlock(height=pick(inputs['height']), temperature=pick(inputs['T']), nStar=pick(g[_capi.LSX_NSTAR]), nTotal=pick(inputs['nTotal']),
                       n=pick(g[_capi.LSX_NSTAR]) if n_start is None else np.tile(n_start, (len(cols), 1, 1)), C=pick(g[_capi.LSX_C]),
                       bg_chi=pick(inputs['chi']), bg_eta=pick(inputs['eta']), bg_sca=pick(inputs['sca']), phi=pick(g[_capi.LSX_PHI]),
                       wphi=pick(g[_capi.LSX_WPHI])).validate(prob)


def test_driver_against_a_twin_fed_through_set_columns(hip_lib, oracle_lib, falc, inputs):
    prob, raw, setup, model = falc
    ks = (0, 40, 81)
    out = response.native_response_function(prob, setup, model, 'temperature', 50.0, ks=ks, lib=hip_lib)
    assert out['mus'] is None and out['shard'] == (0, 6) and out['rf'].shape == (prob.Nspect, 3)
    # the twin: the same columns through set_columns, made from the arrays read back from the natively set-up engine
    e0 = Engine(prob, 1, lib=hip_lib)
    e0.set_columns(0, _twin_blocks(prob, inputs, [0], None))
    it0 = drivers.iterate_mali_engine(e0).n_iter
    I_base, n_base = e0.get(_capi.LSX_I)[0], e0.get(_capi.LSX_N)[0]
    e0.close()
    assert it0 == out['n_iter_base'] and np.array_equal(I_base, out['I_base']) and np.array_equal(n_base, out['n_base'])
    cols = [_col(k, t) for k in ks for t in 'pm']
    batch = _twin_blocks(prob, inputs, cols, n_base)
    eng = Engine(prob, 6, lib=hip_lib, policy_columns=6)
    eng.set_columns(0, batch)
    rec = _Recorder(eng)
    niter = drivers.iterate_mali_columns(rec)
    I, n = eng.get(_capi.LSX_I), eng.get(_capi.LSX_N)
    eng.close()
    assert np.array_equal(niter, out['n_iter'])
    assert np.array_equal(I, out['I']) and np.array_equal(n, out['n'])
    assert np.array_equal(drivers.response_function(I[0::2], I[1::2], I_base), out['rf'])
    # the twin's run inside the computed bars against the oracle on the same arrays
    def make():
        e = Engine(prob, 6, lib=oracle_lib)
        e.set_columns(0, batch)
        oracle_lib.dll.lsx_oracle_set_threads(e._h, 16)
        return e
    eo = make()
    niter_o = drivers.iterate_mali_columns(eo)
    I_o = eo.get(_capi.LSX_I)
    eo.close()
    assert np.array_equal(niter, niter_o)
    bars = envelope.SequenceBars(oracle_lib, make, prob, int(niter.max()), SE_FROM, TOL, what=(_capi.LSX_I, _capi.LSX_GAMMA), what0=(_capi.LSX_J,))
    col = [bars.subset([c]) for c in range(6)]
    dn_last, dn_in, ratio = np.zeros(6), np.zeros(6), 0.0
    for j in range(SE_FROM, len(rec.calls)):
        for c in np.flatnonzero(niter > j):
            dn_in[c] = dn_last[c]
            dn_last[c] = col[c].check_n(rec.calls[j][_capi.LSX_N][c][None], col[c].oracle(j, _capi.LSX_N), j, ' (native twin vs oracle, column %d)' % c,
                                        dn_in[c], quiet=True)
            ratio = max(ratio, dn_last[c] / col[c].chain_cap(j))
    worst = 0.0
    for c in range(6):
        bI = col[c].I_bar(int(niter[c]) - 1, dn_in[c])
        dI = relerr(I[c], I_o[c])
        assert dI <= bI, (c, dI, bI)
        worst = max(worst, dI / bI)
    print('native twin vs oracle: largest delta_n / cap %.3f, I %.3f of its bar' % (ratio, worst))


# ---- 6. against the reference, all 82 depths -------------------------------------------------------------------------------------------
def test_all_depths_against_the_reference(hip_lib, falc):
    prob, raw, setup, model = falc
    ref = load_rf_outputs()
    out = response.native_response_function(prob, setup, model, 'temperature', 50.0, lib=hip_lib)
    assert out['n_iter_base'] == int(ref['base_niter']) == 46
    want = np.array([int(ref['k%d%s_niter' % (k, t)]) for k in range(NS) for t in 'pm'])
    assert np.array_equal(out['n_iter'], want), np.flatnonzero(out['n_iter'] != want)
    dn, dI = relerr(out['n_base'], ref['base_n']), relerr(out['I_base'][:, -1], ref['base_I'][:, -1])
    assert dn < 1e-6 and dI < 1e-6, (dn, dI)
    worst_rf = 0.0
    for k in range(NS):
        for s, t in enumerate('pm'):
            c, pre = 2 * k + s, 'k%d%s_' % (k, t)
            a, b = relerr(out['n'][c], ref[pre + 'n']), relerr(out['I'][c][:, -1], ref[pre + 'I'][:, -1])
            assert a < 1e-6 and b < 1e-6, (pre, a, b)
            dn, dI = max(dn, a), max(dI, b)
        r = _rf_excess(out['I'][2 * k][:, -1], out['I'][2 * k + 1][:, -1], out['I_base'][:, -1], ref['k%dp_I' % k][:, -1], ref['k%dm_I' % k][:, -1],
                       ref['base_I'][:, -1], 1e-6)
        assert r <= 1.0, (k, r)
        worst_rf = max(worst_rf, r)
    assert np.array_equal(out['rf'], drivers.response_function(out['I'][0::2], out['I'][1::2], out['I_base']))
    print('native response function vs reference: largest deviation of n %.3g, of I %.3g (bar 1e-6); rf %.3g of its bar' % (dn, dI, worst_rf))


# ---- 7. the other parameters -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('parameter', ['vturb', 'ne', 'nHTot', 'vlos'])
def test_other_parameters(hip_lib, falc, parameter):
    ks = (10, 60)
    if parameter == 'vlos':
        with pytest.raises(ValueError, match='phi_compact'):
            response.native_response_function(falc[0], falc[2], falc[3], 'vlos', 500.0, ks=ks, lib=hip_lib)
        prob, raw, setup, model = make_setup('falc_ca_vlos.npz')
        model.vlos = raw['vlos']
    else:
        prob, raw, setup, model = falc
    m = model.validated(NS)
    if parameter in ('ne', 'nHTot'):
        # +-2 % of the local value: the amplitude is absolute, so one call per depth
        outs = [response.native_response_function(prob, setup, model, parameter, 0.04 * float(getattr(m, parameter)[0, k]), ks=(k,), lib=hip_lib,
                                                  mus=[0.2, 1.0]) for k in ks]
        amps = [0.04 * float(getattr(m, parameter)[0, k]) for k in ks]
    else:
        amp = {'vturb': 400.0, 'vlos': 1000.0}[parameter]              # +-200 m/s, +-500 m/s
        outs = [response.native_response_function(prob, setup, model, parameter, amp, ks=ks, lib=hip_lib, mus=[0.2, 1.0])]
        amps = [amp]
    assert not np.any(prob.muz == 1.0)          # the quadrature has no vertical ray: shapes and finiteness of the rays' rf
    for out, amp, kk in zip(outs, amps, ([k] for k in ks) if len(outs) > 1 else [list(ks)]):
        nj = 2 * len(kk)
        assert out['rf'].shape == (prob.Nspect, len(kk), 2) and np.all(np.isfinite(out['rf']))
        assert out['I_mus'].shape == (nj, prob.Nspect, 2) and out['I_base_mus'].shape == (prob.Nspect, 2) and np.array_equal(out['mus'], [0.2, 1.0])
        assert np.any(out['rf'] != 0.0)
        batch = native.perturbed(m, parameter, amp, kk)
        for c in range(nj):
            e = Engine(prob, 1, lib=hip_lib, policy_columns=nj)
            e.setup_columns(0, batch.slice(c, c + 1), setup, start_n=out['n_base'])
            it = drivers.iterate_mali_columns(e)
            assert int(it[0]) == int(out['n_iter'][c]), (parameter, c)
            assert np.array_equal(e.get(_capi.LSX_I)[0], out['I'][c]) and np.array_equal(e.get(_capi.LSX_N)[0], out['n'][c]), (parameter, c)
            assert np.array_equal(e.emergent_rays([0.2, 1.0])[0], out['I_mus'][c])
            e.close()
        # the two signs differ from each other and from the base column
        assert not np.array_equal(out['I'][0], out['I'][1]) and not np.array_equal(out['I'][0], out['I_base'])


def test_refusals(hip_lib, falc):
    prob, raw, setup, model = falc
    with pytest.raises(ValueError, match='parameter'):
        response.native_response_function(prob, setup, model, 'pressure', 1.0, ks=(3,), lib=hip_lib)
    for ks in ((-1,), (82,), (3, 100)):
        with pytest.raises(ValueError, match='ks'):
            response.native_response_function(prob, setup, model, 'temperature', 50.0, ks=ks, lib=hip_lib)
    two = native.ColumnModel('column_mass', *(np.stack([getattr(model, k)] * 2) for k in native.ColumnModel.FIELDS[:-1]))
    with pytest.raises(ValueError, match='one'):
        response.native_response_function(prob, setup, two, 'temperature', 50.0, ks=(3,), lib=hip_lib)
