"""Drop-in check against what the reference's own objects computed.  The reference's values come from the fixtures
make_golden.py wrote from it: falc_ca.npz (FALC CaII, test.py's set-up: iterations 1-5), setup_falc.npz (the merged grid of
CaII + H) and live_ref.npz (what those two lack: each line's wlambda and iteration 6; `make_golden.py live_ref` checks that
the other two hold bit for bit what a live run of the reference computes).  The library's side is built from the reference's
model data kept in the fixtures (tests/helpers.build_data_fakes), so the library runs its own set-up chain, as it does on the
reference's objects."""
import numpy as np
import pytest

from conftest import golden, relerr


def test_context_against_live_reference(oracle_lib):
    from helpers import build_data_fakes
    from lightspinner_amd.rh_method import Context

    d = dict(np.load(golden('falc_ca.npz')))
    ref = dict(d, **np.load(golden('live_ref.npz')))
    atmos, spect, eq, bg = build_data_fakes(d, dict(np.load(golden('setup_falc.npz'))))
    name = str(d['atom_names'][0])
    mine = Context(atmos, spect, eq, bg, lib=oracle_lib)
    assert mine.setup == 'native'         # models that carry their atomic data: the library's set-up chain
    assert mine.activeAtoms[0].n is eq[name].n
    assert relerr(mine.activeAtoms[0].vBroad, ref['a0_vBroad']) < 1e-14
    for kr, t_mine in enumerate(mine.activeAtoms[0].trans):
        assert t_mine.Nblue == int(ref['t_Nblue'][kr]) and np.array_equal(t_mine.active, ref['t_active'][kr])
        if t_mine.isLine:
            assert relerr(t_mine.aDamp, ref['t%d_aDamp' % kr]) < 1e-13 and np.array_equal(t_mine.wlambda(), ref['t%d_wlambda' % kr])
            phi = ref['t%d_phi' % kr]          # stored once where it is the same for every ray and direction
            assert t_mine.phi.shape == (t_mine.wavelength.shape[0], atmos.Nrays, 2, atmos.Nspace)
            assert relerr(t_mine.phi, phi if phi.ndim == 4 else np.broadcast_to(phi[:, None, None, :], t_mine.phi.shape)) < 1e-13
            assert relerr(t_mine.wphi, ref['t%d_wphi' % kr]) < 1e-13
    assert kr + 1 == ref['t_Nblue'].shape[0]
    for it in range(1, 7):
        dJ = mine.formal_sol_gamma_matrices()
        assert dJ == pytest.approx(float(ref['fs%d_dJ' % it]), rel=1e-8)
        tol = 1e-12 if it < 5 else 1e-8
        assert relerr(mine.J, ref['fs%d_J' % it]) < tol and relerr(mine.I, ref['fs%d_I' % it]) < tol
        assert relerr(mine.activeAtoms[0].C, ref['a0_C'], floor=1e-300) < 1e-13      # the reference's C is the same every iteration
        if it > 3:
            dP = mine.stat_equil()
            assert dP == pytest.approx(float(ref['se%d_dPops' % it]), rel=1e-7)
            assert relerr(eq[name].n, ref['se%d_n' % it] if it == 6 else ref['se%d_n_a0' % it]) < 1e-7


def test_wavelength_grid_against_live_reference(oracle_lib):
    """the reference's RadiativeSet.compute_wavelength_grid (CaII + H active) and lightspinner_amd.spectrum.compute_wavelength_grid
    on the same models, each transition on its local grid: grid, blueIdx and active sets identical, continuum alpha to 1e-14"""
    from helpers import build_data_fakes, restore_local_grids
    from lightspinner_amd.spectrum import compute_wavelength_grid
    s = dict(np.load(golden('setup_falc.npz')))
    names = [str(x) for x in s['atom_names']]           # the reference's model order
    _, spect0, _, _ = build_data_fakes(dict(np.load(golden('falc_cah.npz'))), s)
    fresh = {m.name: m for m in restore_local_grids(spect0.radSet.activeAtoms, s)}
    models = [fresh[n] for n in names]
    owner = {id(t): m.name for m in models for t in list(m.lines) + list(m.continua)}
    mine = compute_wavelength_grid(models, lib=oracle_lib)
    assert np.array_equal(mine.wavelength, s['grid_wavelength'])
    assert mine.blueIdx == [int(b) for b in s['grid_blueIdx']]
    assert len(mine.transitions) == s['grid_trans_order'].shape[0]
    for k, (t_mine, (a, il, q)) in enumerate(zip(mine.transitions, s['grid_trans_order'])):
        pre = 'm%d_%s_' % (a, 'line' if il else 'cont')
        assert (int(s[pre + 'i'][q]), int(s[pre + 'j'][q]), names[a]) == (t_mine.i, t_mine.j, owner[id(t_mine)])
        b = int(s['grid_blueIdx'][k])
        assert np.array_equal(s['grid_wavelength'][b:b + int(s['grid_Nlambda'][k])], t_mine.wavelength)
        if not il:
            alpha = s['m%d_cont%d_alpha' % (a, q)]
            assert np.max(np.abs(alpha - t_mine.alpha)) <= 1e-14 * np.max(alpha)
    index = {id(t): k for k, t in enumerate(mine.transitions)}
    for la in range(s['grid_wavelength'].shape[0]):
        assert list(np.nonzero(s['grid_active'][:, la])[0]) == [index[id(t)] for t in mine.activeSet[la]]
