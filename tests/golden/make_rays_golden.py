#!/usr/bin/env python3
"""Generate tests/golden/rays_falc.npz: the UNMODIFIED reference's emergent spectra at arbitrary viewing angles.

What a user of the reference does after the MALI loop has converged: build a Context on `Falc82().rays(mus)`
(atmosphere.py:386-393: the wanted direction cosines with zero quadrature weights), put the converged populations and J
into it and call formal_sol_gamma_matrices() once; ctx.I is then [Nspect][nmu] (rh_method.py:638).  The states come from
fixtures that are committed already:
  ca       CaII active, vlos = 0          falc_ca.npz       conv_n_a0, conv_J
  ca_vlos  CaII active, the vlos ramp     falc_ca_vlos.npz  se5_n_a0, last_J
  cah      Ca + H active                  falc_cah.npz      se5_n_a*, last_J
The reference is imported the way make_golden.py imports it (stand-ins for numba / astropy / specutils from _refstubs).
Numbers only are written: the angles and ctx.I per case.

Usage:  python tests/golden/make_rays_golden.py
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import make_golden as mg  # noqa: E402  (puts the reference and the stand-ins on sys.path, applies the numpy-2 patch)

# limb ... the quadrature's largest angle ... disc centre.  (0.05 is left out on purpose: there the C restatement of the
# reference is itself 2.9e-11 from the reference on Ca + H -- it would test libm, not the kernel)
MUS = [0.1, 0.2, 0.33, 0.6, 0.77, 0.9530899229693319, 1.0]


def vlos_ramp():
    k = np.arange(82)
    return 4.0e3 * np.sin(2 * np.pi * k / 41.0) * np.exp(-((k - 35.0) / 25.0) ** 2) + 1.5e3      # gen_falc_ca_vlos


def context_on_rays(active, mus, vlos=None):
    """test.py:8-18 with Atmosphere.rays(mus) in place of the quadrature"""
    ac = mg.Falc82()
    ac.rays([float(m) for m in mus])
    if vlos is not None:
        ac.vlos[:] = vlos
    atmos = ac.convert_scales()
    aSet = mg.RadiativeSet([mg.CaII_atom(), mg.H_6_atom()])
    aSet.set_active(*active)
    spect = aSet.compute_wavelength_grid()
    eqPops = aSet.compute_eq_pops(atmos)
    background = mg.Background(atmos, spect)
    return mg.Context(atmos, spect, eqPops, background)


def final_pass(ctx, pops, J):
    for atom, n in zip(ctx.activeAtoms, pops):
        atom.n[...] = n
    ctx.J[...] = J
    with np.errstate(all='ignore'):          # (zero weights: wphi = 1 / 0 and dJ = inf; neither enters I)
        ctx.formal_sol_gamma_matrices()
    return np.array(ctx.I)


def main():
    d = {'mus': np.array(MUS)}
    cases = (('ca', ['Ca'], None, 'falc_ca.npz', 'conv', 'conv_J'),
             ('ca_vlos', ['Ca'], vlos_ramp(), 'falc_ca_vlos.npz', 'se5', 'last_J'),
             ('cah', ['Ca', 'H'], None, 'falc_cah.npz', 'se5', 'last_J'))
    for name, active, vlos, fixture, ntag, jkey in cases:
        t0 = time.time()
        raw = np.load(os.path.join(HERE, fixture))
        with np.errstate(all='ignore'):
            ctx = context_on_rays(active, MUS, vlos)
        pops = [raw['%s_n_a%d' % (ntag, a)] for a in range(len(ctx.activeAtoms))]
        assert [str(x) for x in raw['atom_names']] == [a.atomicModel.name for a in ctx.activeAtoms]
        assert np.array_equal(raw['wavelength'], np.array(ctx.spect.wavelength))
        I = final_pass(ctx, pops, raw[jkey])
        assert I.shape == (raw['wavelength'].shape[0], len(MUS)) and np.all(np.isfinite(I))
        d['%s_I' % name] = I
        print('%s: I %s, %.1f s' % (name, I.shape, time.time() - t0), flush=True)
    path = os.path.join(HERE, 'rays_falc.npz')
    np.savez_compressed(path, **d)
    print('wrote %s (%.1f kB)' % (path, os.path.getsize(path) / 1e3))


if __name__ == '__main__':
    main()
