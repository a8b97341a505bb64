#!/usr/bin/env python3
"""Generate tests/golden/spectrum_falc.npz: the UNMODIFIED reference's emergent spectra at wavelengths that are not points of the
grid the populations were iterated on.

What a user of the reference does: RadiativeSet.compute_wavelength_grid(extraWavelengths=w) (atomic_set.py:377-383), a Context on
that finer grid and on Falc82().rays(mus) (make_rays_golden.py), the converged populations put into it, J on the finer grid, one
formal_sol_gamma_matrices().  The states are those of rays_falc.npz (committed fixtures); J on the union grid follows the rule of
include/lsx_hip_spectrum.h from the committed J: linear between the bracketing points of the old grid, two products and a sum, held
constant outside.  Cases:
  ca_vlos  CaII active, the vlos ramp   falc_ca_vlos.npz  se5_n_a0, last_J   a window on 8542, one on H & K, six continuum points
                                                                            (two of them beyond the grid)
  cah      Ca + H active                falc_cah.npz      se5_n_a*, last_J   a window on H alpha (inside the Paschen continuum), one on
                                                                            Lyman alpha
Numbers only are written, per case at the extra wavelengths alone: w, bg_chi, bg_eta [nla][Nspace], alpha [Ncont][nla] (zero outside
a continuum's window), I [nla][nmu], and every transition's Nblue / Nlambda on the union grid.  The angles are rays_falc.npz's.

Usage:  python tests/golden/make_spectrum_golden.py [--check]
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import make_golden as mg  # noqa: E402  (puts the reference and the stand-ins on sys.path, applies the numpy-2 patch)
import make_rays_golden as mrg  # noqa: E402

MUS = mrg.MUS
WANTED = {
    'ca_vlos': np.concatenate([np.linspace(854.0, 854.4, 101), np.linspace(392.9, 394.1, 67), [40.0, 91.0, 91.2, 300.0, 1000.0, 5000.0]]),
    'cah': np.concatenate([np.linspace(656.0, 656.6, 130), np.linspace(121.4, 121.8, 33)]),
}


def context_on_grid(active, mus, w, vlos=None):
    """make_rays_golden.context_on_rays with the extra wavelengths in the grid"""
    ac = mg.Falc82()
    ac.rays([float(m) for m in mus])
    if vlos is not None:
        ac.vlos[:] = vlos
    atmos = ac.convert_scales()
    aSet = mg.RadiativeSet([mg.CaII_atom(), mg.H_6_atom()])
    aSet.set_active(*active)
    spect = aSet.compute_wavelength_grid(extraWavelengths=np.asarray(w, dtype=np.float64))
    eqPops = aSet.compute_eq_pops(atmos)
    background = mg.Background(atmos, spect)
    return mg.Context(atmos, spect, eqPops, background)


def by_rule(lam, X, wu):
    """X [Nspect][Nspace] on lam -> on wu: (1 - t) X[l] + t X[l+1] with l = clamp(upper_bound - 1), t clamped to [0, 1]"""
    N = lam.shape[0]
    l = np.clip(np.searchsorted(lam, wu, side='right') - 1, 0, N - 2)
    t = np.clip((wu - lam[l]) / (lam[l + 1] - lam[l]), 0.0, 1.0)
    return (1.0 - t)[:, None] * X[l] + t[:, None] * X[l + 1]


def generate():
    d = {'mus': np.array(MUS)}
    cases = (('ca_vlos', ['Ca'], mrg.vlos_ramp(), 'falc_ca_vlos.npz', 'se5', 'last_J'),
             ('cah', ['Ca', 'H'], None, 'falc_cah.npz', 'se5', 'last_J'))
    for name, active, vlos, fixture, ntag, jkey in cases:
        t0 = time.time()
        raw = np.load(os.path.join(HERE, fixture))
        w = np.sort(WANTED[name])
        lam = np.array(raw['wavelength'])
        assert np.all(np.diff(w) > 0)
        print('%s: %d of the wanted wavelengths are points of the grid' % (name, int(np.isin(w, lam).sum())))
        with np.errstate(all='ignore'):
            ctx = context_on_grid(active, MUS, w, vlos)
        wu = np.array(ctx.spect.wavelength)
        assert np.array_equal(wu, np.union1d(lam, w))
        rows = np.searchsorted(wu, w)
        pops = [raw['%s_n_a%d' % (ntag, a)] for a in range(len(ctx.activeAtoms))]
        assert [str(x) for x in raw['atom_names']] == [a.atomicModel.name for a in ctx.activeAtoms]
        I = mrg.final_pass(ctx, pops, by_rule(lam, np.array(raw[jkey]), wu))
        assert I.shape == (wu.shape[0], len(MUS)) and np.all(np.isfinite(I))
        trans = [t for a in ctx.activeAtoms for t in a.trans]
        assert len(trans) == raw['t_atom'].shape[0]
        alpha = []
        for t in trans:
            if t.isLine:
                continue
            a = np.zeros(wu.shape[0])
            a[t.Nblue:t.Nblue + t.wavelength.shape[0]] = t.alpha
            alpha.append(a[rows])
        bg = ctx.background
        d['%s_w' % name] = w
        d['%s_bg_chi' % name] = np.array(bg.chi)[rows]
        d['%s_bg_eta' % name] = np.array(bg.eta)[rows]
        sca = np.array(bg.sca)
        assert sca.ndim == 1 or np.all(sca == sca[:1])            # (one scattering coefficient per depth: the fixtures' bg_sca)
        d['%s_alpha' % name] = np.stack(alpha)
        d['%s_I' % name] = I[rows]
        d['%s_Nblue' % name] = np.array([t.Nblue for t in trans], dtype=np.int64)
        d['%s_Nlambda' % name] = np.array([t.wavelength.shape[0] for t in trans], dtype=np.int64)
        print('%s: %d extra wavelengths, union grid %d, I %s, %.1f s' % (name, w.shape[0], wu.shape[0], I[rows].shape, time.time() - t0),
              flush=True)
    return d


def main():
    path = os.path.join(HERE, 'spectrum_falc.npz')
    d = generate()
    if '--check' in sys.argv[1:]:
        old = np.load(path)
        bad = [k for k in sorted(set(d) | set(old.files)) if k not in d or k not in old.files or not np.array_equal(d[k], old[k])]
        print('check: %d arrays, %s' % (len(d), 'all equal' if not bad else 'DIFFERENT: ' + ', '.join(bad)))
        sys.exit(1 if bad else 0)
    np.savez_compressed(path, **d)
    print('wrote %s (%.1f kB)' % (path, os.path.getsize(path) / 1e3))


if __name__ == '__main__':
    main()
