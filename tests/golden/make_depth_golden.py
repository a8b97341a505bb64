#!/usr/bin/env python3
"""Generate tests/golden/depth_falc_<case>_<block>.npz: what the UNMODIFIED reference builds at every depth inside its final pass.

As make_rays_golden.py: a Context on `Falc82().rays(MUS)` (atmosphere.py:386-393) holds the converged populations and J of a
committed state and runs formal_sol_gamma_matrices() once.  rh_method.py:601-635 builds chiTot and S per (wavelength, ray,
direction) and formal_solver.piecewise_linear_1d returns I at every depth; the reference keeps I[0] only (rh_method.py:638).  Here
the name `piecewise_linear_1d` in the reference's rh_method module is replaced, for the duration of the call, by a wrapper that
records the `chi` and `S` it is handed and the `I` it returns for the up-going calls and passes everything through unchanged.
  ca       CaII active, vlos = 0          falc_ca.npz       conv_n_a0, conv_J
  ca_vlos  CaII active, the vlos ramp     falc_ca_vlos.npz  se5_n_a0, last_J
  cah      Ca + H active                  falc_cah.npz      se5_n_a*, last_J
Numbers only are written: the angles and chi, S, I as [wavelengths of the block][nmu][82].  A case is cut into blocks of BLOCK
wavelengths, one file each, so that no file exceeds 1 MiB (tests/depth_cases.py puts them together again).

Usage:  python tests/golden/make_depth_golden.py [--check]      (--check: compare with the committed files instead of writing)
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import make_golden as mg  # noqa: E402  (puts the reference and the stand-ins on sys.path, applies the numpy-2 patch)
import make_rays_golden as mr  # noqa: E402

MUS = [0.1, 0.6, 1.0]
BLOCK = 160           # wavelengths per file: 160 x 3 x 82 x 3 arrays x 8 B = 0.94 MB before compression


def final_pass_recorded(ctx, pops, J):
    """-> chi, S, I of the up-going rays, each [Nspect][nmu][Nspace], and ctx.I"""
    rh = sys.modules[type(ctx).__module__]
    original = rh.piecewise_linear_1d
    rec = {'chi': [], 'S': [], 'I': []}

    def recording(atmos, mu, toFrom, wav, chi, S):
        out = original(atmos, mu, toFrom, wav, chi, S)
        if toFrom:
            rec['chi'].append(np.array(chi))
            rec['S'].append(np.array(S))
            rec['I'].append(np.array(out.I))
        return out

    rh.piecewise_linear_1d = recording
    try:
        I_top = mr.final_pass(ctx, pops, J)
    finally:
        rh.piecewise_linear_1d = original
    nmu = len(ctx.atmos.muz)
    shape = (ctx.spect.wavelength.shape[0], nmu, ctx.atmos.height.shape[0])       # the calls come wavelength-major, then by ray
    return tuple(np.array(rec[k]).reshape(shape) for k in ('chi', 'S', 'I')) + (I_top,)


def block_path(name, b):
    return os.path.join(HERE, 'depth_falc_%s_%d.npz' % (name, b))


def main():
    check = '--check' in sys.argv[1:]
    cases = (('ca', ['Ca'], None, 'falc_ca.npz', 'conv', 'conv_J'),
             ('ca_vlos', ['Ca'], mr.vlos_ramp(), 'falc_ca_vlos.npz', 'se5', 'last_J'),
             ('cah', ['Ca', 'H'], None, 'falc_cah.npz', 'se5', 'last_J'))
    for name, active, vlos, fixture, ntag, jkey in cases:
        t0 = time.time()
        raw = np.load(os.path.join(HERE, fixture))
        with np.errstate(all='ignore'):
            ctx = mr.context_on_rays(active, MUS, vlos)
        pops = [raw['%s_n_a%d' % (ntag, a)] for a in range(len(ctx.activeAtoms))]
        assert [str(x) for x in raw['atom_names']] == [a.atomicModel.name for a in ctx.activeAtoms]
        assert np.array_equal(raw['wavelength'], np.array(ctx.spect.wavelength))
        chi, S, I, I_top = final_pass_recorded(ctx, pops, raw[jkey])
        assert np.array_equal(I[:, :, 0], I_top) and all(np.all(np.isfinite(a)) for a in (chi, S, I))
        print('%s: %s, min chi %.2e, min S %.2e, min I %.2e, %.1f s' % (name, I.shape, chi.min(), S.min(), I.min(), time.time() - t0),
              flush=True)
        for b, lo in enumerate(range(0, I.shape[0], BLOCK)):
            d = {'mus': np.array(MUS), 'la0': np.array(lo), 'chi': chi[lo:lo + BLOCK], 'S': S[lo:lo + BLOCK], 'I': I[lo:lo + BLOCK]}
            path = block_path(name, b)
            if check:
                old = np.load(path)
                assert sorted(old.files) == sorted(d) and all(np.array_equal(old[k], d[k]) for k in d), path
                print('  %s: identical' % os.path.basename(path))
            else:
                np.savez_compressed(path, **d)
                size = os.path.getsize(path)
                assert size <= 1 << 20, (path, size)
                print('  wrote %s (%.1f kB)' % (os.path.basename(path), size / 1e3))


if __name__ == '__main__':
    main()
