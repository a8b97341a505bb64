#!/usr/bin/env python3
"""Generate tests/golden/losses_falc_<case>*.npz: the radiative flux, its divergence and the per-transition net cooling as the
UNMODIFIED reference's own formal solution gives them.

As make_depth_golden.py: the name `piecewise_linear_1d` in the reference's rh_method module is replaced, for the duration of ONE
formal_sol_gamma_matrices(), by a recorder that passes everything through and keeps the `chi` and `S` it is handed and the `I` it
returns -- of BOTH directions here.  The context is test.py's own (the five-ray quadrature) holding the populations and J of a
committed state:
  ca       CaII active, vlos = 0          falc_ca.npz       conv_n_a0, conv_J
  ca_vlos  CaII active, the vlos ramp     falc_ca_vlos.npz  se5_n_a0, last_J
  cah      Ca + H active                  falc_cah.npz      se5_n_a*, last_J
A second loop over the reference's own objects (atom.setup_wavelength(la), t.uv(la, mu, toFrom), atom.wla, atom.n, the background)
forms, in the order of include/lsx_hip_losses.h's definitions (wavelength, ray, direction: down then up),
  H[la][k]  = sum  wmu/2 mu (I+ - I-)          Hg = the same with (I+ + I-)
  D[la][k]  = sum  wmu/2 (eta - chi I)         Gd = the same with (eta + chi I)
  Qt[t][k]  = sum  (hc / lambda) wlamu [n_j (Uji + Vji I) - n_i Vij I]       Qtg = the same with + n_i Vij I
  F = 4 pi sum wnu H,  Q = 4 pi sum wnu D  (Fg, Qg from Hg, Gd),  wnu the trapezoid rule in frequency over the merged grid.
The recording is asserted against what the reference itself keeps: sum wmu/2 I against ctx.J, I+[k = 0] against ctx.I, and the
recomputed chiTot against the recorded one, all bit for bit.
Numbers only are written.  F, Q, Qt, their grosses and wnu go to losses_falc_<case>.npz; H, Hg and D, Gd on every fourth wavelength
plus every wavelength of the first line's window go to losses_falc_<case>_H.npz and ..._D.npz.  No file exceeds 1 MiB.

Usage:  python tests/golden/make_losses_golden.py [--check] [case ...]     (--check: compare with the committed files instead of writing)
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import make_golden as mg  # noqa: E402  (puts the reference and the stand-ins on sys.path, applies the numpy-2 patch)
import make_rays_golden as mr  # noqa: E402

import constants as Const  # noqa: E402  (the reference's)

CASES = (('ca', ['Ca'], False, 'falc_ca.npz', 'conv', 'conv_J'),
         ('ca_vlos', ['Ca'], True, 'falc_ca_vlos.npz', 'se5', 'last_J'),
         ('cah', ['Ca', 'H'], False, 'falc_cah.npz', 'se5', 'last_J'))


def trapezoid_wnu(wavelength):
    """nu = c / lambda; wnu[la] = |nu[la - 1] - nu[la + 1]| / 2, half intervals at the two ends"""
    nu = Const.CLight / (np.asarray(wavelength, dtype=np.float64) * Const.NM_TO_M)
    w = np.empty_like(nu)
    if nu.shape[0] == 1:
        w[0] = 0.0
        return w
    w[0] = 0.5 * abs(nu[0] - nu[1])
    w[-1] = 0.5 * abs(nu[-2] - nu[-1])
    w[1:-1] = 0.5 * np.abs(nu[:-2] - nu[2:])
    return w


def recorded_call(ctx, pops, J):
    """one formal_sol_gamma_matrices() from (pops, J) -> chi, S, I [Nspect][Nrays][2][Nspace] (direction 0 down, 1 up)"""
    rh = sys.modules[type(ctx).__module__]
    original = rh.piecewise_linear_1d
    rec = {'chi': [], 'S': [], 'I': []}

    def recording(atmos, mu, toFrom, wav, chi, S):
        out = original(atmos, mu, toFrom, wav, chi, S)
        rec['chi'].append(np.array(chi))
        rec['S'].append(np.array(S))
        rec['I'].append(np.array(out.I))
        return out

    for atom, n in zip(ctx.activeAtoms, pops):
        atom.n[...] = n
    ctx.J[...] = J
    rh.piecewise_linear_1d = recording
    try:
        ctx.formal_sol_gamma_matrices()
    finally:
        rh.piecewise_linear_1d = original
    shape = (ctx.spect.wavelength.shape[0], ctx.atmos.Nrays, 2, ctx.atmos.Nspace)      # the calls come by wavelength, ray, direction
    return tuple(np.array(rec[k]).reshape(shape) for k in ('chi', 'S', 'I'))


def losses(ctx, JDag, chi_rec, I_rec):
    """the second loop: the reference's own objects, rh_method.py:595-632 and :661-667 restated around the recorded I"""
    atmos, spect, bg = ctx.atmos, ctx.spect, ctx.background
    Nspect, Ns = spect.wavelength.shape[0], atmos.Nspace
    trans = [t for a in ctx.activeAtoms for t in a.trans]
    H, Hg, D, Gd = (np.zeros((Nspect, Ns)) for _ in range(4))
    Qt, Qtg = np.zeros((len(trans), Ns)), np.zeros((len(trans), Ns))
    for la, wav in enumerate(spect.wavelength):
        for atom in ctx.activeAtoms:
            atom.setup_wavelength(la)
        e_phot = Const.HC / (wav * Const.NM_TO_M)
        for mu in range(atmos.Nrays):
            hw = 0.5 * atmos.wmu[mu]
            for toFrom, sign in enumerate([-1.0, 1.0]):
                chiTot, etaTot = np.zeros(Ns), np.zeros(Ns)
                for atom in ctx.activeAtoms:
                    for t in atom.trans:
                        if not t.active[la]:
                            continue
                        uv = t.uv(la, mu, toFrom)
                        chiTot += atom.n[t.i] * uv.Vij - atom.n[t.j] * uv.Vji
                        etaTot += atom.n[t.j] * uv.Uji
                chiTot += bg.chi[la]
                eta = etaTot + bg.eta[la] + bg.sca[la] * JDag[la]
                assert np.array_equal(chiTot, chi_rec[la, mu, toFrom])
                I = I_rec[la, mu, toFrom]
                H[la] += hw * atmos.muz[mu] * sign * I
                Hg[la] += hw * atmos.muz[mu] * I
                D[la] += hw * (eta - chiTot * I)
                Gd[la] += hw * (eta + chiTot * I)
                kt = 0
                for atom in ctx.activeAtoms:
                    for kr, t in enumerate(atom.trans):
                        if t.active[la]:
                            wlamu = atom.wla[kr] * hw * 4 * np.pi
                            uv = t.uv(la, mu, toFrom)
                            down = atom.n[t.j] * (uv.Uji + uv.Vji * I)
                            up = atom.n[t.i] * uv.Vij * I
                            Qt[kt + kr] += e_phot * wlamu * (down - up)
                            Qtg[kt + kr] += e_phot * wlamu * (down + up)
                    kt += len(atom.trans)
    return H, Hg, D, Gd, Qt, Qtg


def sample(ctx):
    """every fourth wavelength and every wavelength of the first line's window"""
    t = next(t for a in ctx.activeAtoms for t in a.trans if t.isLine)
    Nspect = ctx.spect.wavelength.shape[0]
    return np.unique(np.concatenate([np.arange(0, Nspect, 4), np.arange(t.Nblue, t.Nblue + t.wavelength.shape[0])])).astype(np.int32)


def main():
    args = sys.argv[1:]
    check = '--check' in args
    wanted = [a for a in args if not a.startswith('--')]
    for name, active, vlos, fixture, ntag, jkey in CASES:
        if wanted and name not in wanted:
            continue
        t0 = time.time()
        raw = np.load(os.path.join(HERE, fixture))
        ctx = mg.build_ctx(active, vlos=mr.vlos_ramp() if vlos else None)
        pops = [raw['%s_n_a%d' % (ntag, a)] for a in range(len(ctx.activeAtoms))]
        assert [str(x) for x in raw['atom_names']] == [a.atomicModel.name for a in ctx.activeAtoms]
        assert np.array_equal(raw['wavelength'], np.array(ctx.spect.wavelength))
        JDag = np.array(raw[jkey])
        chi, S, I = recorded_call(ctx, pops, JDag)
        # the recording against what the reference itself keeps
        Jrec = np.zeros_like(ctx.J)
        for mu in range(ctx.atmos.Nrays):
            for d in range(2):
                Jrec += 0.5 * ctx.atmos.wmu[mu] * I[:, mu, d]
        assert np.array_equal(Jrec, ctx.J) and np.array_equal(I[:, :, 1, 0], ctx.I)
        H, Hg, D, Gd, Qt, Qtg = losses(ctx, JDag, chi, I)
        wnu = trapezoid_wnu(ctx.spect.wavelength)
        four_pi = 4 * np.pi
        idx = sample(ctx)
        files = {
            '': {'wnu': wnu, 'F': four_pi * (wnu @ H), 'Fg': four_pi * (wnu @ Hg), 'Q': four_pi * (wnu @ D), 'Qg': four_pi * (wnu @ Gd),
                 'Qt': Qt, 'Qtg': Qtg, 'I_top': np.array(ctx.I), 'J_pass': np.array(ctx.J), 'la_idx': idx},
            '_H': {'la_idx': idx, 'H': H[idx], 'Hg': Hg[idx]},
            '_D': {'la_idx': idx, 'D': D[idx], 'Gd': Gd[idx]},
        }
        assert all(np.all(np.isfinite(v)) for d in files.values() for v in d.values())
        print('%s: Nspect %d, %d sampled, F[0] %.4e W m-2, max |Q| / Qg %.2e at the top, %.2e at the bottom, %.1f s'
              % (name, H.shape[0], idx.shape[0], files['']['F'][0], abs(files['']['Q'][0]) / files['']['Qg'][0],
                 abs(files['']['Q'][-1]) / files['']['Qg'][-1], time.time() - t0), flush=True)
        for suffix, d in files.items():
            path = os.path.join(HERE, 'losses_falc_%s%s.npz' % (name, suffix))
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
