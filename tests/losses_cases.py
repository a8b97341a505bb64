"""Shared cases of the radiative-losses tests (tests/test_radiative_losses_host.py, tests/test_radiative_losses.py).

The pin: tests/golden/losses_falc_<case>*.npz hold what the unmodified reference's own formal solution gives for the flux, its
divergence and the per-transition cooling on three committed states (tests/golden/make_losses_golden.py), with the GROSS of every
quantity beside it: Hg = sum wmu/2 mu (I+ + I-), Gd = sum wmu/2 (eta + chi I), Qtg = the bracket with + n_i Vij I, Fg and Qg from
those.  Deep down eta - chi I cancels to nothing, so every comparison is relative to the gross, never to the value.

The bar of a quantity x with gross g:   |x - x_ref| <= BASE g + K_ENVELOPE L(|J(+1) - J(-1)|)
where J(+-1) is the mean intensity of the pass in the oracle's runs with every exp(-dtau) a ulp up / down (rates_cases.oracle_runs)
and L is the quantity's own linear dependence on the intensity with every coefficient taken positive:
  D[la][k]    chi |dJ|             where chi depends on the ray (line profiles with a velocity): its largest value over rays and
                                   directions (`chi_max`)
  H[la][k]    |dJ|                 H = sum wmu/2 mu (+-I) and mu <= 1: the flux cannot move by more than the mean intensity does
  Q, F        4 pi sum |wnu| L_D,  4 pi sum |wnu| L_H
  Qt[t][k]    sum_{la in t} (hc / lambda) 4 pi wla |n_j Vji - n_i Vij| |dJ|        (`qt_coefficients`, the profile averaged over
              rays and directions with wmu/2)
BASE and K_ENVELOPE are the suite's (rates_cases.BASE, envelope.K_ENVELOPE)."""
import functools

import numpy as np

import envelope
import rates_cases as rt
from conftest import golden
from depth_cases import phi_offsets
from lightspinner_amd import _capi, fixtures
from lightspinner_amd import constants as Const

CASES = ('ca', 'ca_vlos', 'cah')
BASE = rt.BASE
K_ENVELOPE = envelope.K_ENVELOPE
FOUR_PI = 4.0 * np.pi
STATES = {'ca': ('falc_ca.npz', 'conv', 'conv_J'), 'ca_vlos': ('falc_ca_vlos.npz', 'se5', 'last_J'), 'cah': ('falc_cah.npz', 'se5', 'last_J')}


@functools.lru_cache(maxsize=None)
def fixture(case):
    """-> the arrays of tests/golden/losses_falc_<case>.npz, _H.npz and _D.npz in one dict (read-only)"""
    out = {}
    for suffix in ('', '_H', '_D'):
        part = np.load(golden('losses_falc_%s%s.npz' % (case, suffix)))
        for k in part.files:
            if k in out:
                assert np.array_equal(out[k], part[k]), k
            out[k] = np.array(part[k])
    for a in out.values():
        a.setflags(write=False)
    return out


def state(case, phi_compact=None):
    """the state a fixture was made from -> (prob, block, prof, n [1][NLtot][Ns], J [1][Nspect][Ns]); phi_compact=False: the
    profiles of a vlos = 0 case in the ray-dependent store layout"""
    fx, ntag, jkey = STATES[case]
    prob, block, raw = fixtures.load_problem_npz(golden(fx), phi_compact=phi_compact)
    prof = fixtures.profile_inputs(prob, raw) if block.phi is None else None
    return prob, block, prof, fixtures.pops_from_raw(raw, ntag, prob)[None], np.array(raw[jkey])[None]


def trapezoid_wnu(wavelength):
    """numpy restatement of include/lsx_hip_losses.h: nu = c / lambda, |nu[la - 1] - nu[la + 1]| / 2, half intervals at the ends"""
    nu = Const.CLight / (np.asarray(wavelength, dtype=np.float64) * Const.NM_TO_M)
    w = np.zeros_like(nu)
    if nu.shape[0] > 1:
        w[0], w[-1] = 0.5 * abs(nu[0] - nu[1]), 0.5 * abs(nu[-2] - nu[-1])
        w[1:-1] = 0.5 * np.abs(nu[:-2] - nu[2:])
    return w


def half_weights(prob):
    return 0.5 * np.asarray(prob.wmu, dtype=np.float64)


def weight_sum(prob):
    """sum of wmu / 2 over rays and directions"""
    return 2.0 * float(np.sum(half_weights(prob)))


def mean_profile(prob, phi):
    """LSX_PHI of one column -> [SNl][Nspace]: sum over rays and directions of (wmu / 2) phi"""
    if prob.phi_compact:
        return np.asarray(phi) * weight_sum(prob)
    return np.einsum('m,lmdk->lk', half_weights(prob), np.asarray(phi))


def qt_coefficients(prob, block, n, phi, wphi, col=0):
    """per transition (slice of the merged grid, c [Nlambda][Nspace]): Qt's dependence on the intensity with every coefficient
    positive, c = (hc / lambda) 4 pi wla |n_j Vji - n_i Vij| summed over rays and directions with wmu / 2.
    n [NLtot][Ns]; phi, wphi: LSX_PHI and LSX_WPHI of that column"""
    pbar, poff = mean_profile(prob, phi), phi_offsets(prob)
    hc_k = Const.HC / (Const.KBoltzmann * Const.NM_TO_M)
    out, line = [], 0
    for kr, t in enumerate(prob.trans):
        sl = slice(t.Nblue, t.Nblue + t.Nlambda)
        lam = prob.wavelength[sl]
        act = prob.active[kr, sl].astype(bool)
        o = int(prob.lev_off[t.atom])
        ni, nj = n[o + t.i], n[o + t.j]
        e_phot = Const.HC / (lam * Const.NM_TO_M)
        if t.is_line:
            wla = rt.wlambda(prob, t)[:, None] * np.asarray(wphi)[line][None, :] / Const.HC
            Vij = 0.25 * Const.HC / np.pi * t.Bij * pbar[poff[kr]:poff[kr] + t.Nlambda]
            c = np.abs(nj[None] * (t.Bji / t.Bij) - ni[None]) * Vij
            line += 1
        else:
            wla = (rt.wlambda(prob, t) / lam / Const.HPlanck)[:, None]
            g = (block.nStar[col, o + t.i] / block.nStar[col, o + t.j])[None] * np.exp(-hc_k / lam[:, None] / block.temperature[col][None])
            c = np.abs(nj[None] * g - ni[None]) * np.asarray(t.alpha, dtype=np.float64)[:, None] * weight_sum(prob)
        out.append((sl, np.where(act[:, None], e_phot[:, None] * FOUR_PI * wla * c, 0.0)))
    return out


def chi_max(prob, block, n, phi, col=0):
    """-> [Nspect][Nspace]: the opacity of rh_method.py:613-630 with every transition's share taken positive and, where the profile
    depends on the ray, its largest value over rays and directions: no ray's chi exceeds it.  n [NLtot][Ns]; phi: LSX_PHI of the column"""
    pmax = np.asarray(phi) if prob.phi_compact else np.max(np.asarray(phi), axis=(1, 2))
    poff = phi_offsets(prob)
    hc_k = Const.HC / (Const.KBoltzmann * Const.NM_TO_M)
    out = np.array(block.bg_chi[col], dtype=np.float64)
    for kr, t in enumerate(prob.trans):
        sl = slice(t.Nblue, t.Nblue + t.Nlambda)
        lam = prob.wavelength[sl]
        act = prob.active[kr, sl].astype(bool)[:, None]
        o = int(prob.lev_off[t.atom])
        ni, nj = n[o + t.i][None], n[o + t.j][None]
        if t.is_line:
            c = np.abs(ni - nj * (t.Bji / t.Bij)) * (0.25 * Const.HC / np.pi * t.Bij) * pmax[poff[kr]:poff[kr] + t.Nlambda]
        else:
            g = (block.nStar[col, o + t.i] / block.nStar[col, o + t.j])[None] * np.exp(-hc_k / lam[:, None] / block.temperature[col][None])
            c = np.abs(ni - nj * g) * np.asarray(t.alpha, dtype=np.float64)[:, None]
        out[sl] += np.where(act, c, 0.0)
    return out


def qt_envelope(coefs, dJ):
    """-> [Ntrans][Nspace]: the coefficients of `qt_coefficients` applied to |J(+1) - J(-1)| [Nspect][Nspace]"""
    return np.stack([np.sum(c * dJ[sl], axis=0) for sl, c in coefs])


def pass_envelope(oracle_lib, prob, block, prof, n, J, solver='linear'):
    """-> (|J(+1) - J(-1)| [ncol][Nspect][Nspace], J of the oracle's plain pass) from (n, J)"""
    runs = rt.oracle_runs(oracle_lib, prob, block, prof, n, J, solver)
    return envelope.envelope(runs, 0, _capi.LSX_J), runs[0][0][_capi.LSX_J]


# ---- the made-up cases (tests/final_pass_cases.py) with vlos = 0: 1, 3, 5 and 7 rays, and the three-depth column ------------------------
FIVE_RAYS = 'r5-chained'
MADE_UP = ('r1-sca', 'r3-dead-level', FIVE_RAYS, 'r7-multiplet3', 'deepest3-r7')


@functools.lru_cache(maxsize=None)
def made_up(name):
    """-> (prob, block without profile arrays, profile inputs with a zero velocity, the state to reach): the library builds the
    profiles, which then do not depend on the ray in either store layout.  final_pass_cases has no five-ray problem: FIVE_RAYS is
    toy_problem at five rays, 26 depths and 100 wavelengths (two wavefronts, the second with 36 lanes)"""
    import final_pass_cases as fp
    if name == FIVE_RAYS:
        from toy import toy_problem
        prob, block = toy_problem(seed=51, Nrays=5, Nspace=26, Nspect=100)
        how = 'mali'
    else:
        prob, block = fp.build(name)
        how = fp.BY_NAME[name].state
    blk, (aD, vB, vl) = fp.library_profiles(prob, block)
    return prob, blk, (aD, vB, None if prob.phi_compact else np.zeros_like(vl)), how


def ratio(tag, what, x, ref, gross, env):
    """|x - ref| as a multiple of BASE gross + K_ENVELOPE env, the largest over the entries; printed with the largest deviation
    relative to the gross"""
    x, ref, gross, env = (np.asarray(a, dtype=np.float64) for a in (x, ref, gross, env))
    assert x.shape == ref.shape and np.all(np.isfinite(x)), (tag, what, x.shape, ref.shape)
    assert np.all(gross > 0), (tag, what)
    bound = BASE * gross + K_ENVELOPE * env
    dev = np.abs(x - ref)
    r = float(np.max(dev / bound))
    print('%s %s: largest deviation %.2e of the gross, largest envelope %.2e of the gross, %.3f x the bound'
          % (tag, what, float(np.max(dev / gross)), float(np.max(env / gross)), r))
    return r
