"""The HIP library's Voigt function (lsx_voigt.h: dev_voigt) against mpmath over the whole (a, v) plane, where it reads its table from
global memory (k_voigt_block, k_voigt_wphi: Engine.set_line_profiles) and from LDS (k_depth_rays: Engine.depth_rays at angles that are
not the quadrature's); and k_emergent_rays, k_spectrum and the depth pass on FALC columns whose damping is scaled across 2 pi,
against the oracle's zero-weight context.  tests/voigt_cases.py holds the reference, the bars and the made-up problem; every entry is checked."""
import numpy as np
import pytest

import depth_cases as dc
import voigt_cases as vc
from lightspinner_amd import _capi
from lightspinner_amd.problem import Engine

pytestmark = pytest.mark.gpu
MUS_DEPTH = {1: np.array([0.83]), 7: np.array([0.05, 0.21, 0.4, 0.55, 0.7, 0.93, 1.0])}      # 0.05: a grazing ray


def profiles(lib, prob, block, prof, **kw):
    e = Engine(prob, block.ncol, lib=lib, **kw)
    e.set_columns(0, block)
    e.set_line_profiles(0, *prof)
    out = e.get(_capi.LSX_PHI), e.get(_capi.LSX_WPHI)
    e.close()
    return out


@pytest.mark.parametrize('tiler', ['dp', 'natural'])        # natural: line A is cut at wavelength 21 into pieces of 3 and 12
@pytest.mark.parametrize('ncol,Ns,compact', vc.CASES)
def test_hip_profile_chain_over_the_plane(hip_lib, oracle_lib, ncol, Ns, compact, tiler):
    prob, block, prof = vc.probe(ncol, Ns, compact)
    phi, wphi = profiles(hip_lib, prob, block, prof, options=dict(tiler=tiler))
    r, where = vc.excess_phi(phi, vc.phi_reference(ncol, Ns, compact))
    wref, wbar = vc.wphi_reference(ncol, Ns, compact)
    rw = float(np.max(np.abs(wphi - wref) / wref))
    ophi, owphi = profiles(oracle_lib, prob, block, prof)
    big = ophi >= vc.TINY
    ro = float(np.max(np.abs(phi - ophi)[big] / ophi[big]))
    rwo = float(np.max(np.abs(wphi - owphi) / owphi))
    print('HIP phi: %.3f x the bar against mpmath at %s, %.2e relative against the oracle; wphi %.2e against mpmath (bar %.2e), %.2e '
          'against the oracle' % (r, where, ro, rw, wbar, rwo))
    assert r <= 1.0, (r, where)
    assert rw <= wbar
    assert ro <= 1e-13 and rwo <= 1e-13 and np.all(np.abs(phi - ophi)[~big] <= vc.TINY)


def line_response(prob, n, dphi, nmu, la):
    """(d chi, d eta) [nmu][Nspace] at wavelength la for a change dphi >= 0 of every line's up-going profile: chi and eta are linear
    in phi (rh_method.py:279-281, :613-614)"""
    hc_4pi = 0.25 * 6.62607004e-34 * 2.99792458e8 / np.pi
    dchi, deta = np.zeros((nmu, prob.Nspace)), np.zeros((nmu, prob.Nspace))
    off = dc.phi_offsets(prob)
    for kr, t in enumerate(prob.trans):
        if not (t.is_line and prob.active[kr, la]):
            continue
        o = int(prob.lev_off[t.atom])
        ni, nj = n[o + t.i], n[o + t.j]
        d = dphi[off[kr] + la - t.Nblue][:, 1, :]
        dchi += hc_4pi * t.Bij * np.abs(ni - (t.Bji / t.Bij) * nj) * d
        deta += nj * (t.Aji / t.Bji) * (t.Bji / t.Bij) * hc_4pi * t.Bij * d
    return dchi, deta


@pytest.mark.parametrize('nmu', sorted(MUS_DEPTH))
def test_depth_rays_evaluate_the_true_function(hip_lib, nmu):
    """k_depth_rays forms the profile in the lane from the LDS copy of the table: chi and S against the numpy restatement fed with
    MPMATH profiles at the angles.  Bar: depth_cases' 1e-12 plus the conditioning term carried through chi's (and eta's) linear
    dependence on phi."""
    ncol, Ns = 3, 13
    mus = MUS_DEPTH[nmu]
    prob, block, prof = vc.probe(ncol, Ns, False)
    e = Engine(prob, ncol, lib=hip_lib)
    e.set_columns(0, block)
    e.set_line_profiles(0, *prof)
    J = 0.5 * block.bg_eta / block.bg_chi
    e.set(_capi.LSX_J, J)
    n = e.get(_capi.LSX_N)
    d = e.depth_rays(mus, what=('chi', 'S'))
    e.close()
    hi, lo, bar = vc.phi_reference(ncol, Ns, False, mus=mus, both=False)         # [ncol][SNl][nmu][1][Ns]: the up-going direction
    worst = 0.0
    for c in range(ncol):
        phi = np.repeat(hi[c] + lo[c], 2, axis=2)                                 # restate_chi_S reads index 1 of the direction axis
        chi_r, S_r = dc.restate_chi_S(prob, block, n[c], J[c], phi, nmu, col=c)
        chi, S = dc.to_lambda_major(d.chi[c]), dc.to_lambda_major(d.S[c])
        dphi = np.repeat(bar[c] - vc.BAR * np.abs(hi[c]), 2, axis=2).clip(min=0.0)  # the conditioning part of the profile's bar
        for la in range(prob.Nspect):
            dchi, deta = line_response(prob, n[c], dphi, nmu, la)
            eta_r = S_r[la] * chi_r[la]
            bchi = dc.BASE_CHI_S * np.abs(chi_r[la]) + dchi
            bS = dc.BASE_CHI_S * np.abs(S_r[la]) + (deta + np.abs(S_r[la]) * dchi) / np.abs(chi_r[la])
            assert np.all(chi_r[la] > 0) and np.all(eta_r > 0)
            worst = max(worst, float(np.max(np.abs(chi[la] - chi_r[la]) / bchi)), float(np.max(np.abs(S[la] - S_r[la]) / bS)))
    print('depth_rays nmu = %d: chi, S %.3f x the bar against the restatement on mpmath profiles' % (nmu, worst))
    assert worst <= 1.0


# ---- k_emergent_rays, k_spectrum and the depth pass on a damped batch: real atoms across a = 2 pi ---------------------------------
# These return intensities only: the checker is the zero-weight oracle context (tests/rays_cases.py, tests/spectrum_cases.py) under
# the existing envelope bars -- and tests/test_voigt_plane_host.py holds that oracle's Voigt function to mpmath.
DAMP_SCALE = np.array([1.0, 1.03, 2.0, 10.0, 100.0, 1e-3, 1e-6])       # per column, on every line's aDamp


@pytest.fixture(scope='module')
def damped(hip_lib):
    import rays_cases as rc
    from lightspinner_amd import synth
    prob, block, (aD, vB, vlos) = rc.batch('falc_cah.npz', DAMP_SCALE.shape[0])
    prof = (aD * DAMP_SCALE[:, None, None], vB, vlos)
    amax = prof[0].max(axis=(1, 2))
    assert int(np.sum(amax >= vc.TWO_PI)) == 4 and amax[0] < vc.TWO_PI and prof[0][6].max() < 1e-5      # FALC itself stops at 6.142
    e = Engine(prob, block.ncol, lib=hip_lib)
    synth.load_columns(e, block, prof)
    rc.mali(e)
    yield prob, block, prof, e, e.get(_capi.LSX_N), e.get(_capi.LSX_J)
    e.close()


def test_emergent_rays_on_the_damped_batch(damped, oracle_lib):
    import envelope
    import rays_cases as rc
    prob, block, prof, e, n, J = damped
    mus = rc.MUS20[::3]
    I = e.emergent_rays(mus)
    runs = rc.envelope_runs(oracle_lib, prob, block, prof, mus, n, J)
    assert np.all(np.isfinite(I)) and np.all(I > 0)
    rel, renv = envelope.inside(I, runs, 0, _capi.LSX_I, base=1e-11)
    per = np.max(np.abs(I - runs[0][0][_capi.LSX_I]) / np.abs(runs[0][0][_capi.LSX_I]), axis=(1, 2))
    print('emergent_rays, damped batch: %.2e relative at worst (envelope up to %.2e); per column %s' % (rel, renv, ' '.join('%.1e' % x for x in per)))


def test_spectrum_on_the_damped_batch(damped, oracle_lib):
    """a Ly-alpha window and points far in its wing, and the window of the line with FALC's largest damping (4052 nm: a = 6.14 x the
    column's factor, so k_spectrum takes a >= 2 pi in four columns)"""
    import spectrum_cases as sc
    prob, block, prof, e, n, J = damped
    lya = next(t for t in prob.lines if abs(t.lambda0 - 121.568) < 0.01)
    top = prob.lines[int(np.argmax(prof[0][0].max(axis=1)))]
    assert abs(top.lambda0 - 4052.29) < 0.01
    lam = prob.wavelength
    w = np.unique(np.concatenate([lya.lambda0 + np.linspace(-0.06, 0.06, 41), lya.lambda0 + np.array([-0.7, -0.6, -0.3, 0.3, 0.6, 0.7]),
                                  [lam[lya.Nblue], lam[lya.Nblue + lya.Nlambda - 1]],
                                  top.lambda0 + np.linspace(-1.2, 1.2, 25)]))
    mus = np.array([0.1, 0.25, 0.47, 0.6, 0.88, 1.0])
    alpha = sc.interp_alpha(prob, w)
    got = e.emergent_spectrum(mus, w, alpha=alpha)
    x0, xp, xm = sc.envelope_spectrum(oracle_lib, prob, block, prof, mus, n, J, w, alpha, None)
    b = sc.bound(x0, xp, xm)
    dev = np.abs(got - x0)
    print('spectrum, damped batch: %.2e relative at worst, %.3f x the bound; per column %s'
          % (float(np.max(dev / np.abs(x0))), float(np.max(dev / b)), ' '.join('%.1e' % x for x in np.max(dev / np.abs(x0), axis=(1, 2)))))
    assert got.shape == x0.shape and np.all(np.isfinite(got))
    assert np.all(dev <= b)


def test_depth_pass_on_the_damped_batch(damped, hip_lib, oracle_lib):
    """the depth pass against its own checkers (tests/test_depth_rays.py: check_column), in the windows of Ly-alpha and of the line
    with the largest damping"""
    from test_depth_rays import check_column
    prob, block, prof, e, n, J = damped
    mus = np.concatenate([prob.muz, [0.33]])
    phi = dc.profiles_at(hip_lib, prob, block, prof, mus)
    for t in (prob.lines[0], prob.lines[9]):
        d = e.depth_rays(mus, la0=t.Nblue, nla=t.Nlambda)
        for c in range(block.ncol):
            check_column('damped batch %.0f nm column %d' % (t.lambda0, c), oracle_lib, prob, block, c, n[c], J[c], phi[c], d, c, la0=t.Nblue)
