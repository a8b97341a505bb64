"""Shared cases of the arbitrary-wavelength tests (tests/test_spectrum_host.py, tests/test_spectrum.py).

The checker needs nothing new in the oracle: a zero-weight oracle context (tests/rays_cases.py) on a RE-GRIDDED problem is the
reference's computation on compute_wavelength_grid(extraWavelengths=w).  `regrid` forms the union of the context's grid and the wanted
wavelengths, gives every transition the window the reference gives it on a merged grid (atomic_set.py:401-453: lambda[Nblue] <=
lambda' <= lambda[Nblue + Nlambda - 1], ends inclusive), takes the continua's cross-sections at the wanted wavelengths as given, and
sets J and the background by the rule of include/lsx_hip_spectrum.h.  The profiles are rebuilt by the oracle from the same
(aDamp, vBroad, vlos) on the union grid."""
import dataclasses
import functools

import numpy as np

import rays_cases as rc
from conftest import golden
from lightspinner_amd import fixtures

U = 2.0 ** -52
CASES = ('ca_vlos', 'cah')


def bracket(lam, w):
    """(l, t) of include/lsx_hip_spectrum.h for the wavelengths w on the grid lam, in float64"""
    lam, w = np.asarray(lam, dtype=np.float64), np.atleast_1d(np.asarray(w, dtype=np.float64))
    N = lam.shape[0]
    if N < 2:
        return np.zeros(w.shape, dtype=np.int64), np.zeros(w.shape)
    l = np.clip(np.searchsorted(lam, w, side='right') - 1, 0, N - 2)
    t = np.clip((w - lam[l]) / (lam[l + 1] - lam[l]), 0.0, 1.0)
    return l, t


def interp_rule(lam, X, w):
    """X [..., Nspect, Nspace] on the grid lam -> [..., nla, Nspace] at w: (1 - t) X[l] + t X[l+1], two products and a sum"""
    X = np.asarray(X, dtype=np.float64)
    if len(lam) < 2:
        return np.repeat(X[..., :1, :], len(np.atleast_1d(w)), axis=-2)
    l, t = bracket(lam, w)
    return (1.0 - t)[:, None] * X[..., l, :] + t[:, None] * X[..., l + 1, :]


def windows(prob, wu):
    """every transition's (Nblue, Nlambda) on the union grid wu by the rule"""
    lam = prob.wavelength
    out = []
    for t in prob.trans:
        lo, hi = lam[t.Nblue], lam[t.Nblue + t.Nlambda - 1]
        sel = np.nonzero((wu >= lo) & (wu <= hi))[0]
        out.append((int(sel[0]), int(sel.shape[0])))
    return out


def regrid(prob, block, J, w, alpha=None, bg=None):
    """-> (problem on the union grid, its block with phi = wphi = None, J on it, rows of the wanted wavelengths in it).
    alpha: [Ncont][nla] at w (needed where the problem has continua); bg: None (interpolation mode: the block's background by the
    rule) or (bg_chi, bg_eta[, bg_sca]) of [ncol][nla][Nspace] at w."""
    lam = prob.wavelength
    w = np.atleast_1d(np.asarray(w, dtype=np.float64))
    wu = np.union1d(lam, w)
    rows = np.searchsorted(wu, w)
    own = np.searchsorted(wu, lam)
    assert np.array_equal(wu[rows], w) and np.array_equal(wu[own], lam)
    trans, active = [], np.zeros((len(prob.trans), wu.shape[0]), dtype=np.uint8)
    kc = 0
    for kr, (t, (nb, nl)) in enumerate(zip(prob.trans, windows(prob, wu))):
        t2 = dataclasses.replace(t, Nblue=nb, Nlambda=nl)
        active[kr, nb:nb + nl] = 1
        if not t.is_line:
            a = np.full(wu.shape[0], np.nan)
            a[own[t.Nblue:t.Nblue + t.Nlambda]] = t.alpha
            inw = (rows >= nb) & (rows < nb + nl)                  # (alpha outside the window is not read; a wanted wavelength that
            a[rows[inw]] = np.asarray(alpha[kc])[inw]              # is a point of the grid takes the value handed over, as the entry does)
            t2.alpha = a[nb:nb + nl].copy()
            assert np.all(np.isfinite(t2.alpha))
            kc += 1
        trans.append(t2)
    p2 = dataclasses.replace(prob, wavelength=wu.copy(), trans=trans, active=active, phi_compact=False)

    def on_union(X, given):
        Y = interp_rule(lam, X, wu)
        assert np.array_equal(Y[..., own, :], X)                   # the rule is exact at the grid's own points
        if given is not None:
            Y[..., rows, :] = given                                # (also where a wanted wavelength is a point of the grid)
        return Y
    per_la = dict(bg_chi=on_union(block.bg_chi, None if bg is None else bg[0]),
                  bg_eta=on_union(block.bg_eta, None if bg is None else bg[1]))
    if prob.sca_per_lambda:
        per_la['bg_sca'] = on_union(block.bg_sca, None if bg is None else bg[2])
    b2 = dataclasses.replace(block, phi=None, wphi=None, **per_la)
    return p2, b2, on_union(J, None), rows


def full_prof(prob, block, prof):
    """profile inputs with a velocity array (zeros where there is none): the re-gridded problem is never phi_compact"""
    aD, vB, vl = prof
    return aD, vB, (np.zeros((block.ncol, prob.Nspace)) if vl is None else vl)


def oracle_spectrum(oracle_lib, prob, block, prof, mus, n, J, w, alpha=None, bg=None, solver='linear'):
    """-> [ncol][nla][nmu]: the reference's computation at the wanted wavelengths"""
    p2, b2, J2, rows = regrid(prob, block, J, w, alpha, bg)
    return rc.oracle_rays(oracle_lib, p2, b2, full_prof(prob, block, prof), mus, n, J2, solver)[:, rows]


def envelope_spectrum(oracle_lib, prob, block, prof, mus, n, J, w, alpha=None, bg=None, solver='linear'):
    """-> (x(0), x(+1), x(-1)), each [ncol][nla][nmu]: the same with every exp(-dtau) a ulp up / down (tests/envelope.py)"""
    from lightspinner_amd import _capi
    p2, b2, J2, rows = regrid(prob, block, J, w, alpha, bg)
    runs = rc.envelope_runs(oracle_lib, p2, b2, full_prof(prob, block, prof), mus, n, J2, solver)
    return tuple(runs[u][0][_capi.LSX_I][:, rows] for u in (0, 1, -1))


def bound(x0, xp, xm, extra=0.0):
    """the bar of the GPU tests entry by entry, with the vacuity guard: a bound above 1e-8 |x| anywhere shows nothing"""
    b = (1e-11 + extra) * np.abs(x0) + 3.0 * np.abs(xp - xm)
    assert np.all(b <= 1e-8 * np.abs(x0)), 'vacuous bound: %.2e relative' % float(np.max(b / np.abs(x0)))
    return b


def interp_alpha(prob, w):
    """[Ncont][nla]: np.interp of every continuum's own cross-sections (zero outside its window): a made-up but smooth alpha'
    for the tests in which the checker is handed the same arrays"""
    lam = prob.wavelength
    out = [np.interp(w, lam[t.Nblue:t.Nblue + t.Nlambda], t.alpha, left=0.0, right=0.0) for t in prob.trans if not t.is_line]
    return np.stack(out) if out else None


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(golden('spectrum_falc.npz')))


def fixture_case(name):
    """-> (prob, block, prof, n, J, mus, dict(w, alpha, bg_chi, bg_eta, I, Nblue, Nlambda)) of a case of spectrum_falc.npz"""
    prob, block, prof, n, J, mus, _ = rc.golden_case(name)
    if prof is None:
        raw = dict(np.load(golden({'ca': 'falc_ca.npz', 'cah': 'falc_cah.npz'}[name])))
        prof = fixtures.profile_inputs(prob, raw, with_vlos=False)
    f = fixture()
    return prob, block, prof, n, J, mus, {k: np.array(f['%s_%s' % (name, k)]) for k in ('w', 'alpha', 'bg_chi', 'bg_eta', 'I', 'Nblue', 'Nlambda')}
