"""The oracle's Voigt function (oracle/lsx_oracle.c: voigt_H) and its profile chain (lsx_set_line_profiles) against mpmath over the
whole (a, v) plane: tests/voigt_cases.py holds the reference, the bar and the made-up problem.  Bars: the bare function 1e-13 H_ref
(a and v are handed over exactly); phi 1e-13 H_ref + |dH/dv| 4 u (|v0| + |shift|) entry by entry; wphi 1e-13 + (N_terms + 2) u."""
import ctypes as C

import numpy as np
import pytest

import voigt_cases as vc
from lightspinner_amd import _capi
from lightspinner_amd.problem import Engine

A_GRID = (0.0, 1e-12, 1e-8, 1e-5, 1e-3, 0.03, 0.5, 1.0, 3.0, 5.0, 6.0, 6.28, float(np.nextafter(vc.TWO_PI, 0.0)), vc.TWO_PI,
          float(np.nextafter(vc.TWO_PI, 7.0)), 6.3, 7.0, 3 * np.pi, 4 * np.pi, 30.0, 1e3, 1e6)


def v_grid():
    """k/2 + {0, 1/8-, 1/8, 1/4, 0.3, 3/8-, 3/8, 0.01} for k < 16 and every fourth k < 60 (both grids, either side of each switch), round x = 27, far wings"""
    dn = lambda x: float(np.nextafter(x, 0.0))
    v = [0.5 * k + o for k in list(range(16)) + list(range(16, 60, 4)) for o in (0.0, dn(0.125), 0.125, 0.25, 0.3, dn(0.375), 0.375, 0.01)]
    return np.array(v + [26.9, dn(27.0), 27.0, 27.1, 40.0, 100.0, 1e3, 1e5, 1e8])


def voigt(oracle_lib):
    f = oracle_lib.dll.lsx_oracle_voigt
    f.restype = C.c_double
    f.argtypes = [C.c_double, C.c_double]
    return f


def test_the_reference_checks_itself():
    """a few dozen points a second time: at twice the digits, and by the other route where both apply -- 1e-25 relative"""
    pts = [(a, x) for a in (1e-12, 1e-8, 1e-3, 0.5, 3.0, 6.3) for x in (0.0, 0.3, 5.3, 11.9, 13.6, 20.0)] + [(1e-12, 27.0), (3.0, 30.0)]
    pts += [(a, x) for a in (1e-12, 1e-5, 1.0, 12.0, 30.0, 1e3) for x in (12.5, 14.0, 100.0)]
    worst = 0.0
    for a, x in pts:
        H, dH = vc.H_both(a, x)
        H2, dH2 = vc.H_both(a, x, scale=2)
        worst = max(worst, float(abs(H - H2) / H2), float(abs(dH - dH2) / abs(dH2)) if dH2 != 0 else float(abs(dH)))
    both = [(a, x) for a in (1e-12, 1e-5, 0.5, 1.0, 6.3) for x in (12.5, 14.0, 17.3)] + [(12.0, 0.3), (13.0, 2.0), (20.0, 5.0)]
    for a, x in both:
        Hs, He = vc.H_ref(a, x, route='series'), vc.H_ref(a, x, route='erfc')
        worst = max(worst, float(abs(Hs - He) / He))
    print('reference against itself: %.2e relative at worst over %d points' % (worst, len(pts) + len(both)))
    assert worst <= 1e-25


def test_oracle_voigt_over_the_plane(oracle_lib):
    f = voigt(oracle_lib)
    v = v_grid()
    worst = {}
    for a in A_GRID:
        for x in v:
            got = f(a, x)
            assert np.isfinite(got) and f(a, -x) == got, (a, x)           # H(a, -v) == H(a, v) bitwise
            r, rel = vc.excess_H(got, a, float(x))
            key = ('a < 1e-5' if a < 1e-5 else 'a < 2 pi' if a < vc.TWO_PI else 'a >= 2 pi', 'x < 27' if x < 27.0 else 'x >= 27')
            worst[key] = max(worst.get(key, 0.0), rel)
            assert r <= 1.0, 'H(%r, %r) = %r: %.2f x the bar (%.2e relative)' % (a, x, got, r, rel)
            if a > 0.0 and (a >= vc.TWO_PI or x >= 27.0) and x <= 1e8:
                # no pole term: H is (h a / pi) times a sum of 28 positive terms.  A term: exp(-g^2) within an ulp (2 u; g^2 is exact),
                # x - g, its square, a^2, their sum and the division (5 u); 27 additions of positive numbers (27 u); the factor (3 u).
                # 37 u at the very worst: held to 40 u = 4.4e-15 instead of the 1e-13 of the plane
                assert rel <= 40 * vc.U, 'H(%r, %r) = %r: %.2e relative where only the sum is evaluated' % (a, x, got, rel)
    print('oracle voigt_H against mpmath, largest relative deviation: ' + '; '.join('%s, %s: %.2e' % (k + (w,)) for k, w in sorted(worst.items())))
    # a = 0 is the Gaussian (numpy's own exp(-x * x) is off by x^2 u: looked at where that is far below the bar)
    for x in v[v < 10.0]:
        assert abs(f(0.0, x) - np.exp(-x * x)) <= 1e-13 * np.exp(-x * x), x
    for x in (1e8, 1e200):
        assert np.isfinite(f(1e-300, x)) and f(1e-300, x) >= 0.0


def test_the_probes_cover_the_plane():
    per_case = []
    for case in vc.CASES:
        prob, block, prof = vc.probe(*case)
        per_case.append(vc.samples(prob, prof))
        vc.assert_coverage(vc.coverage(per_case[-1]))                       # every probe alone
    cov = vc.coverage(per_case)
    print('samples per cell (rows: a = 0, decades 1e-12 .. 1e3; columns: x < 1, 3, 7, 27, 1e3, beyond):\n%s' % cov['cells'])
    print({k: v for k, v in cov.items() if k != 'cells'})
    vc.assert_coverage(cov)


@pytest.mark.parametrize('ncol,Ns,compact', vc.CASES)
def test_oracle_profile_chain_over_the_plane(oracle_lib, ncol, Ns, compact):
    prob, block, prof = vc.probe(ncol, Ns, compact)
    e = Engine(prob, ncol, lib=oracle_lib)
    e.set_columns(0, block)
    e.set_line_profiles(0, *prof)
    phi, wphi = e.get(_capi.LSX_PHI), e.get(_capi.LSX_WPHI)
    e.close()
    r, where = vc.excess_phi(phi, vc.phi_reference(ncol, Ns, compact))
    wref, wbar = vc.wphi_reference(ncol, Ns, compact)
    rw = float(np.max(np.abs(wphi - wref) / wref))
    print('oracle phi: %.3f x the bar at %s; wphi %.2e relative (bar %.2e)' % (r, where, rw, wbar))
    assert r <= 1.0, (r, where)
    assert rw <= wbar
