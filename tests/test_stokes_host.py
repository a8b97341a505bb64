"""The polarised final pass without a GPU (include/lsx_hip_stokes.h): the Zeeman patterns of lightspinner_amd/zeeman.py against the
reference's (tests/golden/zeeman_patterns.npz), the Faraday-Voigt function against mpmath, the geometry, the properties of the
propagation matrix and the DELO-linear solve on the host build of the kernel's formulas (liblsx_stokes_host.so), and the entry's
hygiene: header, export, binding, resource report, the sanitized stand-alone program."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import stokes_cases as sc
import voigt_cases as vc
from conftest import ROOT, golden
from lightspinner_amd import _capi, zeeman

CSRC = sc.CSRC
ENTRIES = {'lsx_hip_stokes_rays', 'lsx_hip_stokes_rays_work_cap'}


@pytest.fixture(scope='module')
def host():
    return sc.HostLib()


def ulps(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.spacing(np.abs(b)), 5e-324))) if a.size else 0.0


# ---- 1. patterns ----------------------------------------------------------------------------------------------------------------------
class _Level:
    def __init__(self, q, ls):
        self.J, self.L, self.S = (None, None, None) if np.isnan(q[0]) else (Fraction(q[0]).limit_denominator(2), int(q[1]), Fraction(q[2]).limit_denominator(2))
        self.lsCoupling = bool(ls)


def test_patterns_are_the_references():
    """every line of the five atoms of rh_atoms.py, as it is and with gLandeEff set to two values, and one line without quantum
    numbers: alpha exactly, strength, shift and the effective Lande factor to 4 ulp"""
    g = np.load(golden('zeeman_patterns.npz'))
    assert os.path.getsize(golden('zeeman_patterns.npz')) < 200000
    n = g['has'].shape[0]
    assert n == 184 and int(np.max(np.diff(g['ptr']))) == 27 and set(g['gset'][~np.isnan(g['gset'])]) == {1.1, 2.5}
    worst = [0.0, 0.0, 0.0]
    none = 0
    for l in range(n):
        ls_lo = g['ls'][l] or (not np.isnan(g['lower'][l][0]) and g['lower'][l][0] <= g['lower'][l][1] + g['lower'][l][2])
        ls_up = g['ls'][l] or (not np.isnan(g['upper'][l][0]) and g['upper'][l][0] <= g['upper'][l][1] + g['upper'][l][2])
        line = sc._Line(_Level(g['lower'][l], ls_lo), _Level(g['upper'][l], ls_up), None if np.isnan(g['gset'][l]) else float(g['gset'][l]))
        z = zeeman.zeeman_components(line)
        a, b = int(g['ptr'][l]), int(g['ptr'][l + 1])
        if not g['has'][l]:
            assert z is None, l
            none += 1
        else:
            assert z is not None and np.array_equal(z.alpha, g['alpha'][a:b]), l
            worst[0] = max(worst[0], ulps(z.strength, g['strength'][a:b]))
            worst[1] = max(worst[1], ulps(z.shift, g['shift'][a:b]))
            for q in (-1, 0, 1):
                assert abs(z.strength[z.alpha == q].sum() - 1.0) <= 1e-12
        ge = zeeman.effective_lande(line)
        if np.isnan(g['geff'][l]):
            assert ge is None, l
        else:
            worst[2] = max(worst[2], ulps(ge, g['geff'][l]))
    print('patterns: %d lines, %d without a pattern; worst strength %.1f ulp, shift %.1f ulp, effective Lande factor %.1f ulp' % (n, none, *worst))
    assert none >= 1 and max(worst) <= 4.0


def test_the_patterns_of_the_cases():
    assert np.array_equal(sc.TRIPLET.alpha, [-1, 0, 1]) and np.array_equal(sc.TRIPLET.shift, np.array([-1, 0, 1]) * 1.1)
    assert len(sc.LARGEST) == 27 and len(sc.SMALL) == 6
    nc, al, st, sh = zeeman.pack([None, sc.SMALL, sc.TRIPLET], 3)
    assert list(nc) == [0, 6, 3] and al.shape == (10,) and np.array_equal(al[:6], sc.SMALL.alpha)
    with pytest.raises(ValueError):
        zeeman.pack([None], 2)


# ---- 2. the Faraday-Voigt function ------------------------------------------------------------------------------------------------------
def _samples():
    x = np.unique(np.abs(np.concatenate([vc.X_A, vc.X_B, [0.0, 1e-9, 0.124, 0.126, 0.374, 0.376, 0.5, 1.0, 2.0, 3.3, 5.0, 6.6, 12.0, 20.0, 26.9, 27.1, 60.0]])))
    a, v = [], []
    for ia, av in enumerate(vc.A_VALUES):
        for ix, xv in enumerate(x):
            if (ia + ix) % 2 and xv not in (0.0,):          # thinned: every other (a, x) pair, both signs of each kept one
                continue
            a += [av, av]
            v += [xv, -xv]
    return np.array(a), np.array(v)


def _w_ref(a, v):
    x = abs(v)
    if a == 0.0:
        if x >= 12.0:
            return vc._w(0.0, v, 'series', 1)
        vc.MP.dps = 80 + int(x * x)
        z = vc.MP.mpc(vc.MP.mpf(v), 0)
        return vc.MP.exp(-z * z) * vc.MP.erfc(vc.MP.mpc(0, -1) * z)
    return vc._w(float(a), v, None, 1)


def test_faraday_voigt_against_mpmath(host):
    """all 40 rows of a of voigt_cases, the x aimed at every switch of the rule, both signs of v.  Bar per entry:
    |F - Im w| <= 1e-13 |w| (a and v are handed over exactly: no conditioning term); H of the same call has dev_voigt's bits.
    Measured: worst |F - Im w| / (1e-13 |w|) = 0.007; F(-v) = -F(v) exactly for v != 0"""
    a, v = _samples()
    assert 1500 <= a.shape[0] <= 6000 and len(set(a)) == 40
    H, F, Hv = host.w(a, v)
    assert np.array_equal(H.view(np.uint64), Hv.view(np.uint64))
    worst, where = 0.0, None
    for i in range(0, a.shape[0], 2):          # (v >= 0; the mirrored entry follows)
        w = _w_ref(a[i], float(v[i]))
        vc.MP.dps = 50
        r = float(abs(vc.MP.mpf(float(F[i])) - w.imag) / (sc.BASE * 1e-2 * abs(w)))
        if r > worst:
            worst, where = r, (a[i], v[i])
        assert (F[i + 1] == -F[i] or v[i] == 0.0) and H[i + 1] == H[i]          # (-0.0 is not negative: F(0) is a rounding residue of 4e-17)
    print('Faraday-Voigt: %d samples, worst |F - Im w| / (1e-13 |w|) = %.3f at (a, v) = %s' % (a.shape[0], worst, where))
    assert worst <= 1.0


# ---- 3. geometry -------------------------------------------------------------------------------------------------------------------
def test_geometry(host):
    rng = np.random.default_rng(3)
    g, x, mu = rng.uniform(0, np.pi, 400), rng.uniform(-7, 7, 400), np.concatenate([rng.uniform(0.05, 1, 300), np.ones(100)])
    G = host.geometry(g, x, mu)
    b = np.stack([np.sin(g) * np.cos(x), np.sin(g) * np.sin(x), np.cos(g)], axis=1)
    st = np.sqrt((1 - mu) * (1 + mu))
    l = np.stack([st, 0 * mu, mu], axis=1)
    e1 = np.stack([mu, 0 * mu, -st], axis=1)
    c, b1, b2 = (b * l).sum(1), (b * e1).sum(1), b[:, 1]
    ref = np.stack([c, b1 * b1 + b2 * b2, b1 * b1 - b2 * b2, 2 * b1 * b2], axis=1)
    assert np.max(np.abs(G - ref)) <= 4 * sc.U * 2
    assert np.max(np.abs(G[:, 0] ** 2 + G[:, 1] - 1.0)) <= 4 * 2 * sc.U          # 4 ulp of 1
    at1 = mu == 1.0
    assert np.max(np.abs(G[at1, 2] - np.sin(g[at1]) ** 2 * np.cos(2 * x[at1]))) <= 8 * sc.U
    assert np.max(np.abs(G[at1, 3] - np.sin(g[at1]) ** 2 * np.sin(2 * x[at1]))) <= 8 * sc.U
    # a field along the ray: gamma = acos(mu), chi = 0
    m2 = rng.uniform(0.05, 1, 50)
    A = host.geometry(np.arccos(m2), 0.0, m2)
    assert np.max(np.abs(A[:, 1:])) <= 1e-15 and np.max(np.abs(A[:, 0] - 1.0)) <= 4 * sc.U
    A = host.geometry(0.0, 1.234, 1.0)
    assert A[0, 0] == 1.0 and np.all(A[0, 1:] == 0.0)


# ---- 4. the solver's properties on made-up columns -----------------------------------------------------------------------------------------
MUS = (1.0, 0.6, 0.1)


def _col(Ns, kind='inclined', pats='blend', vlos=True):
    prob, block, prof, J = sc.problem(Ns, 1, vlos=vlos)
    return sc.column(prob, block, prof, block.n, J, sc.field(Ns, 1, kind), sc.PATTERN_SETS[pats], 0, la0=30, nla=87)


def _runs(host, col, mu):
    return {u: host.window(col, mu, u) for u in (0, 1, -1)}


def _bar(r):
    return sc.BASE * np.abs(r[0][0:1]) + sc.K_ENVELOPE * np.abs(r[1] - r[-1])


def _scalar_I(host, col, mu, ulp=0, shift_vZ=None, endpoint=True):
    """the linear rule on chi_c + sum nd phi; shift_vZ = (line, sign): that line's profile at v - sign vZ (a longitudinal triplet's
    I + V and I - V)"""
    nla, Ns = col.wav.shape[0], col.z.shape[0]
    out = np.empty(nla)
    for q in range(nla):
        chi, eta = col.chi_c[q].copy(), col.eta_c[q].copy()
        for l in range(col.lambda0.shape[0]):
            v = (col.wav[q] - col.lambda0[l]) * sc.CLIGHT / (col.vB[l] * col.lambda0[l]) + 1.0 * (mu * col.vlos / col.vB[l])
            if shift_vZ is not None and shift_vZ[0] == l:
                v = v - shift_vZ[1] * (sc.LARMOR * (1e-9 * col.lambda0[l]) * col.B / col.vB[l])
            ph = host.w(col.aD[l], v)[0] / (np.sqrt(np.pi) * col.vB[l])
            chi += col.nd[l] * ph
            eta += col.ne[l] * ph
        I0 = 0.0 if col.lower_zero else sc.thermal_start(col, q, mu, chi)
        out[q] = sc.linear_rule(col.z, chi, eta / chi, mu, I0, ulp, endpoint)
    return out


@pytest.mark.parametrize('Ns', [13, 40])
def test_without_patterns_the_rule_is_the_linear_rule(host, Ns):
    """(a): Q = U = V = 0.0 exactly; I against the numpy restatement of the reference's linear rule, its end point included (and with
    the end-point term taken out of both: the plain rule)"""
    col = _col(Ns, pats='none')
    for mu in MUS:
        r = _runs(host, col, mu)
        assert np.all(r[0][1:] == 0.0)
        ref = _scalar_I(host, col, mu)
        ex = float(np.max(np.abs(r[0][0] - ref) / _bar(r)[0]))
        print('Ns %d mu %.1f: I against the linear rule %.3f of the bar (%.2e relative)' % (Ns, mu, ex, np.max(np.abs(r[0][0] - ref) / ref)))
        assert ex <= 1.0
        plain = host.window(col, mu, endpoint=False)
        assert np.all(np.abs(plain[0] - _scalar_I(host, col, mu, endpoint=False)) <= _bar(r)[0]) and np.all(plain[1:] == 0.0)
        assert np.max(np.abs(plain[0] - r[0][0]) / r[0][0]) > 1e-12          # the end-point term is there


@pytest.mark.parametrize('Ns', [13, 40])
def test_no_field_no_polarisation(host, Ns):
    """(b): B = 0 everywhere with patterns present"""
    col0, col = _col(Ns, pats='none'), _col(Ns, kind='zero', pats='all')
    for mu in MUS:
        r0, r = _runs(host, col0, mu), host.window(col, mu)
        bar = _bar(r0)
        ex = float(max(np.max(np.abs(r[0] - r0[0][0]) / bar[0]), np.max(np.abs(r[1:]) / bar[1:])))
        print('(b) Ns %d mu %.1f: worst deviation / bar %.4f' % (Ns, mu, ex))
        assert np.all(np.abs(r[0] - r0[0][0]) <= bar[0]) and np.all(np.abs(r[1:]) <= bar[1:])


def _K_of(host, col, q, mu):
    Ns = col.z.shape[0]
    K = np.empty((Ns, 11))
    for k in range(Ns):
        v = (col.wav[q] - col.lambda0) * sc.CLIGHT / (col.vB[:, k] * col.lambda0) + 1.0 * (mu * col.vlos[k] / col.vB[:, k])
        vZ = sc.LARMOR * (1e-9 * col.lambda0) * col.B[k] / col.vB[:, k]
        K[k] = host.K(col.chi_c[q, k], col.eta_c[q, k], col.nd[:, k], col.ne[:, k], col.aD[:, k], v, vZ, 1.0 / (np.sqrt(np.pi) * col.vB[:, k]),
                      col.patterns, col.gammaB[k], col.chiB[k], mu)
    return K


@pytest.mark.parametrize('Ns', [13, 40])
def test_field_reversal_flips_V(host, Ns):
    """(c): b -> -b is gamma -> pi - gamma, chi -> chi + pi.  As the issue states it (I, Q, U kept, V flipped) the property holds
    where the magneto-optical terms do not couple: Faraday rotation (rho_V) turns Q into U in the opposite sense when the field is
    reversed, and the Unno-Rachkovsky solution's term eta_V rho_U - eta_U rho_V of Q changes sign.  Measured on the inclined field of
    these columns: Q and U move by up to 0.15 I, I by 3e-3 I, V by 1.6e-2 I.  So it is held (i) on a field along the vertical seen at
    mu = 1 (gamma' = 0 <-> pi: no linear polarisation, rho_Q = rho_U = 0) for the whole solve, (ii) on the inclined field at every
    angle for the propagation matrix (eta_V, rho_V, eps_V flip, the other eight entries keep their bits up to rounding), and (iii)
    for the solve of that matrix with the magneto-optical terms taken out"""
    col = _col(Ns, kind='along')
    rev = col.replace(gammaB=np.pi - col.gammaB, chiB=col.chiB + np.pi)
    r0, r = _runs(host, col, 1.0), host.window(rev, 1.0)
    bar = _bar(r0)
    assert np.max(np.abs(r0[0][3])) > 1e3 * np.max(bar)          # there is a V to flip
    print('(c) Ns %d longitudinal, the whole solve: worst deviation / bar %.4f'
          % (Ns, max(np.max(np.abs(r[:3] - r0[0][:3]) / bar[:3]), np.max(np.abs(r[3] + r0[0][3]) / bar[3]))))
    assert np.all(np.abs(r[:3] - r0[0][:3]) <= bar[:3]) and np.all(np.abs(r[3] + r0[0][3]) <= bar[3]) and np.all(np.abs(r[1:3]) <= bar[1:3])
    col = _col(Ns)
    rev = col.replace(gammaB=np.pi - col.gammaB, chiB=col.chiB + np.pi)
    flip = np.array([1, 1, 1, -1, 1, 1, -1, 1, 1, 1, -1.0])
    worst_K = worst_x = 0.0
    for mu in MUS:
        for q in (20, 43, 60):
            K, Kr = _K_of(host, col, q, mu), _K_of(host, rev, q, mu)
            worst_K = max(worst_K, float(np.max(np.abs(Kr - K * flip) / (1e-13 * np.abs(K[:, [0] * 7 + [7] * 4])))))
            assert np.all(np.abs(Kr - K * flip) <= 1e-13 * np.abs(K[:, [0] * 7 + [7] * 4]))
            assert np.max(np.abs(K[:, 3] / K[:, 0])) > 1e-5 and np.max(np.abs(K[:, 6] / K[:, 0])) > 1e-5
            th = (sc.planck(col.T[-1], col.wav[q]), sc.planck(col.T[-2], col.wav[q]))
            K0, K0r = K.copy(), Kr.copy()
            K0[:, 4:7] = 0.0
            K0r[:, 4:7] = 0.0
            x = {u: host.ray(col.z, K0, mu, th, u) for u in (0, 1, -1)}
            xr = host.ray(col.z, K0r, mu, th)
            bb = sc.BASE * abs(x[0][0]) + sc.K_ENVELOPE * np.abs(x[1] - x[-1])
            worst_x = max(worst_x, float(np.max(np.abs(xr - x[0] * np.array([1, 1, 1, -1.0])) / bb)))
            assert np.all(np.abs(xr - x[0] * np.array([1, 1, 1, -1.0])) <= bb) and abs(x[0][3]) > 10 * bb[3]
    print('(c) Ns %d inclined: the matrix, worst deviation / (1e-13 of eta_I, eps_I) %.4f; the solve without rho, worst deviation / bar %.4f'
          % (Ns, worst_K, worst_x))


@pytest.mark.parametrize('delta', [0.3, 0.5 * np.pi])
def test_azimuth_rotates_Q_and_U(host, delta):
    """(d): at mu = 1, chi -> chi + delta rotates (Q, U) by 2 delta and leaves I and V"""
    for Ns in (13, 40):
        col = _col(Ns)
        r0, r = _runs(host, col, 1.0), host.window(col.replace(chiB=col.chiB + delta), 1.0)
        bar = _bar(r0)
        c2, s2 = np.cos(2 * delta), np.sin(2 * delta)
        Q, Uu = r0[0][1], r0[0][2]
        assert np.max(np.hypot(Q, Uu)) > 1e3 * np.max(bar)
        dev = np.abs(np.stack([r[0] - r0[0][0], r[1] - (c2 * Q - s2 * Uu), r[2] - (s2 * Q + c2 * Uu), r[3] - r0[0][3]]))
        # the bar of each parameter itself; the rotated Q and U mix the two envelopes: the smaller of the two is asked of both
        bq = np.minimum(bar[1], bar[2])
        bars = np.stack([bar[0], bq, bq, bar[3]])
        print('(d) delta %.2f Ns %d: worst deviation / bar %.4f' % (delta, Ns, float(np.max(dev / bars))))
        assert np.all(dev <= bars)


def test_sign_of_V(host):
    """(e): an absorption line in a field pointing at the observer: V > 0 on the blue flank, V < 0 on the red flank"""
    col = _col(40, kind='along', pats='triplet', vlos=False)
    col = col.replace(nd=col.nd * np.array([0.0, 1.0, 0.0])[:, None], ne=col.ne * np.array([0.0, 0.02, 0.0])[:, None])          # (a small line source function: absorption)
    r = host.window(col, 1.0)
    I, V = r[0], r[3]
    core = int(np.argmin(np.abs(col.wav - col.lambda0[1])))
    assert I[core] < 0.8 * I[0] and I[core] < 0.8 * I[-1]                 # an absorption line
    blue, red = slice(core - 6, core - 1), slice(core + 2, core + 7)
    print('(e) line depth %.2f of the continuum; V / I_c between %.3f (blue flank) and %.3f (red flank)' % (1.0 - I[core] / I[0], np.max(V) / I[0], np.min(V) / I[0]))
    assert np.all(V[blue] > 0) and np.all(V[red] < 0) and np.max(np.abs(V)) > 1e-3 * I[0]
    assert np.all(np.abs(r[1:3]) <= 1e-13 * I)                            # longitudinal: no linear polarisation


def test_the_end_point_term_is_one_scalar_term_of_I(host):
    """the shipped end point (lsx_stokes_dev.h, delo_step with last): against the plain DELO step at the last depth Q, U, V keep their
    bits, and I moves by the reference's end-point form minus the plain linear step on eps_I / eta_I, restated here from the matrices
    and the state at depth 1 (the same walk one depth shorter).  Property (f) below pins the rule with the term off; this pins the term"""
    col = _col(13)
    for mu in MUS:
        for q in (20, 43, 60):
            K = _K_of(host, col, q, mu)
            th = (sc.planck(col.T[-1], col.wav[q]), sc.planck(col.T[-2], col.wav[q]))
            a, b = host.ray(col.z, K, mu, th, endpoint=True), host.ray(col.z, K, mu, th, endpoint=False)
            u = host.ray(col.z[1:], K[1:], mu, th, endpoint=False)
            assert np.array_equal(a[1:].view(np.uint64), b[1:].view(np.uint64))
            dtau = 0.5 * (K[1, 0] + K[0, 0]) * abs(col.z[1] - col.z[0]) / mu
            prev = 0.5 * (K[2, 0] + K[1, 0]) * abs(col.z[2] - col.z[1]) / mu
            (w0, w1), (w0p, w1p) = sc._w2(dtau, 0), sc._w2(prev, 0)
            Su, Sk = K[1, 7] / K[1, 0], K[0, 7] / K[0, 0]
            delta = u[0] * (w0 - w0p) + (w0p * Su - w0 * Sk) + (w1p - w1) * (Su - Sk) / dtau
            assert delta != 0.0 and abs((a[0] - b[0]) - delta) <= 1e-13 * abs(b[0]) + 1e-12 * abs(delta)


def test_the_restated_start_values_are_the_final_passes():
    """lsx_stokes_dev.h restates planck, thermal_start and the constants of lsx_final_dev.h (a host compiler cannot read that header):
    the constants have the same literals and the two functions the same statements"""
    mine = open(os.path.join(CSRC, 'lsx_stokes_dev.h')).read()
    theirs = open(os.path.join(CSRC, 'lsx_final_dev.h')).read()
    for name in ('kCLight', 'kHPlanck', 'kKBoltzmann', 'kNM_TO_M'):
        lit = lambda text: re.search(r'constexpr double %s = ([0-9.Ee+-]+);' % name, text).group(1)
        assert lit(mine) == lit(theirs), name
    norm = lambda t: re.sub(r'\s+', '', t)
    body = lambda text, head: norm(text[text.index(head):].split('\n}\n')[0].split('{', 1)[1])
    assert body(mine, 'double planck(double temp, double wav)') == body(theirs, 'double planck(double temp, double wav)')
    assert 'kHC=kHPlanck*kCLight;' in norm(mine) and 'kHC=kHPlanck*kCLight;' in norm(theirs)
    # thermal_start: theirs per angle, dtau_uw = zmu (c_k + chi) 0.5 adz; mine with adz_zmu = adz zmu: the same product up to its order
    assert 'Be-(Bn-Be)/dtau_uw' in norm(mine) and 'Be-(Bn-Be)/dtau_uw' in norm(theirs)
    assert 'dtau_uw=(c_k+chi)*0.5*adz_zmu' in norm(mine) and 'dtau_uw=zmu[m]*(c_k[m]+chi[m])*0.5*adz' in norm(theirs)


def _refine(col, f):
    """the column on f times as many intervals: every quantity linear in the depth index between the old depths"""
    Ns = col.z.shape[0]
    x0, x1 = np.arange(Ns), np.arange((Ns - 1) * f + 1) / f
    it = lambda a: np.interp(x1, x0, a)
    it2 = lambda A: np.stack([it(a) for a in A])
    return col.replace(z=it(col.z), T=it(col.T), chi_c=it2(col.chi_c), eta_c=it2(col.eta_c), nd=it2(col.nd), ne=it2(col.ne), aD=it2(col.aD),
                       vB=it2(col.vB), vlos=it(col.vlos), B=it(col.B), gammaB=it(col.gammaB), chiB=it(col.chiB))


def test_longitudinal_triplet_is_two_scalar_problems(host):
    """(f): gamma' = 0: I + V and I - V obey the scalar equation with the profile at v -+ vB.  The DELO-linear rule on the system and
    the linear rule on the two scalar problems are both second order: their difference falls by at least 3 x per halving of the depth
    step.  Measured (largest |difference| / I over the window, 13 depths, then 2 x and 4 x refined): printed below"""
    base = _col(13, kind='along', pats='triplet', vlos=False)
    g = sc.TRIPLET.shift[2]
    diffs = []
    for f in (1, 2, 4):
        col = _refine(base, f)
        r = host.window(col, 1.0, endpoint=False)          # (the rule itself: the end-point term of I is the reference's, not the rule's)
        plus = _scalar_I(host, col, 1.0, shift_vZ=(1, g), endpoint=False)
        minus = _scalar_I(host, col, 1.0, shift_vZ=(1, -g), endpoint=False)
        diffs.append(max(float(np.max(np.abs(r[0] + r[3] - plus) / r[0])), float(np.max(np.abs(r[0] - r[3] - minus) / r[0]))))
    print('longitudinal triplet, DELO-linear against the scalar linear rule: %.3e, %.3e, %.3e' % tuple(diffs))
    assert diffs[0] > 1e-9                                                # (they are different rules)
    assert diffs[1] <= diffs[0] / 3.0 and diffs[2] <= diffs[1] / 3.0


def test_K_and_ray_are_the_window(host):
    """the two small exports chained by hand give the window call's bits"""
    col = _col(13)
    mu, q = 0.6, 40
    K = np.empty((13, 11))
    for k in range(13):
        v = (col.wav[q] - col.lambda0) * sc.CLIGHT / (col.vB[:, k] * col.lambda0) + 1.0 * (mu * col.vlos[k] / col.vB[:, k])
        vZ = sc.LARMOR * (1e-9 * col.lambda0) * col.B[k] / col.vB[:, k]
        K[k] = host.K(col.chi_c[q, k], col.eta_c[q, k], col.nd[:, k], col.ne[:, k], col.aD[:, k], v, vZ, 1.0 / (np.sqrt(np.pi) * col.vB[:, k]),
                      col.patterns, col.gammaB[k], col.chiB[k], mu)
    assert np.all(np.abs(K[:, 1:4]).sum(1) > 0) and np.all(K[:, 0] ** 2 >= (K[:, 1:4] ** 2).sum(1))
    one = host.ray(col.z, K, mu, thermal=(sc.planck(col.T[-1], col.wav[q]), sc.planck(col.T[-2], col.wav[q])))
    win = host.window(col, mu)[:, q]
    assert np.allclose(one, win, rtol=1e-13, atol=1e-13 * win[0])


def test_the_rules(host):
    B, g, x = sc.field(5, 1)
    ok = [None, sc.SMALL, sc.LARGEST]
    assert host.check(B, g, x, ok) == sc.LSX_OK
    big = zeeman.ZeemanComponents(np.r_[sc.LARGEST.alpha, np.zeros(38, dtype=np.int32)], np.r_[sc.LARGEST.strength, np.zeros(38)], np.r_[sc.LARGEST.shift, np.zeros(38)])
    assert len(big) == sc.MAX_COMPONENTS + 1 and host.check(B, g, x, [big]) == sc.LSX_EUNSUPPORTED
    at = zeeman.ZeemanComponents(big.alpha[:-1], big.strength[:-1], big.shift[:-1])
    assert host.check(B, g, x, [at]) == sc.LSX_OK
    assert host.check(B, g, x, [([-1, 0, 2], [1, 1, 1], [0, 0, 0])]) == sc.LSX_EINVAL
    assert host.check(B, g, x, [([-1, 0, 1], [1, 1, 1 + 1e-11], [0, 0, 0])]) == sc.LSX_EINVAL
    assert host.check(B, g, x, [([-1, 0, 1], [1, 1, 1 + 5e-13], [0, 0, 0])]) == sc.LSX_OK
    assert host.check(B, g, x, [([-1, 0], [1, 1], [0, 0])]) == sc.LSX_EINVAL            # no sigma_r at all
    for bad in (np.nan, np.inf, -1e-30):
        Bb = B.copy()
        Bb[0, 2] = bad
        assert host.check(Bb, g, x, ok) == sc.LSX_EINVAL
    gb = g.copy()
    gb[0, 1] = np.nan
    assert host.check(B, gb, x, ok) == sc.LSX_EINVAL and host.check(B, g, gb, ok) == sc.LSX_EINVAL
    assert host.check(B, g, x, [sc.LARGEST] * 38) == sc.LSX_EUNSUPPORTED                    # 1026 components in one window


# ---- 5. the entry's hygiene ----------------------------------------------------------------------------------------------------------
def test_the_entries_are_exported_declared_in_a_header_of_their_own_and_bound():
    lib = os.path.join(CSRC, 'liblsx_hip.so')
    assert os.path.exists(lib), 'build the HIP library first (make -C lightspinner_amd/csrc)'
    syms = subprocess.run(['nm', '-D', '--defined-only', lib], capture_output=True, text=True, check=True).stdout
    text = open(os.path.join(ROOT, 'include', 'lsx_hip_stokes.h')).read()
    assert set(re.findall(r'\b(lsx_hip_[a-z0-9_]+)\s*\(', text)) == ENTRIES
    assert set(re.findall(r'\bT (lsx_hip_stokes[a-z0-9_]*)\b', syms)) == ENTRIES
    assert '#include "lsx_hip_stokes.h"' in open(os.path.join(ROOT, 'include', 'lsx_hip.h')).read()
    assert not any(s.startswith('lsx_hip_stokes') for s in _capi.REQUIRED_SYMBOLS)        # the common ABI is what it was
    for other in os.listdir(os.path.join(ROOT, 'include')):
        if other != 'lsx_hip_stokes.h':
            assert 'lsx_hip_stokes_rays' not in open(os.path.join(ROOT, 'include', other)).read(), other
    assert int(re.search(r'#define LSX_STOKES_MAX_COMPONENTS (\d+)', text).group(1)) == sc.MAX_COMPONENTS == zeeman.MAX_COMPONENTS
    hip = _capi.load_hip_library()
    assert hip.has_stokes and hip.dll.lsx_hip_stokes_rays.restype is not None


@pytest.mark.parametrize('compiler,std', [('gcc', 'c99'), ('g++', 'c++11')])
def test_the_header_compiles_alone(compiler, std):
    lang = 'c' if compiler == 'gcc' else 'c++'
    r = subprocess.run([compiler, '-std=' + std, '-Wall', '-Wextra', '-pedantic', '-Werror', '-fsyntax-only', '-x', lang,
                        os.path.join(ROOT, 'include', 'lsx_hip_stokes.h')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_oracle_has_no_such_entry_and_the_engine_says_so(oracle_lib):
    from lightspinner_amd import fixtures
    from lightspinner_amd.problem import Engine
    prob, block, raw = fixtures.load_problem_npz(golden('falc_ca.npz'))
    e = Engine(prob, 1, lib=oracle_lib)
    e.set_columns(0, block)
    assert not oracle_lib.has_stokes
    with pytest.raises(NotImplementedError, match='lsx_hip_stokes_rays'):
        e.stokes_rays([1.0], 0.1, 0.0, 0.0)
    e.close()


def test_the_kernel_uses_no_scratch_and_spills_no_vector_register():
    """build/lsx_stokes.ru.log, the compiler's resource report of the unit: every instance without scratch, without a spilled vector
    register and without a dynamic stack"""
    path = os.path.join(CSRC, 'build', 'lsx_stokes.ru.log')
    if not os.path.exists(path):
        subprocess.check_call(['make', '-s', '-j', '8', '-C', CSRC])
    blocks = re.split(r'remark: [^\n]*Function Name: ', open(path).read())[1:]
    names = [b.split()[0] for b in blocks]
    assert names and all('k_stokes_raysILi' in x for x in names), names
    for b, name in zip(blocks, names):
        val = lambda key: int(re.search(re.escape(key) + r':? (\d+)', b).group(1))
        assert val('ScratchSize [bytes/lane]') == 0, name
        assert val('VGPRs Spill') == 0, name
        assert re.search(r'Dynamic Stack: False', b), name


def test_formulas_under_asan_ubsan():
    """the function over the plane, the geometry, the rules at and over the caps, windows with the largest pattern: in a stand-alone
    program"""
    subprocess.check_call(['make', '-s', '-C', CSRC, 'stokessan'])
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:halt_on_error=1', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')
    out = subprocess.run([os.path.join(CSRC, 'lsx_stokes_san')], capture_output=True, text=True, timeout=600, env=env)
    tail = out.stdout[-1500:] + '\n' + out.stderr[-3000:]
    assert out.returncode == 0, tail
    assert 'STOKES SANITIZED RUN COMPLETE' in out.stdout, tail
