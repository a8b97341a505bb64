"""The Voigt function pinned over the whole (a, v) plane (tests/test_voigt_plane_host.py, tests/test_voigt_plane.py).

The reference is mpmath, not scipy (wofz is itself only good to 1-3e-14): H = Re w(z), dH/dv = Re(-2 z w(z)), z = v + i a, by
  a == 0                 exp(-v^2), exactly;
  the series             w = i / (sqrt(pi) z) sum_m (2m - 1)!! / (2 z^2)^m, summed to its smallest term at 50 digits, where |z| >= 12
                         (smallest term < exp(-144)) and the Gaussian part it cannot see, exp(a^2 - x^2), is below 1e-30 of the wing;
  exp(-z^2) erfc(-i z)   everywhere else, at 50 + x^2 / 2 digits: the real part 1 of erfc sits beside an imaginary part of size
                         exp(x^2), so a fixed precision is WRONG for small a and x >~ 12.
`H_ref(a, v, route=..., scale=2)` evaluates by a named route / at twice the digits: the self-check of the host test.

The bar, entry by entry:  |H - H_ref| <= 1e-13 H_ref + |dH/dv| 4 u (|v0| + |shift|)
1e-13 is the suite's figure for phi and wphi (tests/test_line_profiles.py); the second term is the conditioning of H on its argument,
v0 = (lambda - lambda0) c / (v_b lambda0) and shift = mu v_los / v_b being formed with a few roundings each.  A reference below 1e-290
(the row a = 0 at x >= 26 only) is compared absolutely at 1e-290.  wphi: 1e-13 + (N_terms + 2) u relative (sequential summation of
positive terms).

`probe(ncol, Ns, compact)` is a made-up problem from tests/toy.py whose wavelengths, damping, widths and velocities are chosen so
that the samples fill the plane; `coverage` counts them the way the kernels form x and `assert_coverage` holds the conditions."""
import dataclasses
import functools

import mpmath
import numpy as np

import toy

U = 2.0 ** -53
BAR = 1e-13
TINY = 1e-290
MP = mpmath.mp.clone()
CLIGHT = 2.99792458E+08          # the libraries' constant (rh_method.py's CLight)
TWO_PI = 2.0 * np.pi             # the double the libraries compare a with
X_RANGES = (0.0, 1.0, 3.0, 7.0, 27.0, 1e3, np.inf)      # the last bin (x >= 1e3) is counted, not required
A_SPECIAL = (np.nextafter(TWO_PI, 0.0), TWO_PI, TWO_PI * (1 - 1e-3), TWO_PI * (1 + 1e-3), 3 * np.pi, 4 * np.pi)
# one value per row of the coverage table first (a = 0, the decades 1e-12 .. 1e3), the values round 2 pi, then the half decades and 1e4
A_VALUES = np.array([0.0] + [10.0 ** e for e in range(-12, 4)] + list(A_SPECIAL) + [10.0 ** (e + 0.5) for e in range(-12, 4)] + [1e4])
assert A_VALUES.shape[0] == 40 and A_SPECIAL[0] < TWO_PI


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def _series_applies(a, x):
    if a <= 0.0 or a * a + x * x < 144.0:
        return False
    if a >= 1.0:      # |remainder| <= Gamma(M + 1/2) / (pi a |z|^2M): the first omitted term times |z| / (a sqrt(pi))
        return True
    # log of [exp(a^2 - x^2)] / [a / (sqrt(pi) |z|^2)] below log(1e-30)
    return (a * a - x * x) - np.log(a / (np.sqrt(np.pi) * (a * a + x * x))) < -69.0


def _w(a, v, route, scale):
    """w(v + i a) as an mpmath complex; a: float, v: float or mpf (exact)"""
    x = abs(float(v))
    if route is None:
        route = 'series' if _series_applies(a, x) else 'erfc'
    if route == 'series':
        MP.dps = 50 * scale
        z = MP.mpc(MP.mpf(v), MP.mpf(a))
        q = 1 / (2 * z * z)
        s, term, m = MP.mpc(0), MP.mpc(1), 0
        while True:
            s += term
            m += 1
            new = term * (2 * m - 1) * q
            if abs(new) >= abs(term) or abs(new) < MP.mpf(10) ** (-MP.dps) * abs(s):
                break
            term = new
        return MP.mpc(0, 1) / (MP.sqrt(MP.pi) * z) * s
    assert route == 'erfc'
    MP.dps = int(50 + x * x / 2) * scale
    z = MP.mpc(MP.mpf(v), MP.mpf(a))
    return MP.exp(-z * z) * MP.erfc(MP.mpc(0, -1) * z)


_cache = {}


def H_both(a, v, route=None, scale=1):
    """-> (H, dH/dv) as mpmath numbers; cached by (a, v)"""
    key = (float(a), v, route, scale)
    if key not in _cache:
        if a == 0.0 and route is None:
            MP.dps = 50 * scale
            g = MP.exp(-MP.mpf(v) ** 2)
            _cache[key] = (g, -2 * MP.mpf(v) * g)
        else:
            w = _w(float(a), v, route, scale)
            z = MP.mpc(MP.mpf(v), MP.mpf(float(a)))
            _cache[key] = (w.real, (-2 * z * w).real)
    return _cache[key]


def H_ref(a, v, **kw):
    return H_both(a, v, **kw)[0]


def dHdv_ref(a, v, **kw):
    return H_both(a, v, **kw)[1]


def split(x):
    """an mpmath number as (hi, lo) doubles: hi + lo carries it to 1e-32 relative"""
    hi = float(x)
    return hi, (float(x - MP.mpf(hi)) if np.isfinite(hi) else 0.0)


def excess_H(got, a, v, cond=0.0):
    """(|got - H_ref| / bar, relative deviation) of one value of the bare function; cond: 4 u (|v0| + |shift|), 0 where a and v are
    handed over exactly"""
    H, dH = H_both(a, v)
    MP.dps = 50
    dev = abs(MP.mpf(got) - H)
    bar = BAR * H + abs(dH) * cond
    if H < TINY:
        bar = MP.mpf(TINY)
    return float(dev / bar), (float(dev / H) if H >= TINY else 0.0)


# ---- the made-up problem ------------------------------------------------------------------------------------------------------------
NSPECT = 63                                      # three natural tiles of L = 64 / 3 = 21 wavelengths
LINE_A, LINE_B, CONT = (18, 15), (42, 15), (0, 12)      # (Nblue, Nlambda): A straddles wavelength 21 (pieces of 3 and 12)
VREF = 3.0e4
D = 2e-4                                         # distance of the aimed samples from a switch, in x
X_A = np.array([-800.0, -27 - D, -27 + D, -9.125 - D, -9.125 + D, -2.375 - D, -2.375 + D, 0.0,
                0.125 - D, 0.125 + D, 0.375 - D, 0.375 + D, 4.625 - D, 4.625 + D, 60.0])
X_B = np.array([-300.0, -40.0, -27 - 1.5 * D, -27 + 1.5 * D, -13.875 - D, -13.875 + D, -5.125 - D, -5.125 + D, -1.5, 0.6,
                0.875 - D, 0.875 + D, 3.125 - D, 3.125 + D, 500.0])
F_VB = np.array([1, 1, 1, 1, 1, 1, 1, 1, 0.3, 2.7, 11.0, 37.0, 1])            # v_b / VREF by depth (repeated beyond 13 depths)
SIGMA = np.array([0, 0, 0, 0, 0, 0.37, -2.9, 14.0, 0.9, -0.11, 5.0, 0, 61.0])    # v_los / v_b by depth (4-D probes)


@functools.lru_cache(maxsize=None)
def probe(ncol, Ns, compact):
    """-> (prob, block with phi = wphi = None, (aDamp, vBroad, vlos or None))"""
    frac = lambda nb, nl: ((nb + 0.5) / NSPECT, (nb + nl + 0.5) / NSPECT)
    specs = [('c', 0, 2) + frac(*CONT), ('l', 0, 1) + frac(*LINE_A), ('l', 1, 2) + frac(*LINE_B)]
    prob, block = toy.spec_problem([(3, specs)], seed=11, Nspace=Ns, Nrays=3, Nspect=NSPECT, ncol=ncol, phi_compact=compact)
    assert [(t.Nblue, t.Nlambda) for t in prob.trans] == [CONT, LINE_A, LINE_B]
    wl = 100.0 + 10.0 * np.arange(NSPECT)
    trans = list(prob.trans)
    for kr, X in ((1, X_A), (2, X_B)):
        t = trans[kr]
        lam0 = wl[t.Nblue + t.Nlambda // 2]
        wl[t.Nblue:t.Nblue + t.Nlambda] = lam0 * (1.0 + X * (VREF / CLIGHT))
        trans[kr] = dataclasses.replace(t, lambda0=lam0, Aji=2.0 * toy.HC / (lam0 * 1e-9) ** 3 * t.Bji)
    assert np.all(np.diff(wl) > 0)
    prob = dataclasses.replace(prob, wavelength=wl, trans=trans)
    k = np.arange(Ns) % 13
    vB = np.tile(VREF * F_VB[k], (ncol, 1, 1))
    vlos = None if compact else np.tile(SIGMA[k] * VREF * F_VB[k], (ncol, 1)) * (1.0 + 0.25 * np.arange(ncol))[:, None]
    # damping: the depths whose samples sit on the aimed x first, so that every row of the table meets every range of x
    exact = (F_VB[k] == 1) & (compact | (SIGMA[k] == 0))
    order = np.concatenate([np.nonzero(exact)[0], np.nonzero(~exact)[0]])
    aD = np.empty((ncol, 2, Ns))
    j = 0
    for kk in order:
        for c in range(ncol):
            for li in range(2):
                aD[c, li, kk] = A_VALUES[j % A_VALUES.shape[0]]
                j += 1
    block = dataclasses.replace(block, phi=None, wphi=None)
    for a in (wl, vB, aD) + (() if vlos is None else (vlos,)):
        a.setflags(write=False)
    return prob, block, (aD, vB, vlos)


def samples(prob, prof, mus=None, both=True):
    """every sample of the profile chain at the angles `mus` (default: the problem's; compact: none), the way the kernels form it
    -> dict of arrays [SNl][nmu][ndir][ncol][Ns]: a, vb, v0, shift (signed), x = |v0 + shift|; ndir = 2 (down, up) or 1 (up only)"""
    aD, vB, vlos = prof
    mus = np.asarray(prob.muz if mus is None else mus, dtype=np.float64)
    if vlos is None:
        mus, both = np.array([0.0]), False
    sign = np.array([-1.0, 1.0]) if both else np.array([1.0])
    out = {k: [] for k in ('a', 'vb', 'v0', 'shift')}
    for li, t in enumerate(prob.lines):
        w = prob.wavelength[t.Nblue:t.Nblue + t.Nlambda]
        vb = vB[:, t.atom, :]
        v0 = (w[:, None, None] - t.lambda0) * CLIGHT / (vb[None] * t.lambda0)                    # [Nlam][ncol][Ns]
        vl = np.zeros_like(vb) if vlos is None else vlos
        sh = sign[None, :, None, None] * (mus[:, None, None, None] * vl[None, None] / vb[None, None])      # [nmu][ndir][ncol][Ns]
        shape = (t.Nlambda,) + sh.shape
        out['a'].append(np.broadcast_to(aD[:, li, :], shape))
        out['vb'].append(np.broadcast_to(vb, shape))
        out['v0'].append(np.broadcast_to(v0[:, None, None], shape))
        out['shift'].append(np.broadcast_to(sh[None], shape))
    out = {k: np.concatenate(v) for k, v in out.items()}
    out['x'] = np.abs(out['v0'] + out['shift'])
    return out


def coverage(s):
    """the cell counts of the samples `s` (one or several dicts of `samples`)"""
    many = [s] if isinstance(s, dict) else list(s)
    a = np.concatenate([q['a'].ravel() for q in many])
    x = np.concatenate([q['x'].ravel() for q in many])
    with np.errstate(divide='ignore'):
        row = np.where(a == 0, 0, 1 + np.clip(np.floor(np.log10(np.where(a == 0, 1.0, a))), -12, 3) + 12).astype(int)
    col = np.digitize(x, X_RANGES) - 1
    assert np.all((col >= 0) & (col < 6)) and np.all((row >= 0) & (row < 17))
    cells = np.zeros((17, 6), dtype=int)
    np.add.at(cells, (row, col), 1)
    fr = 2.0 * x - np.floor(2.0 * x)
    half = ~((fr >= 0.25) & (fr < 0.75))
    pole = (x < 27.0) & (a < TWO_PI)
    near = lambda f, lo, hi: int(np.sum((f >= lo) & (f < hi)))
    return dict(cells=cells,
                grids={(bool(h), bool(p)): int(np.sum((half == h) & (pole == p))) for h in (0, 1) for p in (0, 1)},
                quarter=(near(fr, 0.25 - 1e-3, 0.25), near(fr, 0.25, 0.25 + 1e-3)),
                three_quarters=(near(fr, 0.75 - 1e-3, 0.75), near(fr, 0.75, 0.75 + 1e-3)),
                x27=(near(x, 27.0 - 1e-3, 27.0), near(x, 27.0, 27.0 + 1e-3)),
                two_pi=(int(np.sum((a < TWO_PI) & (a > 6.0) & (x < 27.0))), int(np.sum((a >= TWO_PI) & (a < 6.6) & (x < 27.0)))),
                two_pi_doubles=(int(np.sum((a == A_SPECIAL[0]) & (x < 27.0))), int(np.sum((a == TWO_PI) & (x < 27.0)))))


def assert_coverage(cov):
    assert np.all(cov['cells'][:, :5] > 0), cov['cells']
    assert all(n > 0 for n in cov['grids'].values()), cov['grids']
    for key in ('quarter', 'three_quarters', 'x27'):
        assert min(cov[key]) >= 20, (key, cov[key])
    assert min(cov['two_pi']) > 0 and min(cov['two_pi_doubles']) > 0, (cov['two_pi'], cov['two_pi_doubles'])


@functools.lru_cache(maxsize=None)
def _reference(ncol, Ns, compact, mus, both):
    prob, block, prof = probe(ncol, Ns, compact)
    s = samples(prob, prof, None if mus is None else np.array(mus), both)
    aD, vB, vlos = prof
    shape = s['a'].shape
    H, lo, bar = np.empty(shape), np.empty(shape), np.empty(shape)
    MP.dps = 60
    mu = np.array([0.0]) if vlos is None else np.asarray(prob.muz if mus is None else mus, dtype=np.float64)
    sign = (-1.0, 1.0) if (both and vlos is not None) else (1.0,)
    c_mp = MP.mpf(CLIGHT)
    o = 0
    for t in prob.lines:
        for l in range(t.Nlambda):
            dl = (MP.mpf(float(prob.wavelength[t.Nblue + l])) - MP.mpf(t.lambda0)) * c_mp / MP.mpf(t.lambda0)
            for c in range(shape[3]):
                for k in range(shape[4]):
                    vb = MP.mpf(float(vB[c, t.atom, k]))
                    for m in range(shape[1]):
                        for d in range(shape[2]):
                            MP.dps = 60
                            sh = 0 if vlos is None else sign[d] * MP.mpf(float(mu[m])) * MP.mpf(float(vlos[c, k])) / vb
                            v = abs(dl / vb + sh)
                            i = (o + l, m, d, c, k)
                            h, dh = H_both(float(s['a'][i]), v)
                            MP.dps = 60
                            H[i], lo[i] = split(h)
                            cond = 4.0 * U * (abs(s['v0'][i]) + abs(s['shift'][i]))
                            bar[i] = TINY if h < TINY else float(BAR * h + abs(dh) * cond)
        o += t.Nlambda
    for a in (H, lo, bar):
        a.setflags(write=False)
    return s, H, lo, bar


def reference(ncol, Ns, compact, mus=None, both=True):
    """-> (samples, H_ref hi, H_ref lo, bar on H), arrays [SNl][nmu][ndir][ncol][Ns]; computed once per case"""
    return _reference(ncol, Ns, compact, None if mus is None else tuple(float(m) for m in mus), both)


def phi_reference(ncol, Ns, compact, mus=None, both=True):
    """-> (phi_ref hi, lo, bar on phi) in LSX_PHI's layout with the column first: [ncol][SNl][nmu][ndir][Ns] ([ncol][SNl][Ns] compact)"""
    s, H, lo, bar = reference(ncol, Ns, compact, mus, both)
    nrm = np.sqrt(np.pi) * s['vb']
    out = [np.moveaxis(a / nrm, 3, 0) for a in (H, lo, bar)]
    return [a[:, :, 0, 0, :] if compact else a for a in out]


def excess_phi(phi, ref):
    """the largest |phi - phi_ref| / bar over all entries, and where"""
    hi, lo, bar = ref
    r = np.abs((np.asarray(phi) - hi) - lo) / bar
    assert r.shape == np.asarray(phi).shape and np.all(np.isfinite(phi))
    return float(np.max(r)), np.unravel_index(int(np.argmax(r)), r.shape)


@functools.lru_cache(maxsize=None)
def wphi_reference(ncol, Ns, compact):
    """-> (wphi_ref [ncol][Nlines][Ns], relative bar): 1 / sum phi_ref wlambda wmu / 2, summed in mpmath"""
    prob, block, prof = probe(ncol, Ns, compact)
    s, H, lo, _ = reference(ncol, Ns, compact)
    out = np.empty((ncol, prob.Nlines, Ns))
    MP.dps = 60
    sqrt_pi, o = MP.sqrt(MP.pi), 0
    for li, t in enumerate(prob.lines):
        w = [MP.mpf(float(x)) for x in prob.wavelength[t.Nblue:t.Nblue + t.Nlambda]]
        n = t.Nlambda
        wla = [(w[1] - w[0]) / 2 if l == 0 else ((w[l] - w[l - 1]) / 2 if l == n - 1 else (w[l + 1] - w[l - 1]) / 2) for l in range(n)]
        wla = [x * MP.mpf(CLIGHT) / MP.mpf(t.lambda0) for x in wla]
        for c in range(ncol):
            for k in range(Ns):
                acc = MP.mpf(0)
                for l in range(n):
                    for m in range(prob.Nrays):
                        for d in range(2):
                            i = (o + l, 0, 0, c, k) if compact else (o + l, m, d, c, k)
                            acc += (MP.mpf(float(H[i])) + MP.mpf(float(lo[i]))) * wla[l] * MP.mpf(float(prob.wmu[m])) / 2
                out[c, li, k] = float(sqrt_pi * MP.mpf(float(prof[1][c, t.atom, k])) / acc)
        o += n
    nterms = max(t.Nlambda for t in prob.lines) * prob.Nrays * 2
    return out, BAR + (nterms + 2) * U


CASES = [(3, 13, True), (5, 13, True), (3, 13, False), (5, 13, False)]
