#!/usr/bin/env python3
"""Generate tests/golden/background_eos.npz: the UNMODIFIED reference's equation of state and continuous opacity
(witt.py, background.py:15-53), point by point, with its own one-ulp envelope.

The reference is imported the way make_golden.py imports it.  Numbers only are written:
  tables     tpf, the first 28 elements' pf / eion / nstage, the 99 abundances as read (before witt.__init__ normalises
             them) and masses, weightPerH, and the reference's own avw, ab_others, rho_from_H
  points     'falc'   the 82 FALC points (temperature, nHTot of falc_ca.npz)
             'rf'     the 164 response-function points: depth k at T[k] + 25 K (rows 0..81) and T[k] - 25 K (rows 82..163)
             'grid'   the branch grid: 22 temperatures on either side of every literal temperature switch, each at FALC's
                      smallest, geometric-mean and largest nHTot (row = 22 * density + temperature)
  per point  pgas, pe, the 17 partials, the number of witt.pe_pg evaluations (npepg), the number of values compared with
             eos.prec (nstop) and margin = min |dif - prec| / prec over them (asserted >= 1e-5: no point is near a flip)
  chi        on the branch grid at the two wavelengths (c / nu0)(1 +- 1e-6) of every literal frequency nu0 of witt.py:778-1362
             whose wavelength lies in [20 nm, 10 um], and at 40, 500, 5000 nm
  envelope   the same quantities with every exp / log / log10 of witt's namespace (the math names and np.exp) moved by +1 and
             by -1 unit in the last place: *_env = |x(+1) - x(-1)|.  For chi on FALC and on the response-function points the
             plain values are in falc_*.npz / rf_ca_inputs.npz already: only the envelope is written, for the union of the
             three FALC grids' wavelengths, as the relative width |x(+1) - x(-1)| / |x| scaled by 2^50 and rounded TOWARDS
             ZERO to float16 (a bound made from it is never wider than the exact one).

Usage:  python tests/golden/make_background_golden.py [--check]
"""
import math
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

RAW_ABUND = None


def _import_reference():
    global RAW_ABUND
    import make_golden as mg  # noqa: F401  (puts the reference and the stand-ins on sys.path)
    import witt
    import constants as Const
    from atomic_table import get_global_atomic_table
    if RAW_ABUND is None:
        RAW_ABUND = np.array(witt.witt.ABUND)       # witt.__init__ normalises the class attribute in place (witt.py:166-167)
    return witt, Const, get_global_atomic_table().weightPerH


T_GRID = [900., 1000., 1500., 1999., 2001., 3999., 4001., 5000., 6999., 7729., 7731., 7999., 8001., 9000., 11999., 12001.,
          20000., 29999., 30001., 60000., 1e5, 1.5e5]
ENV_SCALE = 2.0 ** 50


def literal_frequencies():
    """every literal frequency of witt.py:778-1362 (edges and switches), Hz"""
    nu = [4.05933E13, 2.463e15, 3.28805E15, 1.8259E14, 2.111E14, 2.055E14, 1.31522E14, 5.15e15, 2.7254E15, 2.4196E15, 2.0761E15,
          1.443E15, 3.517915E15, 2.941534E15, 2.653317E15, 3.635492E15, 2.564306E15, 2.870454e15, 2.460127e15, 2.110779e15,
          2.922E15, 21000. * 2.99792458E10]
    import witt
    for tab in (witt.HEFREQ0, witt.FREQMG, witt.FREQSI1, witt.FREQSI2):
        nu += [float(x) for x in tab]
    nu += [float(x) * 2.99792458E10 for x in np.unique(witt.WNO1)]
    for Z, nmax in ((1.0, 8), (2.0, 9)):           # COULX's edges (witt.py:827)
        nu += [Z * Z * 3.28805e15 / (N + 1.0) ** 2 for N in range(nmax)]
    return np.unique(np.array(nu))


def edge_wavelengths():
    lam = 2.997925e18 / literal_frequencies() / 10.0          # nm
    lam = lam[(lam >= 20.0) & (lam <= 1.0e4)]
    w = np.concatenate([lam * (1 - 1e-6), lam * (1 + 1e-6), [40.0, 500.0, 5000.0]])
    return np.unique(w)


class Prec:
    """stands in for eos.prec: records every value compared with it"""
    __array_ufunc__ = None
    value = 1.e-5

    def __init__(self):
        self.seen = []

    def _note(self, x):
        self.seen.append(float(x))
        if len(self.seen) > 20000:
            raise RuntimeError('the reference does not terminate at this point')
        return float(x)

    def __lt__(self, x): return self.value < self._note(x)      # x > prec
    def __le__(self, x): return self.value <= self._note(x)     # x >= prec
    def __gt__(self, x): return self.value > self._note(x)
    def __ge__(self, x): return self.value >= self._note(x)


class _NpProxy:
    def __init__(self, shift):
        self._shift = shift

    def __getattr__(self, name):
        return getattr(np, name)

    def exp(self, x):
        return np.nextafter(np.exp(x), self._shift * np.inf)


def shifted_namespace(witt, shift):
    """witt's exp / log / log10 (math) and np.exp moved by `shift` units in the last place; 0 restores"""
    for name in ('exp', 'log', 'log10'):
        f = getattr(math, name)
        setattr(witt, name, f if shift == 0 else (lambda x, f=f: math.nextafter(f(x), shift * math.inf)))
    witt.np = np if shift == 0 else _NpProxy(shift)


def run_points(witt, Const, wph, T, nH, wl_nm=None, wl_at=None, log=''):
    """-> dict of arrays over the points.  wl_nm: wavelengths for chi at every point; wl_at: per point, or None"""
    eos = witt.witt()
    prec = Prec()
    eos.prec = prec
    count = [0]
    inner = eos.pe_pg

    def counting(*a, **k):
        count[0] += 1
        return inner(*a, **k)
    eos.pe_pg = counting
    n = len(T)
    out = {'pgas': np.zeros(n), 'pe': np.zeros(n), 'partials': np.zeros((n, 17)), 'npepg': np.zeros(n, np.int32),
           'nstop': np.zeros(n, np.int32), 'margin': np.zeros(n)}
    if wl_nm is not None:
        out['chi'] = np.zeros((n, len(wl_nm)))
    t0 = time.time()
    for i in range(n):
        t, nh = np.float64(T[i]), np.float64(nH[i])
        rho = Const.Amu * wph * nh * Const.CM_TO_M**3 / Const.G_TO_KG
        prec.seen, count[0] = [], 0
        out['pgas'][i] = eos.pg_from_rho(t, rho)
        out['pe'][i] = eos.pe_from_rho(t, rho)
        out['npepg'][i], out['nstop'][i] = count[0], len(prec.seen)
        out['margin'][i] = np.min(np.abs(np.array(prec.seen) - prec.value) / prec.value)
        out['partials'][i] = eos.getBackgroundPartials(t, out['pgas'][i], out['pe'][i], divide_by_u=True)
        if wl_nm is not None:
            out['chi'][i] = eos.contOpacity(t, out['pgas'][i], out['pe'][i], np.asarray(wl_nm) * 10) / Const.CM_TO_M
        if log and (i % 20 == 19 or i == n - 1):
            print('  %s: %d / %d (%.0f s)' % (log, i + 1, n, time.time() - t0), flush=True)
    return out, eos


def encode_rel(width, plain):
    """relative width * 2^50 as float16, rounded towards zero"""
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(plain != 0, width / np.abs(plain), 0.0) * ENV_SCALE
    h = r.astype(np.float16)
    over = h.astype(np.float64) > r
    h[over] = np.nextafter(h[over], np.float16(0))
    assert np.all(np.isfinite(h)) and np.all(h.astype(np.float64) <= r)
    return h


def generate():
    witt, Const, wph = _import_reference()
    falc = np.load(os.path.join(HERE, 'falc_ca.npz'))
    Tf, nHf = falc['temperature'].astype(np.float64), falc['nHTot'].astype(np.float64)
    sets = {'falc': (Tf, nHf),
            'rf': (np.concatenate([Tf + 25.0, Tf - 25.0]), np.concatenate([nHf, nHf])),
            'grid': (np.tile(np.array(T_GRID), 3), np.repeat(np.array([nHf.min(), np.exp(np.mean(np.log(nHf))), nHf.max()]), len(T_GRID)))}
    w_edge = edge_wavelengths()
    w_falc = np.unique(np.concatenate([np.load(os.path.join(HERE, f))['wavelength'] for f in ('falc_ca.npz', 'falc_cah.npz', 'falc_all.npz')]))
    w_rf = np.array(falc['wavelength'])
    grids = {'falc': w_falc, 'rf': w_rf, 'grid': w_edge}

    d = {'T_grid': np.array(T_GRID), 'grid_wavelength': w_edge, 'falc_env_wavelength': w_falc, 'rf_env_wavelength': w_rf,
         'env_scale': np.float64(ENV_SCALE), 'weight_per_H': np.float64(wph)}
    res = {}
    for shift in (0, +1, -1):
        shifted_namespace(witt, shift)
        try:
            for name, (T, nH) in sets.items():
                res[name, shift], eos = run_points(witt, Const, wph, T, nH, wl_nm=grids[name], log='%s %+d' % (name, shift))
        finally:
            shifted_namespace(witt, 0)
        if shift == 0:
            # the tables of lsx_eos_tables, and what witt.__init__ derives from the abundances
            d['abund'], d['amass'], d['tpf'] = RAW_ABUND, np.array(witt.witt.AMASS), np.array(eos.tpf)
            ne = 28
            d['nstage'] = np.array([eos.el[i].nstage for i in range(ne)], np.int32)
            pf, eion = np.zeros((ne, 6, len(eos.tpf))), np.zeros((ne, 6))
            for i in range(ne):
                pf[i, :d['nstage'][i]] = eos.el[i].pf
                eion[i, :d['nstage'][i]] = eos.el[i].eion
            d['pf'], d['eion'] = pf, eion
            d['ref_avw'], d['ref_ab_others'], d['ref_rho_from_H'] = np.float64(eos.avw), np.float64(eos.ab_others), np.float64(eos.rho_from_H)
    for name, (T, nH) in sets.items():
        p, up, dn = res[name, 0], res[name, 1], res[name, -1]
        d[name + '_temperature'], d[name + '_nHTot'] = T, nH
        for key in ('pgas', 'pe', 'partials', 'npepg', 'nstop', 'margin'):
            d['%s_%s' % (name, key)] = p[key]
        for key in ('pgas', 'pe', 'partials'):
            d['%s_%s_env' % (name, key)] = np.abs(up[key] - dn[key])
        assert np.all(p['margin'] >= 1e-5), (name, p['margin'].min())
        print('%s: smallest stop-test margin %.3g, most stop tests %d, most pe_pg evaluations %d' %
              (name, p['margin'].min(), p['nstop'].max(), p['npepg'].max()))
        env = np.abs(up['chi'] - dn['chi'])
        if name == 'grid':
            d['grid_chi'], d['grid_chi_env'] = p['chi'], env
        elif name == 'falc':
            d['falc_chi_env16'] = encode_rel(env, p['chi']).T.copy()            # [nw][82]
            for f in ('falc_ca.npz', 'falc_cah.npz', 'falc_all.npz'):           # the plain values are the committed backgrounds
                g = np.load(os.path.join(HERE, f))
                idx = np.searchsorted(w_falc, g['wavelength'])
                dev = np.max(np.abs(p['chi'].T[idx] - g['bg_chi']) / g['bg_chi'])
                print('  %s: regenerated chi vs the committed bg_chi: %.3g' % (f, dev))
                assert dev < 1e-11, (f, dev)
        else:
            d['rf_chi_env16'] = encode_rel(env, p['chi'])                       # [164][287]: point (k, +-) at depth k
    return d


def main():
    d = generate()
    path = os.path.join(HERE, 'background_eos.npz')
    if '--check' in sys.argv[1:]:
        old = np.load(path)
        bad = [k for k in d if k not in old.files or not np.array_equal(old[k], d[k])] + [k for k in old.files if k not in d]
        print('check: %d arrays, %d differ %s' % (len(d), len(bad), bad))
        sys.exit(1 if bad else 0)
    np.savez_compressed(path, **d)
    size = os.path.getsize(path)
    print('wrote %s (%.1f kB)' % (path, size / 1e3))
    assert size < (1 << 20), size


if __name__ == '__main__':
    main()
