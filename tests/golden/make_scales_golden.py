#!/usr/bin/env python3
"""Generate tests/golden/scales_falc.npz: the UNMODIFIED reference's AtmosphereConstructor.convert_scales
(atmosphere.py:70-144) on FALC and on columns made from it, on the three depth scales, with its own one-ulp envelope.

The reference is imported the way make_background_golden.py imports it, and that module's shifted_namespace moves every
exp / log / log10 of witt's namespace by +1 and by -1 unit in the last place.  Numbers only are written.  Per case `name`:
  <name>_scale                        0 geometric, 1 column mass, 2 tau500 (ScaleType's values)
  <name>_depth_scale, _temperature, _nHTot, _ne      the inputs, SI, [N]
  <name>_height, _cmass, _tau_ref, _chi_c            the reference's results, [3][N]: shift 0, +1, -1
(chi_c is what convert_scales puts into its local chi_c: the value of eos.contOpacity(...) / CM_TO_M is recorded on its way there.)
Cases:
  falc_<scale>            FALC (fal.py's Falc82) on its own column-mass scale; geometric takes the height and tau500 the tau_ref
                          of the column-mass result
  s<a>_<b>_<scale>        the depth slices [a:b] of the same
  p<i>_<scale>            six smoothly perturbed FALC columns (temperature, nHTot, ne), geometric / tau500 from each column's own
                          column-mass result
  fine_cm                 FALC refined to 325 depths, column mass
Every geometric case's raw tau[0] = 0.5 chi_c[0] (h[0] - h[1]) is asserted to be at least 1e-3 relative away from 1 (the
reference sets it to 0 above 1: no case sits on that switch).

Usage:  python tests/golden/make_scales_golden.py [--check]
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import make_background_golden as mbg  # noqa: E402

SCALES = ('geo', 'cm', 'tau')             # index = ScaleType's value
SLICES = ((0, 40), (70, 82), (60, 62), (80, 82), (78, 82), (25, 58))
LOGG = 2.44
NPERT = 6


class _Recorder:
    """stands in for the name `witt` of atmosphere.py: the same class, its contOpacity's results noted"""

    def __init__(self, cls, cm_to_m):
        self.cls, self.cm_to_m, self.chi = cls, cm_to_m, []

    def __call__(self):
        eos = self.cls()
        inner = eos.contOpacity

        def noting(*a, **k):
            r = inner(*a, **k)
            self.chi.append(float(np.asarray(r / self.cm_to_m).reshape(-1)[0]))
            return r
        eos.contOpacity = noting
        return eos


def _constructor(atmosphere, scale, ds, T, nH, ne):
    """an AtmosphereConstructor as nondimensionalise() leaves it (no units are involved in what convert_scales computes)"""
    ac = object.__new__(atmosphere.AtmosphereConstructor)
    ac.depthScale, ac.temperature, ac.nHTot, ac.ne = (np.array(a, dtype=np.float64) for a in (ds, T, nH, ne))
    ac.scale = atmosphere.ScaleType(scale)
    ac.vlos, ac.vturb, ac.hydrogenPops = np.zeros(len(ds)), np.zeros(len(ds)), None
    ac.lowerBc, ac.upperBc = atmosphere.BoundaryCondition.Thermalised, atmosphere.BoundaryCondition.Zero
    ac.mux = ac.muy = ac.muz = ac.wmu = None
    ac.dimensioned = False
    return ac


def run_case(ref, scale, ds, T, nH, ne):
    """-> dict of [3][N] arrays: the reference at shift 0, +1, -1"""
    witt, atmosphere, Const = ref
    out = {k: [] for k in ('height', 'cmass', 'tau_ref', 'chi_c')}
    for shift in (0, +1, -1):
        rec = _Recorder(witt.witt, Const.CM_TO_M)
        keep = atmosphere.witt
        atmosphere.witt = rec
        mbg.shifted_namespace(witt, shift)
        try:
            ac = _constructor(atmosphere, scale, ds, T, nH, ne)
            ac.convert_scales(logG=LOGG)
        finally:
            mbg.shifted_namespace(witt, 0)
            atmosphere.witt = keep
        assert len(rec.chi) == len(ds)
        for k, v in (('height', ac.height), ('cmass', ac.cmass), ('tau_ref', ac.tau_ref), ('chi_c', rec.chi)):
            out[k].append(np.array(np.asarray(v), dtype=np.float64).reshape(-1))
    return {k: np.array(v) for k, v in out.items()}


def perturbed(i, T, nH, ne):
    x = np.linspace(0.0, 1.0, len(T))
    a = 0.01 + 0.008 * i
    Tp = T * (1.0 + a * np.sin(2 * np.pi * (1 + 0.5 * i) * x + 0.7 * i))
    nHp = nH * np.exp(3 * a * np.cos(2 * np.pi * (0.5 + 0.4 * i) * x + 0.3 * i))
    nep = ne * np.exp(2 * a * np.sin(2 * np.pi * (0.8 + 0.3 * i) * x + 1.1 * i))
    return Tp, nHp, nep


def refined(cm, T, nH, ne, sub=4):
    """every interval cut into `sub`: linear in log(cmass), log(nHTot), log(ne) and in T against the depth index"""
    n = len(cm)
    xi = np.arange(n, dtype=np.float64)
    xo = np.arange((n - 1) * sub + 1, dtype=np.float64) / sub
    f = lambda y: np.interp(xo, xi, y)
    return np.exp(f(np.log(cm))), f(T), np.exp(f(np.log(nH))), np.exp(f(np.log(ne)))


def generate():
    witt, Const, wph = mbg._import_reference()
    import atmosphere
    from fal import Falc82
    ref = (witt, atmosphere, Const)
    ac = Falc82()
    ac.nondimensionalise()
    cm, T, nH, ne = (np.array(np.asarray(a), dtype=np.float64) for a in (ac.depthScale, ac.temperature, ac.nHTot, ac.ne))
    assert ac.scale is atmosphere.ScaleType.ColumnMass and T.min() >= 2500.0
    d = {'logG': np.float64(LOGG), 'weight_per_H': np.float64(wph)}
    names = []
    t0 = time.time()

    def add(name, scale, ds, T_, nH_, ne_):
        r = run_case(ref, scale, ds, T_, nH_, ne_)
        d[name + '_scale'] = np.int32(scale)
        for k, v in (('depth_scale', ds), ('temperature', T_), ('nHTot', nH_), ('ne', ne_)):
            d['%s_%s' % (name, k)] = np.array(v, dtype=np.float64)
        for k, v in r.items():
            d['%s_%s' % (name, k)] = v
        if scale == 0:
            raw = 0.5 * r['chi_c'][:, 0] * (ds[0] - ds[1])
            assert np.all(np.abs(raw - 1.0) >= 1e-3), (name, raw)
            print('  %s: raw tau[0] %.3g, returned tau %s' % (name, raw[0], r['tau_ref'][0][:4]))
        assert np.all(np.diff(r['tau_ref'], axis=1) > 0), name
        names.append(name)
        print('%-14s N = %3d, tau %.3g .. %.3g, height %.6g .. %.6g (%.0f s)' % (name, len(ds), r['tau_ref'][0][0], r['tau_ref'][0][-1],
              r['height'][0][0], r['height'][0][-1], time.time() - t0), flush=True)
        return r

    def three(prefix, cm_, T_, nH_, ne_, slices=()):
        base = add(prefix + '_cm', 1, cm_, T_, nH_, ne_)
        h, tau = base['height'][0], base['tau_ref'][0]
        add(prefix + '_geo', 0, h, T_, nH_, ne_)
        add(prefix + '_tau', 2, tau, T_, nH_, ne_)
        for a, b in slices:
            s = slice(a, b)
            for sc, ds in ((1, cm_), (0, h), (2, tau)):
                add('s%d_%d_%s' % (a, b, SCALES[sc]), sc, ds[s], T_[s], nH_[s], ne_[s])

    three('falc', cm, T, nH, ne, SLICES)
    for i in range(NPERT):
        three('p%d' % i, cm, *perturbed(i, T, nH, ne))
    add('fine_cm', 1, *refined(cm, T, nH, ne))
    d['cases'] = np.array(names)
    return d


def main():
    d = generate()
    path = os.path.join(HERE, 'scales_falc.npz')
    if '--check' in sys.argv[1:]:
        old = np.load(path)
        bad = [k for k in d if k not in old.files or not np.array_equal(old[k], d[k])] + [k for k in old.files if k not in d]
        print('check: %d arrays, %d differ %s' % (len(d), len(bad), bad))
        sys.exit(1 if bad else 0)
    np.savez_compressed(path, **d)
    size = os.path.getsize(path)
    print('wrote %s (%.1f kB)' % (path, size / 1e3))
    assert size < (1 << 20), size
    # the relative envelopes of the reference itself
    for sc in (1, 2, 0):
        for q in ('tau_ref', 'cmass', 'height'):
            w = 0.0
            for n in d['cases']:
                if int(d[n + '_scale']) != sc:
                    continue
                r = d['%s_%s' % (n, q)]
                s = np.abs(r[0]) + (np.abs(r[0][0]) if q == 'height' else 0.0)
                w = max(w, float(np.max(np.abs(r[1] - r[2]) / np.maximum(s, 1e-300))))
            print('largest relative envelope, %s scale, %s: %.3g' % (SCALES[sc], q, w))


if __name__ == '__main__':
    main()
