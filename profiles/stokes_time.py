#!/usr/bin/env python3
"""Full-Stokes emergent spectra (lsx_hip_stokes_rays) beside the two unpolarised final passes on the same columns and window.

    python3 profiles/stokes_time.py [--columns N] [--reps N] [--out FILE]

C3's shape: FALC-perturbed CaII columns with ray-dependent profiles, after five MALI iterations.  The window is that of the
854.2 nm line (854.44 nm in vacuum); the field is 0.1 T, inclined 45 degrees, azimuth 30 degrees, at every depth; the line carries
a normal triplet (effective Lande factor 1.1), the other lines stay unpolarised.  After a warm-up of every call the three entries are
alternated `reps` times in this one process, each at mu = 1 and at five angles:
  stokes   host time of the whole Engine.stokes_rays call (field upload, kernels, the copy of the result to the host)
  rays     Engine.emergent_rays (the WHOLE grid: the entry has no window; its time scaled by the window's share is given too)
  depth    Engine.depth_rays on the window (all six arrays)
One JSON line."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from lightspinner_amd import fixtures, synth, zeeman, Engine  # noqa: E402

MUS5 = np.array([0.2, 0.4, 0.6, 0.8, 1.0])


class _Triplet:
    gLandeEff = 1.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--columns', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    prob, base, raw = fixtures.load_problem_npz(os.path.join(ROOT, 'tests', 'golden', 'falc_ca.npz'), phi_compact=False)
    blk, prof = synth.perturbed_columns(prob, base, raw, ncol=a.columns)
    eng = Engine(prob, a.columns)
    synth.load_columns(eng, blk, prof)
    for it in range(5):
        eng.formal_sol_gamma()
        if it >= 3:
            eng.stat_equil()
    lines = [t for t in prob.trans if t.is_line]
    k = [i for i, t in enumerate(lines) if abs(t.lambda0 - 854.44) < 0.1][0]
    la0, nla = lines[k].Nblue, lines[k].Nlambda
    pats = [None] * len(lines)
    pats[k] = zeeman.zeeman_components(_Triplet())
    fld = (0.1, np.deg2rad(45.0), np.deg2rad(30.0))
    calls = {'stokes': lambda mu: eng.stokes_rays(mu, *fld, patterns=pats, la0=la0, nla=nla),
             'rays': lambda mu: eng.emergent_rays(mu),
             'depth': lambda mu: eng.depth_rays(mu, la0=la0, nla=nla)}
    for f in calls.values():
        for mu in (MUS5[-1:], MUS5):
            f(mu)
    s = calls['stokes'](MUS5)
    t = {(n, m): [] for n in calls for m in (1, 5)}
    for _ in range(a.reps):
        for m in (1, 5):
            for n, f in calls.items():
                t0 = time.perf_counter()
                f(MUS5[5 - m:])
                t[(n, m)].append(1e3 * (time.perf_counter() - t0))
    med = {n: {str(m): float(np.median(t[(n, m)])) for m in (1, 5)} for n in calls}
    out = dict(columns=a.columns, Nspace=prob.Nspace, Nspect=prob.Nspect, window=[int(la0), int(nla)], reps=a.reps, median_ms=med,
               min_ms={n: {str(m): float(min(t[(n, m)])) for m in (1, 5)} for n in calls},
               max_ms={n: {str(m): float(max(t[(n, m)])) for m in (1, 5)} for n in calls},
               rays_scaled_to_window_ms={str(m): med['rays'][str(m)] * nla / prob.Nspect for m in (1, 5)},
               stokes_over_depth={str(m): med['stokes'][str(m)] / med['depth'][str(m)] for m in (1, 5)},
               stokes_over_rays_scaled={str(m): med['stokes'][str(m)] / (med['rays'][str(m)] * nla / prob.Nspect) for m in (1, 5)},
               largest_V_over_I=float(np.max(np.abs(s.V) / s.I)))
    eng.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
