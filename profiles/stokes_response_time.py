#!/usr/bin/env python3
"""Response functions of the Stokes spectrum to the field vector (lsx_hip_response_stokes) beside the brute force they replace.

    python3 profiles/stokes_response_time.py [--columns N] [--reps N] [--work-cap-mib M] [--out FILE]

The shape of profiles/stokes_time.py: FALC-perturbed CaII columns with ray-dependent profiles, after five MALI iterations; the
window of the 854.2 nm line (854.44 nm in vacuum); 0.1 T, inclined 45 degrees, azimuth 30 degrees, at every depth; the line carries a
normal triplet (effective Lande factor 1.1).  All three parameters, all depths.  After a warm-up the two entries are alternated
`reps` times in this one process, each at mu = 1 and at five angles:
  response   host time of the whole Engine.stokes_response call (uploads, both stages, the Stokes pass behind them for the
             unperturbed vector, the copies of the results to the host)
  stokes     host time of one Engine.stokes_rays call of the same columns, window and angles
--work-cap-mib: the cap of the response's device memory (default: the library's 256 MiB); it decides into how many passes a call
is cut, and the walks of a pass are one launch whose time hardly depends on how many columns it holds.
Brute force needs 6 Nspace + 1 such Stokes calls; that product is given beside the response's time, and the two ratios.
The two stages apart are kernel times: run this script under a kernel trace,
    rocprofv3 --kernel-trace --stats -- python3 profiles/stokes_response_time.py --reps 3
and read k_response_nodes, k_response_walk and k_stokes_rays from the statistics.
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
    ap.add_argument('--columns', type=int, default=100)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--work-cap-mib', type=int, default=None)
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
    if a.work_cap_mib is not None:
        eng.stokes_response(MUS5[-1:], *fld, patterns=pats, la0=la0, nla=nla, ks=[0], work_cap_bytes=a.work_cap_mib << 20)
    calls = {'response': lambda mu: eng.stokes_response(mu, *fld, patterns=pats, la0=la0, nla=nla),
             'stokes': lambda mu: eng.stokes_rays(mu, *fld, patterns=pats, la0=la0, nla=nla)}
    for f in calls.values():
        for mu in (MUS5[-1:], MUS5):
            f(mu)
    r = calls['response'](MUS5)
    t = {(n, m): [] for n in calls for m in (1, 5)}
    for _ in range(a.reps):
        for m in (1, 5):
            for n, f in calls.items():
                t0 = time.perf_counter()
                f(MUS5[5 - m:])
                t[(n, m)].append(1e3 * (time.perf_counter() - t0))
    med = {n: {str(m): float(np.median(t[(n, m)])) for m in (1, 5)} for n in calls}
    nbrute = 6 * prob.Nspace + 1
    out = dict(columns=a.columns, work_cap_mib=a.work_cap_mib, Nspace=prob.Nspace, window=[int(la0), int(nla)], reps=a.reps, median_ms=med,
               min_ms={n: {str(m): float(min(t[(n, m)])) for m in (1, 5)} for n in calls},
               max_ms={n: {str(m): float(max(t[(n, m)])) for m in (1, 5)} for n in calls},
               brute_force_calls=nbrute,
               brute_force_ms={str(m): nbrute * med['stokes'][str(m)] for m in (1, 5)},
               response_over_one_stokes_call={str(m): med['response'][str(m)] / med['stokes'][str(m)] for m in (1, 5)},
               brute_force_over_response={str(m): nbrute * med['stokes'][str(m)] / med['response'][str(m)] for m in (1, 5)},
               largest_dV_dB_over_I=float(np.max(np.abs(r.rf['B'][:, 3]) / np.max(r.stokes.I))))
    eng.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
