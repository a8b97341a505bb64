#!/usr/bin/env python3
"""Emergent spectra at arbitrary angles (lsx_hip_emergent_rays) against what it replaces: a second, zero-weight context whose
`muz` is the wanted angles and a full lsx_formal_sol_gamma on it.

    python3 profiles/rays_time.py [c3|c4|both] [--reps N] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -o rays --output-format csv -- python3 profiles/rays_time.py both --trace

C3's shape: 1000 FALC-perturbed CaII columns with ray-dependent profiles; C4's share: 1250 Ca + H columns.  Per shape, after a
warm-up of every call, the two alternatives are alternated `reps` times in this one process:
  new   host time of the whole Engine.emergent_rays call for nmu = 1 and 5 (kernels + the copy of the result to the host)
  old   lsx_time_formal_sol (device events, ms_total) of the zero-weight context with the same 5 angles -- the formal solution
        alone: building that context (a second copy of every column, the profiles at the new angles) is left out of the figure
--trace: a few untimed calls of each path only, for a kernel trace (kernel times come from the trace's statistics).
Bytes a column needs are computed from the shapes: what the kernel must read once and write once, against the 6.29 TB/s the
project uses as achievable bandwidth.  One JSON line per shape."""
import argparse
import dataclasses
import json
import os
import sys
import time

os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from lightspinner_amd import fixtures, synth, Engine, _capi  # noqa: E402

ACHIEVABLE_BPS = 6.29e12
MUS5 = np.array([0.2, 0.4, 0.6, 0.8, 1.0])


def needed_bytes_per_column(prob, nmu):
    """what one column's final pass must move: the four wavelength-by-depth streams (background opacity and emissivity, J, the
    continua's Boltzmann factor), populations, nStar ratios and geometry once, the profile inputs (aDamp, vBroad, vlos) once,
    and the result"""
    Ns, Nspect = prob.Nspace, prob.Nspect
    ncont = sum(1 for t in prob.trans if not t.is_line)
    streams = (4 if ncont else 3) * Nspect * Ns
    small = (prob.NLtot + ncont + 3) * Ns + (prob.Nlines + prob.Natoms + 1) * Ns
    return 8 * (streams + small + Nspect * nmu)


def kept_bytes_per_column(prob):
    """the extra device memory of the feature: aDamp, vBroad, vlos and a flag per column"""
    return 8 * (prob.Nlines + prob.Natoms + 1) * prob.Nspace + 1


def shape(workload, ncol, reps, trace):
    fixture = os.path.join(ROOT, 'tests', 'golden', 'falc_cah.npz' if workload == 'c4' else 'falc_ca.npz')
    prob, base, raw = fixtures.load_problem_npz(fixture, phi_compact=False)
    blk, prof = synth.perturbed_columns(prob, base, raw, ncol=ncol)
    eng = Engine(prob, ncol)
    synth.load_columns(eng, blk, prof)
    for it in range(5):
        eng.formal_sol_gamma()
        if it >= 3:
            eng.stat_equil()
    # the alternative: a second context on the wanted angles with zero weights, every column uploaded again, n and J copied over
    p2 = dataclasses.replace(prob, muz=MUS5.copy(), wmu=np.zeros(5))
    old = Engine(p2, ncol)
    synth.load_columns(old, blk, prof)
    old.set(_capi.LSX_N, eng.get(_capi.LSX_N))
    old.set(_capi.LSX_J, eng.get(_capi.LSX_J))
    # warm-up of every shape the timed window uses
    I5 = eng.emergent_rays(MUS5)
    eng.emergent_rays(MUS5[-1:])
    old.formal_sol_gamma()                     # (ONE call: with zero weights the next one starts from J = 0)
    Iold = old.get(_capi.LSX_I)
    old.time_formal_sol(2, 2)
    agree = float(np.max(np.abs(I5 - Iold) / np.abs(Iold)))
    if trace:
        for _ in range(3):
            eng.emergent_rays(MUS5)
            eng.emergent_rays(MUS5[-1:])
            old.formal_sol_gamma()
        return dict(workload=workload, columns=ncol, trace=True, new_against_old_rel=agree)
    t_new = {1: [], 5: []}
    t_old = []
    for _ in range(reps):
        for nmu in (1, 5):
            t0 = time.perf_counter()
            eng.emergent_rays(MUS5[5 - nmu:])
            t_new[nmu].append(1e3 * (time.perf_counter() - t0))
        t_old.append(old.time_formal_sol(0, 5)[0])
    med = lambda v: float(np.median(v))
    out = dict(workload=workload, columns=ncol, Nspect=prob.Nspect, Nspace=prob.Nspace, reps=reps,
               new_call_host_ms={str(k): dict(median=med(v), min=float(min(v)), max=float(max(v))) for k, v in t_new.items()},
               old_formal_sol_ms_total=dict(median=med(t_old), min=float(min(t_old)), max=float(max(t_old))),
               needed_bytes_per_column={str(k): needed_bytes_per_column(prob, k) for k in (1, 5)},
               kept_bytes_per_column=kept_bytes_per_column(prob),
               achievable_Bps=ACHIEVABLE_BPS, new_against_old_rel=agree)
    out['time_at_achievable_bandwidth_ms'] = {k: 1e3 * ncol * v / ACHIEVABLE_BPS for k, v in out['needed_bytes_per_column'].items()}
    eng.close(); old.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('workload', nargs='?', default='both', choices=['c3', 'c4', 'both'])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--columns', type=int, default=None)
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []
    for wl in (('c3', 'c4') if a.workload == 'both' else (a.workload,)):
        r = shape(wl, a.columns or (1000 if wl == 'c3' else 1250), a.reps, a.trace)
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
