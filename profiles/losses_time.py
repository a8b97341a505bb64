#!/usr/bin/env python3
"""Radiative flux and net cooling from a converged context (lsx_hip_radiative_losses) beside the radiative rates of the same
context (lsx_hip_radiative_rates): the same walk with two angle sums fewer, the yardstick.

    python3 profiles/losses_time.py [c3|c4|both] [--reps N] [--columns N] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -o losses --output-format csv -- python3 profiles/losses_time.py both --trace

C3's shape: 1000 FALC-perturbed CaII columns with ray-dependent profiles; C4's share: 1250 Ca + H columns; both after five MALI
iterations.  Per shape, after a warm-up of every call, the two are alternated `reps` times in this one process on this one context:
  losses  host time of the whole Engine.radiative_losses call for F, Q and Qt (the pass, the two reductions, the copy to the host)
  rates   host time of the whole Engine.radiative_rates call (its pass, its reduction, the copy of the three results)
and once more with the monochromatic H and D asked for (the transpose and 2 x Nspect x Nspace doubles per column over the link).
--trace: a few untimed calls of each only, for a kernel trace (kernel times come from the trace's statistics).
Bytes a column needs are computed from the shapes as profiles/rates_time.py does, with three work arrays per (wavelength, depth)
in place of one.  One JSON line per shape."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from lightspinner_amd import fixtures, synth, Engine  # noqa: E402

ACHIEVABLE_BPS = 6.29e12
WORK_CAP = 256 << 20


def work_bytes_per_column(prob):
    """the pass's work arrays: H, D and sum (wmu / 2) I per (wavelength, depth), the pair (sum phi I, sum phi) per (line wavelength, depth)"""
    return 8 * prob.Nspace * (3 * prob.Nspect + 2 * prob.SNl)


def needed_bytes_per_column(prob):
    """what one column's pass must move: the wavelength-by-depth streams once (background opacity and emissivity, J, the continua's
    Boltzmann factor), the line profiles of every ray and direction once, populations, nStar ratios, wphi and geometry once, the
    work arrays written once and read once, and F, Q and Qt"""
    Ns, Nspect = prob.Nspace, prob.Nspect
    ncont = sum(1 for t in prob.trans if not t.is_line)
    streams = (4 if ncont else 3) * Nspect * Ns
    phi = prob.SNl * Ns * (1 if prob.phi_compact else 2 * prob.Nrays)
    small = (prob.NLtot + ncont + prob.Nlines + 3) * Ns
    return 8 * (streams + phi + small + (2 + prob.Ntrans) * Ns) + 2 * work_bytes_per_column(prob)


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
    out = dict(workload=workload, columns=ncol, Nspect=prob.Nspect, Nspace=prob.Nspace, Ntrans=prob.Ntrans, reps=reps,
               library=eng.lib.path)
    for _ in range(2):                         # warm-up: tables, work arrays, staging
        L = eng.radiative_losses(what=('F', 'Q', 'Qt', 'H', 'D'))
        eng.radiative_losses()
        eng.radiative_rates()
    assert all(np.all(np.isfinite(x)) for x in (L.F, L.Q, L.Qt, L.H, L.D)) and np.all(L.F[:, 0] > 0)
    if trace:
        for _ in range(3):
            eng.radiative_losses()
            eng.radiative_rates()
        eng.close()
        return dict(workload=workload, columns=ncol, trace=True)
    t_new, t_all, t_rates = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        eng.radiative_losses()
        t1 = time.perf_counter()
        eng.radiative_rates()
        t2 = time.perf_counter()
        eng.radiative_losses(what=('F', 'Q', 'Qt', 'H', 'D'))
        t3 = time.perf_counter()
        t_new.append(1e3 * (t1 - t0))
        t_rates.append(1e3 * (t2 - t1))
        t_all.append(1e3 * (t3 - t2))
    stats = lambda v: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
    work = work_bytes_per_column(prob)
    per_pass = max(1, min(ncol, WORK_CAP // work))
    out.update(losses_call_host_ms=stats(t_new), rates_call_host_ms=stats(t_rates), losses_with_H_D_call_host_ms=stats(t_all),
               ratio_to_rates=float(np.median(t_new) / np.median(t_rates)),
               needed_bytes_per_column=needed_bytes_per_column(prob), work_bytes_per_column=work,
               columns_per_pass=per_pass, passes=-(-ncol // per_pass), work_bytes_allocated=per_pass * work,
               achievable_Bps=ACHIEVABLE_BPS)
    out['time_at_achievable_bandwidth_ms'] = 1e3 * ncol * out['needed_bytes_per_column'] / ACHIEVABLE_BPS
    out['achieved_Bps_whole_call'] = ncol * out['needed_bytes_per_column'] / (1e-3 * float(np.median(t_new)))
    eng.close()
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
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
