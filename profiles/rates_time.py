#!/usr/bin/env python3
"""Radiative rates from a converged context (lsx_hip_radiative_rates) against one formal solution of the same context.

    python3 profiles/rates_time.py [c3|c4|both] [--reps N] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -o rates --output-format csv -- python3 profiles/rates_time.py both --trace
    LSX_HIP_LIBRARY=<another build> python3 profiles/rates_time.py both --fs-only      # the formal solution of that build alone

C3's shape: 1000 FALC-perturbed CaII columns with ray-dependent profiles; C4's share: 1250 Ca + H columns; both after five MALI
iterations.  Per shape, after a warm-up of every call, the two are alternated `reps` times in this one process:
  rates   host time of the whole Engine.radiative_rates call (both kernels per pass + the copy of the three results to the host)
  fs      lsx_time_formal_sol (device events, ms_total) of the same context
--trace: a few untimed calls of each only, for a kernel trace (kernel times come from the trace's statistics).
--fs-only: the formal solution alone (a library without the entry: the parent commit's, for the ratio on one box).
Bytes a column needs are computed from the shapes: what the pass must read once and write once, the work arrays written by the
first kernel and read by the second included, against the 6.29 TB/s the project uses as achievable bandwidth.  One JSON line per
shape."""
import argparse
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
WORK_CAP = 256 << 20


def work_bytes_per_column(prob):
    """the pass's work arrays: sum_mu (wmu / 2) I per (wavelength, depth), and the pair (sum phi I, sum phi) per (line wavelength, depth)"""
    return 8 * prob.Nspace * (prob.Nspect + 2 * prob.SNl)


def needed_bytes_per_column(prob):
    """what one column's pass must move: the wavelength-by-depth streams once (background opacity and emissivity, J, the continua's
    Boltzmann factor), the line profiles of every ray and direction once, populations, nStar ratios, wphi and geometry once, the
    work arrays written once and read once, and the three results"""
    Ns, Nspect = prob.Nspace, prob.Nspect
    ncont = sum(1 for t in prob.trans if not t.is_line)
    streams = (4 if ncont else 3) * Nspect * Ns
    phi = prob.SNl * Ns * (1 if prob.phi_compact else 2 * prob.Nrays)
    small = (prob.NLtot + ncont + prob.Nlines + 3) * Ns
    return 8 * (streams + phi + small + 3 * prob.Ntrans * Ns) + 2 * work_bytes_per_column(prob)


def shape(workload, ncol, reps, trace, fs_only):
    fixture = os.path.join(ROOT, 'tests', 'golden', 'falc_cah.npz' if workload == 'c4' else 'falc_ca.npz')
    prob, base, raw = fixtures.load_problem_npz(fixture, phi_compact=False)
    blk, prof = synth.perturbed_columns(prob, base, raw, ncol=ncol)
    eng = Engine(prob, ncol)
    synth.load_columns(eng, blk, prof)
    for it in range(5):
        eng.formal_sol_gamma()
        if it >= 3:
            eng.stat_equil()
    eng.time_formal_sol(2, 2)
    out = dict(workload=workload, columns=ncol, Nspect=prob.Nspect, Nspace=prob.Nspace, Ntrans=prob.Ntrans, reps=reps,
               library=eng.lib.path)
    if fs_only:
        t_fs = [eng.time_formal_sol(0, 5)[0] for _ in range(reps)]
        out['formal_sol_ms_total'] = dict(median=float(np.median(t_fs)), min=float(min(t_fs)), max=float(max(t_fs)))
        eng.close()
        return out
    r = eng.radiative_rates()                  # warm-up: tables, work arrays, staging
    eng.radiative_rates()
    assert all(np.all(np.isfinite(x)) and np.all(x > 0) for x in (r.Rij, r.Rji, r.Rji_ref))
    if trace:
        for _ in range(3):
            eng.radiative_rates()
            eng.formal_sol_gamma()
        eng.close()
        return dict(workload=workload, columns=ncol, trace=True)
    t_new, t_fs = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        eng.radiative_rates()
        t_new.append(1e3 * (time.perf_counter() - t0))
        t_fs.append(eng.time_formal_sol(0, 5)[0])
    med = lambda v: float(np.median(v))
    work = work_bytes_per_column(prob)
    per_pass = max(1, min(ncol, WORK_CAP // work))
    out.update(rates_call_host_ms=dict(median=med(t_new), min=float(min(t_new)), max=float(max(t_new))),
               formal_sol_ms_total=dict(median=med(t_fs), min=float(min(t_fs)), max=float(max(t_fs))),
               ratio_to_formal_sol=med(t_new) / med(t_fs),
               needed_bytes_per_column=needed_bytes_per_column(prob), work_bytes_per_column=work,
               columns_per_pass=per_pass, passes=-(-ncol // per_pass), work_bytes_allocated=per_pass * work,
               achievable_Bps=ACHIEVABLE_BPS)
    out['time_at_achievable_bandwidth_ms'] = 1e3 * ncol * out['needed_bytes_per_column'] / ACHIEVABLE_BPS
    out['achieved_Bps_whole_call'] = ncol * out['needed_bytes_per_column'] / (1e-3 * med(t_new))
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('workload', nargs='?', default='both', choices=['c3', 'c4', 'both'])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--columns', type=int, default=None)
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--fs-only', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []
    for wl in (('c3', 'c4') if a.workload == 'both' else (a.workload,)):
        r = shape(wl, a.columns or (1000 if wl == 'c3' else 1250), a.reps, a.trace, a.fs_only)
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
