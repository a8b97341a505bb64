#!/usr/bin/env python3
"""Ng acceleration of the MALI loop (lsx_hip_ng_configure): what k_ng_step adds to a statistical equilibrium, and what it saves.

    python3 profiles/ng_time.py [kernel|single|rf|all] [--reps N] [--order 1|2] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -o ng --output-format csv -- python3 profiles/ng_time.py kernel --trace

kernel  C3's shape (1000 FALC-perturbed CaII columns) and C4's share (1250 Ca + H columns).  Every timed call is
        lsx_stat_equil_async + lsx_sync (host time), behind an untimed formal solution so that the history moves; the calls of one
        cycle of order + 2 are told apart by their place in it: the first order + 1 store, the last extrapolates.  The same calls
        with Ng off are the baseline; the difference is what the launch adds.  --trace: a few untimed cycles only, for a kernel
        trace (k_ng_step's own durations come from the trace's statistics: the storing calls are order + 1 of every order + 2).
single  iterations to convergence (the reference's loop and thresholds) of one FALC CaII / Ca + H column, plain and with Ng, and
        the wall time of the loop.
rf      the CaII response function at every depth (164 perturbed columns, per-column stopping rule): per-column iteration counts,
        total wall time, and the largest |rf(Ng) - rf(plain)| relative to the largest |rf(plain)|.
One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from lightspinner_amd import fixtures, synth, Engine, _capi, drivers, response  # noqa: E402
from lightspinner_amd.problem import NgOptions  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def stats(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def kernel(workload, ncol, order, reps, trace):
    prob, base, raw = fixtures.load_problem_npz(os.path.join(GOLDEN, 'falc_cah.npz' if workload == 'c4' else 'falc_ca.npz'),
                                                phi_compact=False)
    blk, prof = synth.perturbed_columns(prob, base, raw, ncol=ncol)
    eng = Engine(prob, ncol)
    synth.load_columns(eng, blk, prof)
    for _ in range(3):
        eng.formal_sol_gamma()
    slots = order + 2

    def cycles(n, timed):
        t = [[] for _ in range(slots)]
        for _ in range(n):
            for p in range(slots):
                eng.formal_sol_gamma()
                t0 = time.perf_counter()
                eng.stat_equil_async()
                eng.sync()
                if timed:
                    t[p].append(1e3 * (time.perf_counter() - t0))
        return t

    cycles(2, False)                                     # warm-up, Ng off
    off = [x for p in cycles(0 if trace else reps, True) for x in p]
    eng.configure_ng(order)
    cycles(3 if trace else 2, False)
    st = eng.ng_state()
    out = dict(measurement='kernel', workload=workload, columns=ncol, order=order, elements_per_column=prob.NLtot * prob.Nspace,
               history_bytes=8 * slots * ncol * prob.NLtot * prob.Nspace, steps_taken=int(st.applied.sum()),
               steps_rejected=int(st.rejected.sum()))
    if not trace:
        on = cycles(reps, True)
        store, extra = [x for p in on[:-1] for x in p], on[-1]
        out.update(reps=reps, stat_equil_host_ms=dict(ng_off=stats(off), storing=stats(store), extrapolating=stats(extra)),
                   added_ms=dict(storing=float(np.median(store) - np.median(off)), extrapolating=float(np.median(extra) - np.median(off))))
    eng.close()
    return out


def loop(eng, ng):
    """the reference's loop on a one-column engine -> (iterations, wall ms)"""
    eng.configure_ng(ng)
    t0 = time.perf_counter()
    h = drivers.iterate_mali_engine(eng)
    return h.n_iter, 1e3 * (time.perf_counter() - t0), h.converged


def single(case, order):
    prob, block, _ = fixtures.load_problem_npz(os.path.join(GOLDEN, 'falc_%s.npz' % case))
    eng = Engine(prob, 1)
    out = dict(measurement='single', case=case, order=order)
    for name, ng in (('warm-up', None), ('plain', None), ('ng', NgOptions(order))):
        eng.set_columns(0, block)
        n, ms, ok = loop(eng, ng)
        if name != 'warm-up':
            out[name] = dict(iterations=n, wall_ms=ms, converged=ok)
    if out.get('ng'):
        st = eng.ng_state()
        out['ng'].update(steps=int(st.applied[0]), rejected=int(st.rejected[0]))
    eng.close()
    return out


def rf(order):
    prob, base, _ = fixtures.load_problem_npz(os.path.join(GOLDEN, 'falc_ca.npz'))
    fx = dict(np.load(os.path.join(GOLDEN, 'rf_ca_inputs.npz')))
    out = dict(measurement='rf', order=order, columns=2 * prob.Nspace)
    res = {}
    for name, ng in (('warm-up', None), ('plain', None), ('ng', NgOptions(order))):
        t0 = time.perf_counter()
        r = response.run_response_function(prob, base, fx, range(prob.Nspace), ng=ng)
        ms = 1e3 * (time.perf_counter() - t0)
        if name != 'warm-up':
            res[name] = r
            it = np.asarray(r['n_iter'])
            out[name] = dict(wall_ms=ms, base_iterations=r['n_iter_base'], iterations=it.tolist(), iterations_sum=int(it.sum()),
                             iterations_max=int(it.max()))
    d = np.abs(res['ng']['rf'] - res['plain']['rf'])
    out['max_abs_drf'] = float(d.max())
    out['max_abs_rf_plain'] = float(np.abs(res['plain']['rf']).max())
    out['max_drf_over_max_rf'] = out['max_abs_drf'] / out['max_abs_rf_plain']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('what', nargs='?', default='all', choices=['kernel', 'single', 'rf', 'all'])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--order', type=int, default=2, choices=[1, 2])
    ap.add_argument('--columns', type=int, default=None)
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []

    def emit(r):
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)

    if a.what in ('kernel', 'all'):
        for wl in ('c3', 'c4'):
            emit(kernel(wl, a.columns or (1000 if wl == 'c3' else 1250), a.order, a.reps, a.trace))
    if a.what in ('single', 'all') and not a.trace:
        for case in ('ca', 'cah'):
            emit(single(case, a.order))
    if a.what in ('rf', 'all') and not a.trace:
        emit(rf(a.order))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
