#!/usr/bin/env python3
"""The penalty and the uncertainties of a regularised field fit (lsx_hip_regular_penalty, lsx_hip_regular_uncertainty) beside the calls
of the fit they follow, and a whole regularised fit beside the plain one.

    python3 profiles/fit_regular_time.py [--columns N] [--reps N] [--loop-reps N] [--angles 1|5] [--max-iter N] [--out FILE]

The workload of profiles/fit_time.py and profiles/fit_instrument_time.py at 1000 columns: FALC-perturbed CaII columns with
ray-dependent profiles after five MALI iterations; the window of the 854.2 nm line with a normal triplet; the observation is the
spectrum of 0.1 T, 45 degrees, 30 degrees at every depth, weights 1 / (1e-3 max I)^2; hat nodes over the depth index, off the truth.
Two parameterisations: P = 6 (four B nodes, one each for gammaB and chiB) and P = 24 (eight each); the penalty is
Penalty.smoothness(order=2) with 1e6 T^-2, 1e2 rad^-2, 1e2 rad^-2 (it vanishes on the truth, so both loops walk to the same minimum).
After a warm-up of every call, alternated `reps` times in this one process, host time of the whole call (each ends in a stream
synchronise):
    fit_field_normal, fit_field_penalty (with grad and hess), fit_field_penalty (chi2 alone), fit_field_uncertainty (the sandwich)
then, alternated `loop-reps` times:
    the plain fit_field_columns, the regularised one with uncertainty=True
both from the same start, with the same bounds (B in [1e-3, 1] T, gammaB in [0, pi], chiB in [-pi, pi]) and the same cap on the
iterations.  The spread of the plain loop is the yardstick for the difference.
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

from lightspinner_amd import _capi, drivers, fit, fixtures, synth, zeeman, Engine  # noqa: E402

MUS5 = np.array([0.2, 0.4, 0.6, 0.8, 1.0])
ALPHA = {'B': 1e6, 'gammaB': 1e2, 'chiB': 1e2}


class _Triplet:
    gLandeEff = 1.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--columns', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--loop-reps', type=int, default=3)
    ap.add_argument('--angles', type=int, default=1, choices=(1, 5))
    ap.add_argument('--max-iter', type=int, default=8)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    prob, base, raw = fixtures.load_problem_npz(os.path.join(ROOT, 'tests', 'golden', 'falc_ca.npz'), phi_compact=False)
    blk, prof = synth.perturbed_columns(prob, base, raw, ncol=a.columns)
    eng = Engine(prob, a.columns, lib=_capi.load_hip_library())
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
    Ns, nc = prob.Nspace, a.columns
    mus = MUS5 if a.angles == 5 else np.array([1.0])
    st = eng.stokes_rays(mus, 0.1, np.deg2rad(45.0), np.deg2rad(30.0), patterns=pats, la0=la0, nla=nla)
    obs = np.stack([st.I, st.Q, st.U, st.V], axis=1)
    w = np.broadcast_to((1.0 / (1e-3 * obs[:, 0].max(axis=(1, 2))) ** 2)[:, None, None, None], obs.shape).copy()
    kw = dict(patterns=pats, la0=la0, nla=nla)
    out = dict(columns=nc, Nspace=Ns, window=[int(la0), int(nla)], angles=len(mus), reps=a.reps, loop_reps=a.loop_reps, max_iter=a.max_iter,
               library=eng.lib.path, cases={})
    hat = lambda n: fit.hat_basis(np.arange(Ns), np.linspace(0, Ns - 1, n)) if n > 1 else np.ones((1, Ns))
    for nnode in ((4, 1, 1), (8, 8, 8)):
        basis, _ = fit.stack_basis(B=hat(nnode[0]), gammaB=hat(nnode[1]), chiB=hat(nnode[2]))
        P = sum(nnode)
        truth = np.tile(np.concatenate([np.full(nnode[0], 0.1), np.full(nnode[1], np.deg2rad(45.0)), np.full(nnode[2], np.deg2rad(30.0))]), (nc, 1))
        start = truth * np.concatenate([np.full(nnode[0], 1.1), np.ones(nnode[1] + nnode[2])]) \
            + np.concatenate([np.zeros(nnode[0]), np.full(nnode[1], 0.09), np.full(nnode[2], -0.09)])
        pen = fit.Penalty.smoothness(nnode, ALPHA, order=2)
        ne = eng.fit_field_normal(mus, basis, nnode, start, obs, weight=w, **kw)
        calls = {'fit_field_normal': lambda: eng.fit_field_normal(mus, basis, nnode, start, obs, weight=w, **kw),
                 'fit_field_penalty': lambda: eng.fit_field_penalty(start, pen, ne.chi2, ne.grad, ne.hess),
                 'fit_field_penalty, chi2 alone': lambda: eng.fit_field_penalty(start, pen, ne.chi2),
                 'fit_field_uncertainty': lambda: eng.fit_field_uncertainty(ne.hess, basis, nnode, penalty=pen)}
        lo = np.concatenate([np.full(nnode[0], 1e-3), np.zeros(nnode[1]), np.full(nnode[2], -np.pi)])       # B in T, the angles in rad
        hi = np.concatenate([np.ones(nnode[0]), np.full(nnode[1], np.pi), np.full(nnode[2], np.pi)])
        loop = dict(weight=w, lo=lo, hi=hi, max_iter=a.max_iter, **kw)
        loops = {'plain loop': lambda: drivers.fit_field_columns(eng, obs, mus, basis, start, nnode, **loop),
                 'regularised loop, uncertainty': lambda: drivers.fit_field_columns(eng, obs, mus, basis, start, nnode, penalty=pen,
                                                                                    uncertainty=True, **loop)}
        first = {c: f() for c, f in list(calls.items()) + list(loops.items())}              # the warm-up of every call
        t = {c: [] for c in list(calls) + list(loops)}
        for group, n in ((calls, a.reps), (loops, a.loop_reps)):
            for _ in range(n):
                for c, f in group.items():
                    t0 = time.perf_counter()
                    f()
                    t[c].append(1e3 * (time.perf_counter() - t0))
        pl, rg = first['plain loop'], first['regularised loop, uncertainty']
        calls_of = lambda r: dict(normal=len(r.history) - 1, chi2=len(r.history))
        out['cases']['P = %d' % P] = dict(
            nnode=list(nnode), penalty_rows=pen.nrow, median_ms={c: float(np.median(v)) for c, v in t.items()},
            min_ms={c: float(min(v)) for c, v in t.items()}, max_ms={c: float(max(v)) for c, v in t.items()},
            plain=dict(iterations=[int(pl.iterations.min()), int(pl.iterations.max())], calls=calls_of(pl),
                       converged=int((pl.status == fit.CONVERGED).sum()), node_error=float(np.max(np.abs(pl.nodes - truth)))),
            regularised=dict(iterations=[int(rg.iterations.min()), int(rg.iterations.max())], calls=calls_of(rg),
                             converged=int((rg.status == fit.CONVERGED).sum()), node_error=float(np.max(np.abs(rg.nodes - truth))),
                             largest_penalty=float(rg.penalty.max()), uncertainty_status_1=int(rg.uncertainty.status.sum()),
                             largest_sigma=[float(rg.uncertainty.parameter(q).max()) for q in fit.PARAMETERS]))
    eng.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
