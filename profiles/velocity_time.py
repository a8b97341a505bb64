#!/usr/bin/env python3
"""The normal equations of the field fit with four quantities (B, gammaB, chiB, vlos: lsx_hip_velocity_fit_normal) beside the same call
with three, and beside the three-quantity call of another build of the library (the parent commit's).

    python3 profiles/velocity_time.py [--columns N] [--reps N] [--angles 1|5] [--parent LIBRARY] [--out FILE]

The workload of profiles/fit_time.py at 1000 columns: FALC-perturbed CaII columns with ray-dependent profiles, after five MALI
iterations; the window of the 854.2 nm line; the line carries a normal triplet; the observation is the spectrum of 0.1 T, 45 degrees,
30 degrees and 1.5 km/s at every depth; two hat nodes per quantity over the depth index, off the truth.  After a warm-up of every call,
the calls are alternated `reps` times in this one process, in the order
    this build (2,2,2,2), this build (2,2,2), the parent's build (2,2,2)
host time of the whole call, which ends in a stream synchronise.  --parent: the other build's liblsx_hip.so, loaded beside this one
(its own engine on the same columns); without it that row is left out.  Under `rocprofv3 --kernel-trace --stats` the two instances of
k_response_nodes tell the node stage of the two calls apart (<true>: with the velocity, nine variants a depth; <false>: seven).
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

from lightspinner_amd import _capi, fit, fixtures, synth, zeeman, Engine  # noqa: E402

MUS = {1: np.array([1.0]), 5: np.array([0.2, 0.4, 0.6, 0.8, 1.0])}


class _Triplet:
    gLandeEff = 1.1


def converged_engine(prob, blk, prof, ncol, lib):
    eng = Engine(prob, ncol, lib=lib)
    synth.load_columns(eng, blk, prof)
    for it in range(5):
        eng.formal_sol_gamma()
        if it >= 3:
            eng.stat_equil()
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--columns', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--angles', type=int, default=5, choices=sorted(MUS))
    ap.add_argument('--parent', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    mus = MUS[a.angles]
    prob, base, raw = fixtures.load_problem_npz(os.path.join(ROOT, 'tests', 'golden', 'falc_ca.npz'), phi_compact=False)
    blk, prof = synth.perturbed_columns(prob, base, raw, ncol=a.columns)
    eng = converged_engine(prob, blk, prof, a.columns, _capi.load_hip_library())
    par = converged_engine(prob, blk, prof, a.columns, _capi.LsxLibrary(os.path.abspath(a.parent))) if a.parent else None
    lines = [t for t in prob.trans if t.is_line]
    k = [i for i, t in enumerate(lines) if abs(t.lambda0 - 854.44) < 0.1][0]
    la0, nla = lines[k].Nblue, lines[k].Nlambda
    pats = [None] * len(lines)
    pats[k] = zeeman.zeeman_components(_Triplet())
    Ns, nc = prob.Nspace, a.columns
    hats = fit.hat_basis(np.arange(Ns), [0.0, Ns - 1.0])
    basis3, nnode3 = fit.stack_basis(B=hats, gammaB=hats, chiB=hats)
    basis4, nnode4 = fit.stack_basis(B=hats, gammaB=hats, chiB=hats, vlos=hats)
    truth = np.tile([0.1, 0.1, np.deg2rad(45.0), np.deg2rad(45.0), np.deg2rad(30.0), np.deg2rad(30.0), 1.5e3, 1.5e3], (nc, 1))
    start = truth * np.array([1.1, 1.1, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]) + np.array([0, 0, 0.09, 0.09, -0.09, -0.09, -500.0, -500.0])
    vl = np.asarray(prof[2], dtype=np.float64)                                # the columns' own velocity
    # three quantities: the observation is the spectrum in the columns' own velocity, as in profiles/fit_time.py
    st = eng.stokes_rays(mus, 0.1, np.deg2rad(45.0), np.deg2rad(30.0), patterns=pats, la0=la0, nla=nla)
    obs3 = np.stack([st.I, st.Q, st.U, st.V], axis=1)
    st = eng.stokes_rays(mus, 0.1, np.deg2rad(45.0), np.deg2rad(30.0), patterns=pats, la0=la0, nla=nla, vlos=vl + 1.5e3)
    obs4 = np.stack([st.I, st.Q, st.U, st.V], axis=1)
    weight = lambda o: np.broadcast_to((1.0 / (1e-3 * o[:, 0].max(axis=(1, 2))) ** 2)[:, None, None, None], o.shape).copy()
    w3, w4 = weight(obs3), weight(obs4)
    base4 = np.zeros((nc, 4, Ns))
    base4[:, 3] = vl
    kw = dict(patterns=pats, la0=la0, nla=nla)
    calls = {'this (2,2,2,2)': lambda: eng.fit_field_normal(mus, basis4, nnode4, start, obs4, weight=w4, base=base4, **kw),
             'this (2,2,2)': lambda: eng.fit_field_normal(mus, basis3, nnode3, start[:, :6], obs3, weight=w3, **kw)}
    if par is not None:
        calls['parent (2,2,2)'] = lambda: par.fit_field_normal(mus, basis3, nnode3, start[:, :6], obs3, weight=w3, **kw)
    order = list(calls)
    first = {c: calls[c]() for c in order}                                   # the warm-up of every call
    same = lambda x, y: bool(np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64)))
    check = {}
    if par is not None:
        check['three_quantities_have_the_parents_bits'] = all(same(getattr(first['this (2,2,2)'], q), getattr(first['parent (2,2,2)'], q))
                                                              for q in ('chi2', 'grad', 'hess'))
    t = {c: [] for c in order}
    for _ in range(a.reps):
        for c in order:
            t0 = time.perf_counter()
            calls[c]()
            t[c].append(1e3 * (time.perf_counter() - t0))
    stat = lambda f: {c: float(f(t[c])) for c in order}
    out = dict(columns=nc, Nspace=Ns, window=[int(la0), int(nla)], angles=len(mus), reps=a.reps, library=eng.lib.path,
               median_ms=stat(np.median), min_ms=stat(min), max_ms=stat(max), checks=check)
    eng.close()
    if par is not None:
        par.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
