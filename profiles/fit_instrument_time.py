#!/usr/bin/env python3
"""The field fit through an instrument (lsx_hip_instrument_fit_normal, lsx_hip_instrument_fit_chi2; k_fit_smear) beside the fit
without one, and beside the same two calls of another build of the library (the parent commit's).

    python3 profiles/fit_instrument_time.py [--columns N] [--reps N] [--parent LIBRARY] [--no-instrument] [--out FILE]

The workload of profiles/fit_time.py at 1000 columns: FALC-perturbed CaII columns with ray-dependent profiles, after five MALI
iterations; the window of the 854.2 nm line; the line carries a normal triplet; five angles; the observation is the spectrum of
0.1 T, 45 degrees, 30 degrees at every depth; two hat nodes per parameter over the depth index, off the truth.  The instrument is the
analogue of the recovery tests' (a) on this window: 2 nla / 3 pixels uniform over the window behind a Gaussian of fwhm 2 x the
window's median spacing.  After a warm-up of every call, the calls are alternated `reps` times in this one process, in the order
    this build with the instrument, this build without, the parent's build without
for fit_field_normal and fit_field_chi2 each: host time of the whole call, which ends in a stream synchronise.  --parent: the other
build's liblsx_hip.so, loaded beside this one (its own engine on the same columns); without it those two rows are left out.
--no-instrument leaves the instrument's rows out: two builds alone, in either order (LSX_HIP_LIBRARY names the first), which is the
control for what the order of the engines and of the calls does to the figures.
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

MUS5 = np.array([0.2, 0.4, 0.6, 0.8, 1.0])


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
    ap.add_argument('--parent', default=None)
    ap.add_argument('--no-instrument', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    prob, base, raw = fixtures.load_problem_npz(os.path.join(ROOT, 'tests', 'golden', 'falc_ca.npz'), phi_compact=False)
    blk, prof = synth.perturbed_columns(prob, base, raw, ncol=a.columns)
    engines = {'this': converged_engine(prob, blk, prof, a.columns, _capi.load_hip_library())}
    if a.parent:
        engines['parent'] = converged_engine(prob, blk, prof, a.columns, _capi.LsxLibrary(os.path.abspath(a.parent)))
    eng = engines['this']
    lines = [t for t in prob.trans if t.is_line]
    k = [i for i, t in enumerate(lines) if abs(t.lambda0 - 854.44) < 0.1][0]
    la0, nla = lines[k].Nblue, lines[k].Nlambda
    pats = [None] * len(lines)
    pats[k] = zeeman.zeeman_components(_Triplet())
    Ns, nc = prob.Nspace, a.columns
    hats = fit.hat_basis(np.arange(Ns), [0.0, Ns - 1.0])
    basis, nnode = fit.stack_basis(B=hats, gammaB=hats, chiB=hats)
    truth = np.tile([0.1, 0.1, np.deg2rad(45.0), np.deg2rad(45.0), np.deg2rad(30.0), np.deg2rad(30.0)], (nc, 1))
    start = truth * np.array([1.1, 1.1, 1.0, 1.0, 1.0, 1.0]) + np.array([0, 0, 0.09, 0.09, -0.09, -0.09])
    grid = np.asarray(prob.wavelength, dtype=np.float64)[la0:la0 + nla]
    inst = fit.Instrument.gaussian(grid, np.linspace(grid[0], grid[-1], 2 * nla // 3), 2.0 * float(np.median(np.diff(grid))))
    st = eng.stokes_rays(MUS5, 0.1, np.deg2rad(45.0), np.deg2rad(30.0), patterns=pats, la0=la0, nla=nla)
    obs = np.stack([st.I, st.Q, st.U, st.V], axis=1)
    seen = obs if a.no_instrument else eng.apply_instrument(obs, inst)
    weight = lambda o: np.broadcast_to((1.0 / (1e-3 * o[:, 0].max(axis=(1, 2))) ** 2)[:, None, None, None], o.shape).copy()
    w, ws = weight(obs), weight(seen)
    kw = dict(patterns=pats, la0=la0, nla=nla)
    calls = {('normal', 'this, instrument'): lambda: eng.fit_field_normal(MUS5, basis, nnode, start, seen, weight=ws, instrument=inst, **kw),
             ('normal', 'this'): lambda: eng.fit_field_normal(MUS5, basis, nnode, start, obs, weight=w, **kw),
             ('chi2', 'this, instrument'): lambda: eng.fit_field_chi2(MUS5, basis, nnode, start, seen, weight=ws, instrument=inst, **kw),
             ('chi2', 'this'): lambda: eng.fit_field_chi2(MUS5, basis, nnode, start, obs, weight=w, **kw)}
    if a.parent:
        par = engines['parent']
        calls[('normal', 'parent')] = lambda: par.fit_field_normal(MUS5, basis, nnode, start, obs, weight=w, **kw)
        calls[('chi2', 'parent')] = lambda: par.fit_field_chi2(MUS5, basis, nnode, start, obs, weight=w, **kw)
    if a.no_instrument:
        calls = {c: f for c, f in calls.items() if 'instrument' not in c[1]}
    order = sorted(calls, key=lambda c: (c[0] != 'normal', ['this, instrument', 'this', 'parent'].index(c[1])))
    first = {c: calls[c]() for c in order}                                   # the warm-up of every call
    same = lambda x, y: bool(np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64)))
    lead = 'this' if a.no_instrument else 'this, instrument'
    check = dict(chi2_entry_is_the_normal_entrys=same(first[('chi2', lead)][0], first[('normal', lead)].chi2))
    if a.parent:
        check['without_an_instrument_the_bits_are_the_parents'] = all(
            same(getattr(first[('normal', 'this')], q), getattr(first[('normal', 'parent')], q)) for q in ('chi2', 'grad', 'hess')) \
            and same(first[('chi2', 'this')][0], first[('chi2', 'parent')][0])
    t = {c: [] for c in order}
    for _ in range(a.reps):
        for c in order:
            t0 = time.perf_counter()
            calls[c]()
            t[c].append(1e3 * (time.perf_counter() - t0))
    stat = lambda f: {'%s: %s' % c: float(f(t[c])) for c in order}
    out = dict(columns=nc, Nspace=Ns, window=[int(la0), int(nla)], angles=len(MUS5), reps=a.reps, nnode=list(nnode),
               instrument=None if a.no_instrument else dict(nobs=inst.nobs, width=inst.width), library=eng.lib.path, median_ms=stat(np.median), min_ms=stat(min), max_ms=stat(max), checks=check)
    for e in engines.values():
        e.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
