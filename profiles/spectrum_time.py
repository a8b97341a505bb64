#!/usr/bin/env python3
"""Emergent spectra at arbitrary wavelengths (lsx_hip_spectrum) against what it replaces and against the emergent-ray entry.

    python3 profiles/spectrum_time.py [c3|c4|both] [--reps N] [--parent-lib PATH] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -o spectrum --output-format csv -- python3 profiles/spectrum_time.py both --trace

C3's shape: 1000 FALC-perturbed CaII columns with ray-dependent profiles; C4's share: 1250 Ca + H columns; state after five MALI
iterations.  Per shape, after a warm-up of every call, alternated `reps` times in this one process, for nmu = 1 and 5:
  (a) own   Engine.emergent_spectrum with wavelength = the context's own grid, interpolation mode, against Engine.emergent_rays
            (of the library at --parent-lib where given: a second engine on it, loaded beside this one): the same work per
            (wavelength, depth, angle)
  (b) win   a 101-point window on the first line with the background handed over: the whole call
  (c) old   what a user did for (b): a second context on the union grid with zero-weight rays, every column uploaded again, n and J
            copied, one formal solution, I read back -- set-up included (once per shape; it is far off the others)
--trace: a few untimed calls of each path only, for a kernel trace.  One JSON line per shape."""
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

MUS5 = np.array([0.2, 0.4, 0.6, 0.8, 1.0])


def by_rule(lam, X, w):
    l = np.clip(np.searchsorted(lam, w, side='right') - 1, 0, lam.shape[0] - 2)
    t = np.clip((w - lam[l]) / (lam[l + 1] - lam[l]), 0.0, 1.0)
    return (1.0 - t)[:, None] * X[..., l, :] + t[:, None] * X[..., l + 1, :]


def alpha_at(prob, w):
    lam = prob.wavelength
    return np.stack([np.interp(w, lam[t.Nblue:t.Nblue + t.Nlambda], t.alpha, left=0.0, right=0.0) for t in prob.trans if not t.is_line])


def union_problem(prob, blk, J, w, alpha, bg):
    """the problem on the union grid (tests/spectrum_cases.py, regrid): what the old way needs"""
    lam = prob.wavelength
    wu = np.union1d(lam, w)
    rows, own = np.searchsorted(wu, w), np.searchsorted(wu, lam)
    trans, active, kc = [], np.zeros((len(prob.trans), wu.shape[0]), dtype=np.uint8), 0
    for kr, t in enumerate(prob.trans):
        sel = np.nonzero((wu >= lam[t.Nblue]) & (wu <= lam[t.Nblue + t.Nlambda - 1]))[0]
        t2 = dataclasses.replace(t, Nblue=int(sel[0]), Nlambda=int(sel.shape[0]))
        active[kr, sel] = 1
        if not t.is_line:
            a = np.zeros(wu.shape[0])
            a[rows] = alpha[kc]
            a[own[t.Nblue:t.Nblue + t.Nlambda]] = t.alpha
            t2.alpha = a[sel].copy()
            kc += 1
        trans.append(t2)

    def on_union(X, given):
        Y = by_rule(lam, X, wu)
        if given is not None:
            Y[..., rows, :] = given
        return Y
    b2 = dataclasses.replace(blk, phi=None, wphi=None, bg_chi=on_union(blk.bg_chi, bg[0]), bg_eta=on_union(blk.bg_eta, bg[1]))
    return dataclasses.replace(prob, wavelength=wu, trans=trans, active=active, phi_compact=False), b2, on_union(J, None), rows


def shape(workload, ncol, reps, trace, parent):
    fixture = os.path.join(ROOT, 'tests', 'golden', 'falc_cah.npz' if workload == 'c4' else 'falc_ca.npz')
    prob, base, raw = fixtures.load_problem_npz(fixture, phi_compact=False)
    blk, prof = synth.perturbed_columns(prob, base, raw, ncol=ncol)

    def converged(lib=None):
        e = Engine(prob, ncol, lib=lib)
        synth.load_columns(e, blk, prof)
        for it in range(5):
            e.formal_sol_gamma()
            if it >= 3:
                e.stat_equil()
        return e
    eng = converged()
    rays_eng = converged(_capi.LsxLibrary(parent)) if parent else eng
    lam = prob.wavelength
    a_own = np.zeros((prob.Ntrans - prob.Nlines, prob.Nspect))
    for kc, t in enumerate(t for t in prob.trans if not t.is_line):
        a_own[kc, t.Nblue:t.Nblue + t.Nlambda] = t.alpha
    line = next(t for t in prob.trans if t.is_line)
    w = line.lambda0 + np.linspace(-0.2, 0.2, 101)
    a_win = alpha_at(prob, w)
    bg = (by_rule(lam, blk.bg_chi, w), by_rule(lam, blk.bg_eta, w))
    calls = {
        'own': lambda mus: eng.emergent_spectrum(mus, lam, alpha=a_own),
        'rays': lambda mus: rays_eng.emergent_rays(mus),
        'win': lambda mus: eng.emergent_spectrum(mus, w, alpha=a_win, bg_chi=bg[0], bg_eta=bg[1]),
    }
    for f in calls.values():                     # warm-up of every shape the timed window uses
        f(MUS5)
        f(MUS5[-1:])
    agree = float(np.max(np.abs(calls['own'](MUS5) - calls['rays'](MUS5)) / np.abs(calls['rays'](MUS5))))
    if trace:
        for _ in range(3):
            for f in calls.values():
                f(MUS5)
                f(MUS5[-1:])
        return dict(workload=workload, columns=ncol, trace=True, own_against_rays_rel=agree)
    t = {(k, nmu): [] for k in calls for nmu in (1, 5)}
    for _ in range(reps):
        for nmu in (1, 5):
            for k, f in calls.items():
                t0 = time.perf_counter()
                f(MUS5[5 - nmu:])
                t[(k, nmu)].append(1e3 * (time.perf_counter() - t0))
    # (c) the old way, set-up included
    t0 = time.perf_counter()
    J = eng.get(_capi.LSX_J)
    p2, b2, J2, rows = union_problem(prob, blk, J, w, a_win, bg)
    p2 = dataclasses.replace(p2, muz=MUS5.copy(), wmu=np.zeros(5))
    old = Engine(p2, ncol)
    synth.load_columns(old, b2, prof)
    old.set(_capi.LSX_N, eng.get(_capi.LSX_N))
    old.set(_capi.LSX_J, J2)
    old.formal_sol_gamma()
    Iold = old.get(_capi.LSX_I)[:, rows]
    t_old = 1e3 * (time.perf_counter() - t0)
    win_old = float(np.max(np.abs(calls['win'](MUS5) - Iold) / np.abs(Iold)))
    med = lambda v: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
    out = dict(workload=workload, columns=ncol, Nspect=prob.Nspect, Nspace=prob.Nspace, reps=reps, window=int(w.shape[0]),
               parent_lib=bool(parent), host_ms={'%s_nmu%d' % k: med(v) for k, v in t.items()},
               old_way_5_angles_ms=t_old, own_against_rays_rel=agree, window_against_old_way_rel=win_old)
    eng.close(); old.close()
    if parent:
        rays_eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('workload', nargs='?', default='both', choices=['c3', 'c4', 'both'])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--columns', type=int, default=None)
    ap.add_argument('--parent-lib', default=None, help="the parent commit's liblsx_hip.so: its lsx_hip_emergent_rays is the yardstick of (a)")
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []
    for wl in (('c3', 'c4') if a.workload == 'both' else (a.workload,)):
        r = shape(wl, a.columns or (1000 if wl == 'c3' else 1250), a.reps, a.trace, a.parent_lib)
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
