#!/usr/bin/env python3
"""The depth-resolved final pass (lsx_hip_depth_rays) against the emergent-ray pass (lsx_hip_emergent_rays) for the same angles:
the new pass does a superset of that one's work, so the ratio is the meaningful figure.

    python3 profiles/depth_time.py [c3|c4|both] [--reps N] [--rays-library PATH] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -o depth --output-format csv -- python3 profiles/depth_time.py both --trace

C3's shape: 1000 FALC-perturbed CaII columns with ray-dependent profiles; C4's share: 1250 Ca + H columns; state after five MALI
iterations.  Windows: CaII K's own wavelengths (every output asked for) and the full grid (z_tau1 asked for, a map of the formation
height: the five depth-resolved arrays of a full-grid call are gigabytes on the host); nmu = 1 and 5.  Per shape, after a warm-up of every call, the calls are
alternated `reps` times in this one process: host time of the whole Engine.depth_rays call (kernels, the copies of the results, one
wait per pass) and of Engine.emergent_rays for the same angles -- of this library, or of the build --rays-library names (the parent
commit's).  --trace: a few untimed calls of each only, for a kernel trace.  Bytes are computed from the shapes: what the pass must
read once, write once and read back once, against the 6.29 TB/s the project uses as achievable bandwidth.  One JSON line per shape."""
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
MUS5 = np.array([0.2, 0.4, 0.6, 0.8, 1.0])
CA_K = 393.366          # nm


def needed_bytes_per_column(prob, nmu, nla):
    """the streams of the window (background opacity and emissivity, J, the continua's Boltzmann factor) and the small per-depth
    arrays once; chi, S, tau, contrib, I written once, chi and S read back once; z_tau1"""
    Ns = prob.Nspace
    ncont = sum(1 for t in prob.trans if not t.is_line)
    streams = (4 if ncont else 3) * nla * Ns
    small = (prob.NLtot + ncont + 3) * Ns + (prob.Nlines + prob.Natoms + 1) * Ns
    return 8 * (streams + small + (7 * Ns + 1) * nmu * nla)


def shape(workload, ncol, reps, trace, rays_library):
    fixture = os.path.join(ROOT, 'tests', 'golden', 'falc_cah.npz' if workload == 'c4' else 'falc_ca.npz')
    prob, base, raw = fixtures.load_problem_npz(fixture, phi_compact=False)
    blk, prof = synth.perturbed_columns(prob, base, raw, ncol=ncol)
    eng = Engine(prob, ncol)
    synth.load_columns(eng, blk, prof)
    for it in range(5):
        eng.formal_sol_gamma()
        if it >= 3:
            eng.stat_equil()
    rays = eng
    if rays_library:
        rays = Engine(prob, ncol, lib=_capi.LsxLibrary(rays_library))
        synth.load_columns(rays, blk, prof)
        rays.set(_capi.LSX_N, eng.get(_capi.LSX_N))
        rays.set(_capi.LSX_J, eng.get(_capi.LSX_J))
    k_line = min((t for t in prob.trans if t.is_line), key=lambda t: abs(t.lambda0 - CA_K))
    windows = {'CaII K': (k_line.Nblue, k_line.Nlambda, _capi_all()), 'full grid': (0, prob.Nspect, ('z_tau1',))}
    calls = [(w, nmu) for w in windows for nmu in (1, 5)]

    def depth(w, nmu):
        la0, nla, what = windows[w]
        return eng.depth_rays(MUS5[5 - nmu:], la0=la0, nla=nla, what=what)
    for w, nmu in calls:                       # warm-up of every shape the timed window uses
        d = depth(w, nmu)
    top = rays.emergent_rays(MUS5)
    rays.emergent_rays(MUS5[-1:])
    la0, nla, _ = windows['CaII K']
    dk = depth('CaII K', 5)
    agree = float(np.max(np.abs(np.moveaxis(dk.I[:, :, 0, :], 1, 2) - top[:, la0:la0 + nla]) / np.abs(top[:, la0:la0 + nla])))
    if trace:
        for _ in range(3):
            for w, nmu in calls:
                depth(w, nmu)
            rays.emergent_rays(MUS5)
            rays.emergent_rays(MUS5[-1:])
        return dict(workload=workload, columns=ncol, trace=True, I_top_against_emergent_rays_rel=agree)
    t_new = {c: [] for c in calls}
    t_rays = {1: [], 5: []}
    for _ in range(reps):
        for c in calls:
            t0 = time.perf_counter()
            depth(*c)
            t_new[c].append(1e3 * (time.perf_counter() - t0))
        for nmu in (1, 5):
            t0 = time.perf_counter()
            rays.emergent_rays(MUS5[5 - nmu:])
            t_rays[nmu].append(1e3 * (time.perf_counter() - t0))
    stat = lambda v: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
    out = dict(workload=workload, columns=ncol, Nspect=prob.Nspect, Nspace=prob.Nspace, reps=reps,
               rays_library=rays_library or 'this build', achievable_Bps=ACHIEVABLE_BPS, I_top_against_emergent_rays_rel=agree,
               windows={w: dict(la0=int(v[0]), nla=int(v[1]), outputs=list(v[2])) for w, v in windows.items()},
               depth_call_host_ms={'%s, nmu %d' % c: stat(v) for c, v in t_new.items()},
               emergent_rays_call_host_ms={str(k): stat(v) for k, v in t_rays.items()},
               needed_bytes_per_column={'%s, nmu %d' % (w, nmu): needed_bytes_per_column(prob, nmu, windows[w][1]) for w, nmu in calls},
               work_bytes_per_column={'%s, nmu %d' % (w, nmu): 8 * (5 * prob.Nspace + 1) * nmu * windows[w][1] for w, nmu in calls})
    out['time_at_achievable_bandwidth_ms'] = {k: 1e3 * ncol * v / ACHIEVABLE_BPS for k, v in out['needed_bytes_per_column'].items()}
    eng.close()
    if rays is not eng:
        rays.close()
    return out


def _capi_all():
    from lightspinner_amd.problem import DepthRays
    return DepthRays.FIELDS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('workload', nargs='?', default='both', choices=['c3', 'c4', 'both'])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--columns', type=int, default=None)
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--rays-library', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []
    for wl in (('c3', 'c4') if a.workload == 'both' else (a.workload,)):
        r = shape(wl, a.columns or (1000 if wl == 'c3' else 1250), a.reps, a.trace, a.rays_library)
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
