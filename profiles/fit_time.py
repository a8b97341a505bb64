#!/usr/bin/env python3
"""The normal equations of the field fit on the device (lsx_hip_fit_field_normal) beside what had to be done without them: the
response copied to the host, contracted and summed in numpy.

    python3 profiles/fit_time.py [--columns N] [--reps N] [--out FILE]

The workload of profiles/stokes_response_time.py: FALC-perturbed CaII columns with ray-dependent profiles, after five MALI
iterations; the window of the 854.2 nm line; the line carries a normal triplet; the observation is the spectrum of 0.1 T, 45 degrees,
30 degrees at every depth; two hat nodes per parameter over the depth index, off the truth.  After a warm-up the two are alternated
`reps` times in this one process, each at mu = 1 and at five angles:
  device   host time of the whole Engine.fit_field_normal call (uploads, the Stokes pass, the response's two stages, the contraction
           and the sums, P x P numbers a column back)
  numpy    Engine.stokes_response of the expanded field (rf and stokes to the host), then J = rf . basis, grad = J^T W r, hess = J^T W J
           with einsum in float64; its two parts are timed apart (response_ms, numpy_ms)
Then one whole drivers.fit_field_columns run at five angles: its wall time, the part spent inside the library's three entries, and a
CPU profile of the rest (the loop's own Python), the ten heaviest functions by own time.
One JSON line."""
import argparse
import cProfile
import io
import json
import os
import pstats
import sys
import time

os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from lightspinner_amd import drivers, fit, fixtures, synth, zeeman, Engine  # noqa: E402

MUS5 = np.array([0.2, 0.4, 0.6, 0.8, 1.0])
NAMES = ('B', 'gammaB', 'chiB')


class _Triplet:
    gLandeEff = 1.1


def numpy_normal(eng, mu, field, basis, nnode, obs, w, pats, la0, nla):
    t0 = time.perf_counter()
    r = eng.stokes_response(mu, field[:, 0], field[:, 1], field[:, 2], patterns=pats, la0=la0, nla=nla)
    t1 = time.perf_counter()
    S = np.stack([r.stokes.I, r.stokes.Q, r.stokes.U, r.stokes.V], axis=1)
    o = np.cumsum([0] + list(nnode))
    J = np.concatenate([np.einsum('cslkm,nk->cnslm', r.rf[p], basis[o[i]:o[i + 1]]) for i, p in enumerate(NAMES)], axis=1)
    J = J.reshape(J.shape[0], J.shape[1], -1)
    res = (obs - S).reshape(S.shape[0], -1)
    ww = w.reshape(S.shape[0], -1)
    out = np.sum(ww * res * res, axis=1), np.einsum('cnd,cd->cn', J, ww * res), np.einsum('cad,cbd,cd->cab', J, J, ww)
    return out, 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--columns', type=int, default=100)
    ap.add_argument('--reps', type=int, default=10)
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
    Ns, nc = prob.Nspace, a.columns
    hats = fit.hat_basis(np.arange(Ns), [0.0, Ns - 1.0])
    basis, nnode = fit.stack_basis(B=hats, gammaB=hats, chiB=hats)
    truth = np.tile([0.1, 0.1, np.deg2rad(45.0), np.deg2rad(45.0), np.deg2rad(30.0), np.deg2rad(30.0)], (nc, 1))
    start = truth * np.array([1.1, 1.1, 1.0, 1.0, 1.0, 1.0]) + np.array([0, 0, 0.09, 0.09, -0.09, -0.09])
    data = {}
    for m in (1, 5):
        st = eng.stokes_rays(MUS5[5 - m:], 0.1, np.deg2rad(45.0), np.deg2rad(30.0), patterns=pats, la0=la0, nla=nla)
        obs = np.stack([st.I, st.Q, st.U, st.V], axis=1)
        w = np.broadcast_to((1.0 / (1e-3 * obs[:, 0].max(axis=(1, 2))) ** 2)[:, None, None, None], obs.shape).copy()
        data[m] = (obs, w)
    kw = dict(patterns=pats, la0=la0, nla=nla)
    dev = lambda m: eng.fit_field_normal(MUS5[5 - m:], basis, nnode, start, data[m][0], weight=data[m][1], **kw)
    ref = lambda m, f: numpy_normal(eng, MUS5[5 - m:], f, basis, nnode, data[m][0], data[m][1], pats, la0, nla)
    agree = {}
    for m in (1, 5):
        ne = dev(m)
        (c, g, H), _, _ = ref(m, ne.field)
        agree[str(m)] = float(max(np.max(np.abs(ne.chi2 / c - 1)), np.max(np.abs(ne.hess - H)) / np.max(np.abs(H)),
                                  np.max(np.abs(ne.grad - g)) / np.max(np.abs(g))))
        field = ne.field
    t = {(n, m): [] for n in ('device', 'numpy', 'response', 'contraction') for m in (1, 5)}
    for _ in range(a.reps):
        for m in (1, 5):
            t0 = time.perf_counter()
            dev(m)
            t[('device', m)].append(1e3 * (time.perf_counter() - t0))
            t0 = time.perf_counter()
            _, tr, tn = ref(m, field)
            t[('numpy', m)].append(1e3 * (time.perf_counter() - t0))
            t[('response', m)].append(tr)
            t[('contraction', m)].append(tn)
    stat = lambda f: {n: {str(m): float(f(t[(n, m)])) for m in (1, 5)} for n in ('device', 'numpy', 'response', 'contraction')}
    med = stat(np.median)
    # one whole fit at five angles: wall time, the time inside the library's entries, the loop's own Python under a CPU profile
    inside = [0.0]
    dll = eng.lib.dll
    timed = {}
    for name in ('lsx_hip_fit_field_normal', 'lsx_hip_fit_field_chi2', 'lsx_hip_fit_field_step'):
        f = getattr(dll, name)

        def wrap(*args, _f=f):
            t0 = time.perf_counter()
            rc = _f(*args)
            inside[0] += time.perf_counter() - t0
            return rc
        timed[name] = f
        setattr(dll, name, wrap)
    prof_ = cProfile.Profile()
    t0 = time.perf_counter()
    prof_.enable()
    r = drivers.fit_field_columns(eng, data[5][0], MUS5, basis, start, nnode, weight=data[5][1], **kw)
    prof_.disable()
    wall = time.perf_counter() - t0
    for name, f in timed.items():
        setattr(dll, name, f)
    stats = pstats.Stats(prof_, stream=io.StringIO()).stats            # (file, line, function) -> (calls, primitive calls, own, cumulative, callers)
    heavy = sorted(stats.items(), key=lambda kv: -kv[1][2])[:10]
    out = dict(columns=nc, Nspace=Ns, window=[int(la0), int(nla)], reps=a.reps, nnode=list(nnode), median_ms=med, min_ms=stat(min),
               max_ms=stat(max), numpy_over_device={str(m): med['numpy'][str(m)] / med['device'][str(m)] for m in (1, 5)},
               largest_relative_difference=agree,
               fit=dict(wall_ms=1e3 * wall, inside_library_ms=1e3 * inside[0], iterations=[int(r.iterations.min()), int(r.iterations.max())],
                        status=sorted(set(int(v) for v in r.status)), chi2_first=float(r.history[0].max()), chi2_last=float(r.chi2.max()),
                        largest_node_error=float(np.max(np.abs(r.nodes - truth))),
                        heaviest_python=[dict(own_ms=1e3 * v[2], calls=int(v[1]), where='%s:%d(%s)' % (os.path.basename(k[0]), k[1], k[2])) for k, v in heavy]))
    eng.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
