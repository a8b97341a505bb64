#!/usr/bin/env python3
"""The size of the fixed-population approximation of a velocity handed over per call (include/lsx_hip_stokes_velocity.h):
on FALC Ca II 854.2 nm, Context.compute_stokes(vlos=v) on the context converged at rest against Context.compute_stokes on a context
converged with atmos.vlos = v, for uniform v.

    python3 profiles/velocity_approx.py [--v 500 2000 5000] [--out FILE]

0.1 T at 45 and 30 degrees, a normal triplet of g = 1.1 on the line, mu = 1 and 0.6.  Converged: drivers.iterate_mali to dJ < 1e-6,
dPops < 1e-6.  Reported per v: the largest |dI| / I_c (I_c: the largest I of the window) and the largest |dV| / max |V|.
One JSON line."""
import argparse
import json
import os
import sys

os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np  # noqa: E402

from helpers import build_fakes  # noqa: E402
from lightspinner_amd import drivers  # noqa: E402
from lightspinner_amd.rh_method import Context  # noqa: E402

MUS = [1.0, 0.6]


def converged(d, v):
    atmos, spect, eq, bg = build_fakes(d)
    atmos.vlos = np.full(np.asarray(atmos.vlos).shape, float(v))
    ctx = Context(atmos, spect, eq, bg)
    h = drivers.iterate_mali(ctx, dJ_tol=1e-6, dPops_tol=1e-6, max_iter=2000)
    trans = [t for a in ctx.activeAtoms for t in a.trans]
    t = [t for t in trans if t.isLine and abs(t.lambda0 - 854.44) < 0.1][0]
    t.transModel.gLandeEff = 1.1
    return ctx, t, len(h.dJ)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--v', type=float, nargs='+', default=[500.0, 2000.0, 5000.0])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    d = dict(np.load(os.path.join(ROOT, 'tests', 'golden', 'falc_ca.npz')))
    rest, line, n0 = converged(d, 0.0)
    B, g, x = 0.1, np.deg2rad(45.0), np.deg2rad(30.0)
    rows = []
    for v in a.v:
        fixed = rest.compute_stokes(MUS, B, g, x, transition=line, vlos=v)
        ctx, t, n = converged(d, v)
        moved = ctx.compute_stokes(MUS, B, g, x, transition=t)
        ctx.close()
        rows.append(dict(v=v, iterations=n, dI_over_Ic=float(np.max(np.abs(fixed.I - moved.I)) / np.max(moved.I)),
                         dV_over_maxV=float(np.max(np.abs(fixed.V - moved.V)) / np.max(np.abs(moved.V))),
                         dQ_over_maxQ=float(np.max(np.abs(fixed.Q - moved.Q)) / np.max(np.abs(moved.Q)))))
    rest.close()
    line_ = json.dumps(dict(line='Ca II 854.2 nm', mus=MUS, iterations_at_rest=n0, rows=rows))
    print(line_, flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line_ + '\n')


if __name__ == '__main__':
    main()
