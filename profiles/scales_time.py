#!/usr/bin/env python3
"""Depth-scale conversion on the device (lsx_hip_convert_scales): how long it takes, beside the background at one wavelength.

    python3 profiles/scales_time.py [--columns 1,165,1000] [--reps R]

For each column count N, FALC-perturbed columns on FALC's column-mass scale, after one warm-up call each and `reps` repeats (the
median is printed), in one process:
  scales_cm / scales_tau / scales_geo   Engine.convert_scales(install=True, read_back=False): equation of state, opacity at 500 nm,
                                        integration, heights copied into the context -- nothing comes back over PCIe
  background_1   Engine.background at ONE wavelength (500 nm) for the same columns, arrays read back: the same equation of state and
                 opacity without the integration
  eos            Engine.eos alone
No threshold.  One JSON line per column count."""
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
from lightspinner_amd.background import EosTables  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def median_ms(f, reps):
    f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--columns', default='1,165,1000')
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    fx = np.load(os.path.join(GOLDEN, 'background_eos.npz'))
    tab = EosTables(fx['tpf'], fx['pf'], fx['eion'], fx['nstage'], fx['abund'], fx['amass'], float(fx['weight_per_H']))
    cm = np.load(os.path.join(GOLDEN, 'scales_falc.npz'))['falc_cm_depth_scale']
    prob, block, d = fixtures.load_problem_npz(os.path.join(GOLDEN, 'falc_ca.npz'))
    for n in (int(x) for x in a.columns.split(',')):
        batch, _ = synth.perturbed_columns(prob, block, d, ncol=n, seed=1234, vlos_sigma=0.0)
        T = np.ascontiguousarray(batch.temperature)
        nH, ne, ds = np.tile(d['nHTot'], (n, 1)), np.tile(d['ne'], (n, 1)), np.tile(cm, (n, 1))
        eng = Engine(prob, n)
        eng.set_columns(0, batch)
        r = eng.convert_scales(tab, 'column_mass', ds, T, nH)
        out = {'columns': n, 'Nspace': prob.Nspace}
        out['scales_cm_ms'] = median_ms(lambda: eng.convert_scales(tab, 'column_mass', ds, T, nH, install=True, read_back=False), a.reps)
        out['scales_tau_ms'] = median_ms(lambda: eng.convert_scales(tab, 'tau500', r.tau_ref, T, nH, install=True, read_back=False), a.reps)
        out['scales_geo_ms'] = median_ms(lambda: eng.convert_scales(tab, 'geometric', r.height, T, nH, ne, install=True, read_back=False), a.reps)
        out['background_1_ms'] = median_ms(lambda: eng.background(tab, T, nH, ne, wavelength=[500.0]), a.reps)
        out['eos_ms'] = median_ms(lambda: eng.eos(tab, T, nH), a.reps)
        eng.close()
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
