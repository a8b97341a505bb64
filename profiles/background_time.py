#!/usr/bin/env python3
"""The background on the device (lsx_hip_background, lsx_hip_eos): how long it takes, against what it replaces.

    python3 profiles/background_time.py [--columns N] [--reps R]

Times, after one warm-up call each and `reps` repeats (the median is printed):
  eos        Engine.eos on N FALC-perturbed columns
  install    Engine.background(install=True, read_back=False) on the CaII grid (287 wavelengths) for N columns: equation of state,
             opacity, pack into the context -- nothing comes back over PCIe
  upload     Engine.set_columns with host arrays for the same N columns: what an install saves (it also uploads everything else)
  one        Engine.background for ONE column on the CaII / Ca + H / five-atom grids, arrays read back: what the reference's
             Background(atmos, spect) does in 6.1 s on the CaII grid
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

from lightspinner_amd import fixtures, synth, Engine  # noqa: E402
from lightspinner_amd.background import EosTables, _carrier_problem  # noqa: E402

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
    ap.add_argument('--columns', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    fx = np.load(os.path.join(GOLDEN, 'background_eos.npz'))
    tab = EosTables(fx['tpf'], fx['pf'], fx['eion'], fx['nstage'], fx['abund'], fx['amass'], float(fx['weight_per_H']))
    prob, block, d = fixtures.load_problem_npz(os.path.join(GOLDEN, 'falc_ca.npz'))
    n = a.columns
    batch, _ = synth.perturbed_columns(prob, block, d, ncol=n, seed=1234, vlos_sigma=0.0)
    T = np.ascontiguousarray(batch.temperature)
    nH, ne = np.tile(d['nHTot'], (n, 1)), np.tile(d['ne'], (n, 1))
    eng = Engine(prob, n)
    eng.set_columns(0, batch)
    out = {'columns': n, 'Nspect': prob.Nspect}
    out['eos_ms'] = median_ms(lambda: eng.eos(tab, T, nH), a.reps)
    out['install_ms'] = median_ms(lambda: eng.background(tab, T, nH, ne, install=True, read_back=False), a.reps)
    out['upload_ms'] = median_ms(lambda: eng.set_columns(0, batch), a.reps)
    eng.close()
    one = _carrier_problem(82)
    e1 = Engine(one, 1)
    for name in ('falc_ca', 'falc_cah', 'falc_all'):
        g = np.load(os.path.join(GOLDEN, name + '.npz'))
        out['one_%s_ms' % name] = median_ms(lambda: e1.background(tab, g['temperature'], g['nHTot'], g['ne'], wavelength=g['wavelength']), a.reps)
        out['one_%s_nla' % name] = int(g['wavelength'].shape[0])
    e1.close()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
