#!/usr/bin/env python3
"""The FALC CaII temperature response function (165 columns): native set-up plus solve beside the fixture-driven path.

    python3 profiles/response_time.py [--reps R]

In one process, after one warm-up run each, interleaved (native, fixture, native, ...), `reps` repeats, the median printed:
  native_ms    response.native_response_function: every input of every column made on the device (Engine.setup_columns: depth scales,
               background, LTE populations, broadening, profiles, collisional rates), then the two batched solves
  fixture_ms   response.run_response_function: the perturbed columns' inputs taken from tests/golden/rf_ca_inputs.npz (loaded before
               the clock starts), the same two solves
  setup_ms     Engine.setup_columns of the 164 perturbed columns alone (engine creation not included)
No threshold.  One JSON line."""
import argparse
import json
import os
import sys
import time

os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from lightspinner_amd import Engine, atomdata, fixtures, native, response  # noqa: E402
from lightspinner_amd.background import EosTables  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    fx = np.load(os.path.join(GOLDEN, 'background_eos.npz'))
    tab = EosTables(fx['tpf'], fx['pf'], fx['eion'], fx['nstage'], fx['abund'], fx['amass'], float(fx['weight_per_H']))
    sf = dict(np.load(os.path.join(GOLDEN, 'setup_falc.npz')))
    sc = np.load(os.path.join(GOLDEN, 'scales_falc.npz'))
    prob, base, d = fixtures.load_problem_npz(os.path.join(GOLDEN, 'falc_ca.npz'))
    fixture = dict(np.load(os.path.join(GOLDEN, 'rf_ca_inputs.npz')))
    setup = native.NativeSetup(atomdata.from_fixture(sf, atoms=[1]), atomdata.from_fixture(sf, atoms=[0]).atoms[0], [float(sf['m1_abundance'])],
                               tab, float(sc['logG']))
    model = native.ColumnModel('column_mass', sc['falc_cm_depth_scale'], d['temperature'], d['ne'], d['nHTot'], d['vturb'])
    ks = list(range(prob.Nspace))

    def run_native():
        return response.native_response_function(prob, setup, model, 'temperature', float(fixture['tempPert']), ks=ks)

    def run_fixture():
        return response.run_response_function(prob, base, fixture, ks)

    batch = native.perturbed(model.validated(prob.Nspace), 'temperature', float(fixture['tempPert']), ks)
    eng = Engine(prob, batch.ncol, policy_columns=batch.ncol)

    def run_setup():
        eng.setup_columns(0, batch, setup)

    runs = {'native_ms': run_native, 'fixture_ms': run_fixture, 'setup_ms': run_setup}
    res = {k: f() for k, f in runs.items()}                       # warm-up
    t = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, f in runs.items():
            t0 = time.perf_counter()
            f()
            t[k].append((time.perf_counter() - t0) * 1e3)
    eng.close()
    out = {'columns': 1 + batch.ncol, 'reps': a.reps}
    out.update({k: float(np.median(v)) for k, v in t.items()})
    out['n_iter_equal'] = bool(np.array_equal(res['native_ms']['n_iter'], res['fixture_ms']['n_iter']))
    out['rf_max_abs_difference'] = float(np.max(np.abs(res['native_ms']['rf'] - res['fixture_ms']['rf'])))
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
