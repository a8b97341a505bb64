#!/usr/bin/env python3
"""Generate tests/golden/boundary_*.npz: the reference's own Gamma loop (rh_method.py:565-745, the unmodified
formal_sol_gamma_matrices, set up as tests/golden/make_topology_golden.py sets it up: reference_context) under radiation boundary
conditions the reference declares but never reads (atmosphere.py:18-20; include/lsx_hip_boundary.h).

The one thing replaced is the module attribute rh_method.piecewise_linear_1d, before the loop runs: solver() below forms the start
value of the ray from the table of the header (tests/boundary_cases.py, start_value) and hands it to the reference's own
formal_solver.piecewise_1d_impl -- the recurrence, Psi* = 0 at the first point, the end-point rule and the Gamma accumulation are the
reference's.  With the default kinds (thermalised below, zero above) solver() IS the reference's piecewise_linear_1d, bit for bit:
tests/test_boundary_host.py holds it to the topology fixture.

Cases, combinations, given intensities, protocol and what is kept: tests/boundary_cases.py.  Numbers only; fixed member time stamps
and the file budget of the topology fixture.

Usage:  python tests/golden/make_boundary_golden.py
"""
import os
import sys
import time
import warnings
import zipfile
import zlib

import make_topology_golden as mt            # puts the reference, its stubs, the repository and tests/ on the path

import numpy as np  # noqa: E402

import formal_solver  # noqa: E402
import rh_method  # noqa: E402
import utils  # noqa: E402

import boundary_cases as bc  # noqa: E402
import topology_cases as tc  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


class Solver:
    """what stands in for rh_method.piecewise_linear_1d: the kinds of both ends, the given intensities [Nspect][Nrays]"""

    def __init__(self, lower, upper, I_lower, I_upper, wavelength):
        self.kind = {True: lower, False: upper}
        self.given = {True: I_lower, False: I_upper}
        self.wavelength = np.asarray(wavelength)

    def __call__(self, atmos, mu, toFrom, wav, chi, S):
        toFrom = bool(toFrom)
        given = None
        if self.kind[toFrom] == bc.GIVEN:
            la = int(np.searchsorted(self.wavelength, wav))
            assert self.wavelength[la] == wav
            given = self.given[toFrom][la, mu]
        Iupw = bc.start_value(self.kind[toFrom], toFrom, given, atmos.muz[mu], atmos.height, atmos.temperature, wav, chi,
                              planck_fn=utils.planck)
        I, PsiStar = formal_solver.piecewise_1d_impl(atmos.muz[mu], toFrom, Iupw, atmos.height, chi, S)
        return formal_solver.IPsi(I, PsiStar)


def run_column(prob, block, col, combo):
    """the protocol of tests/boundary_cases.py on one column under one combination -> {key: array}"""
    lo, up = bc.kinds(combo)
    I_lower, I_upper = bc.given_arrays(prob, block, col)
    ctx = mt.reference_context(prob, block, col)
    trans = sorted((ct for atom in ctx.activeAtoms for ct in atom.trans), key=lambda ct: ct.kr)
    d = {}
    saved = rh_method.piecewise_linear_1d
    rh_method.piecewise_linear_1d = Solver(lo, up, I_lower, I_upper, prob.wavelength)
    try:
        with warnings.catch_warnings(), np.errstate(all='ignore'):
            warnings.simplefilter('ignore')
            for it in (1, 2):
                if it == 2:
                    for ct in trans:
                        ct.Rij.fill(0.0)
                        ct.Rji.fill(0.0)
                dJ = ctx.formal_sol_gamma_matrices()
                tag = 'fs%d_' % it
                d[tag + 'I'] = ctx.I.copy()
                d[tag + 'dJ'] = np.float64(dJ)
                d[tag + 'Gamma'] = np.concatenate([atom.Gamma.reshape(atom.Nlevel ** 2, prob.Nspace) for atom in ctx.activeAtoms])
                if it == 1:
                    d[tag + 'J'] = ctx.J.copy()
                else:
                    d[tag + 'Rij'] = np.stack([ct.Rij for ct in trans]) if trans else np.zeros((0, prob.Nspace))
                    d[tag + 'Rji'] = np.stack([ct.Rji for ct in trans]) if trans else np.zeros((0, prob.Nspace))
    finally:
        rh_method.piecewise_linear_1d = saved
    return d


def run_case(name):
    t0 = time.time()
    prob, block = tc.build(name)
    out = {}
    for col in tc.golden_columns(name, block.ncol):
        out['%s/c%d/digest' % (name, col)] = tc.input_digest(prob, block, col)
        for combo in bc.COMBOS:
            for k, v in run_column(prob, block, col, combo).items():
                out['%s/%s/c%d/%s' % (name, combo, col, k)] = v
        # the default kinds through the same solver: not stored, only the SHA-256 of each array -- tests/test_boundary_host.py finds
        # the same bits in the topology fixture, which the reference's own piecewise_linear_1d wrote
        for k, v in run_column(prob, block, col, bc.DEFAULT).items():
            if k in bc.DEFAULT_KEYS:
                out['%s/%s/c%d/sha_%s' % (name, bc.DEFAULT, col, k)] = bc.sha(v)
    print('%-55s %5.1f s' % (name, time.time() - t0), flush=True)
    return out


def write(d):
    for f in os.listdir(HERE):
        if f.startswith('boundary_') and f.endswith('.npz'):
            os.remove(os.path.join(HERE, f))
    files, used = [[]], 0
    for key, arr in d.items():
        raw = mt._member(arr)
        size = len(zlib.compress(raw, 6)) + len(key) * 2 + 120
        if files[-1] and used + size > mt.FILE_BUDGET:
            files.append([])
            used = 0
        files[-1].append((key, raw))
        used += size
    for k, members in enumerate(files):
        path = os.path.join(HERE, 'boundary_%02d.npz' % k)
        with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED, compresslevel=6) as z:
            for key, raw in members:
                zi = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
                zi.compress_type = zipfile.ZIP_DEFLATED
                zi.external_attr = 0o644 << 16
                z.writestr(zi, raw, compresslevel=6)
        print('wrote %s (%.1f kB)' % (path, os.path.getsize(path) / 1e3), flush=True)


if __name__ == '__main__':
    import multiprocessing as mp
    t0 = time.time()
    nproc = max(1, min(8, len(os.sched_getaffinity(0)), len(bc.CASES)))
    with mp.get_context('fork').Pool(nproc) as pool:
        results = pool.map(run_case, bc.CASES, chunksize=1)
    d = {}
    for r in results:
        d.update(r)
    write(d)
    print('done in %.1f s' % (time.time() - t0), flush=True)
