"""Shared cases of the emergent-spectra tests (tests/test_emergent_rays_host.py, tests/test_emergent_rays.py).

The checker needs nothing new in the oracle: a context whose `muz` is the wanted angles and whose `wmu` is zero IS the
reference's computation (atmosphere.py:386-393 builds exactly that; rh_method.py:638 then leaves the emergent intensity of every
ray in ctx.I).  `oracle_rays` builds it on the oracle library, sets the populations and J, runs one formal solution and reads
LSX_I; dJ is inf and Gamma is garbage with zero weights, neither is looked at."""
import dataclasses
import functools

import numpy as np

from conftest import golden
from lightspinner_amd import _capi, fixtures, synth
from lightspinner_amd.problem import Engine

MUS20 = np.linspace(0.1, 1.0, 20)            # all tolerance tests use mu >= 0.1 (tests/golden/make_rays_golden.py)
# reference-against-oracle bars of the golden cases: tests/test_oracle_golden.py's bar for the oracle against golden arrays (CaII),
# the suite's bar for the emergent intensity of the Ca + H problem
GOLDEN_BAR = {'ca': 1e-11, 'ca_vlos': 1e-11, 'cah': 3e-11}
GOLDEN_CASES = tuple(GOLDEN_BAR)


def zero_weight_problem(prob, mus):
    mus = np.atleast_1d(np.asarray(mus, dtype=np.float64))
    return dataclasses.replace(prob, muz=mus.copy(), wmu=np.zeros_like(mus))


def without_profiles(prob, block):
    """a ray-dependent context's profile arrays are per ray: at other angles they are rebuilt from the profile inputs"""
    return block if prob.phi_compact else dataclasses.replace(block, phi=None, wphi=None)


def oracle_engine(oracle_lib, prob, block, prof, mus, n, J, solver='linear', threads=16):
    """the zero-weight oracle context, loaded: columns, profiles at the new angles, populations and J"""
    p2 = zero_weight_problem(prob, mus)
    e = Engine(p2, block.ncol, lib=oracle_lib)
    oracle_lib.dll.lsx_oracle_set_threads(e._h, int(threads))
    synth.load_columns(e, without_profiles(prob, block), None if prob.phi_compact else prof)
    e.set_formal_solver(solver)
    e.set(_capi.LSX_N, n)
    e.set(_capi.LSX_J, J)
    return e


def oracle_rays(oracle_lib, prob, block, prof, mus, n, J, solver='linear'):
    """-> [ncol][Nspect][nmu]: what the reference computes on atmos.rays(mus) from these populations and this J"""
    e = oracle_engine(oracle_lib, prob, block, prof, mus, n, J, solver)
    with np.errstate(all='ignore'):
        e.formal_sol_gamma()
    out = e.get(_capi.LSX_I)
    e.close()
    return out


def golden_case(name):
    """-> (prob, block, prof, n [1][NLtot][Ns], J [1][Nspect][Ns], mus, I_ref [Nspect][nmu]) of a case of rays_falc.npz"""
    g = np.load(golden('rays_falc.npz'))
    fixture, ntag, jkey = {'ca': ('falc_ca.npz', 'conv', 'conv_J'), 'ca_vlos': ('falc_ca_vlos.npz', 'se5', 'last_J'),
                           'cah': ('falc_cah.npz', 'se5', 'last_J')}[name]
    prob, block, raw = fixtures.load_problem_npz(golden(fixture))
    prof = None if prob.phi_compact else fixtures.profile_inputs(prob, raw)
    n = fixtures.pops_from_raw(raw, ntag, prob)[None]
    return prob, block, prof, n, np.array(raw[jkey])[None], np.array(g['mus']), np.array(g['%s_I' % name])


def relmax(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / np.abs(b)))


@functools.lru_cache(maxsize=None)
def _oracle_golden(oracle_lib, name):
    prob, block, prof, n, J, mus, I_ref = golden_case(name)
    return oracle_rays(oracle_lib, prob, block, prof, mus, n, J)[0]


def dev_ref(oracle_lib, name):
    """how far the oracle's zero-weight context is from the reference on a golden case (largest relative deviation)"""
    return relmax(_oracle_golden(oracle_lib, name), golden_case(name)[-1])


def batch(fixture, ncol, first=0, seed=1234):
    """FALC-perturbed columns with a line-of-sight velocity: ray-dependent profiles built by the library"""
    prob, base, raw = fixtures.load_problem_npz(golden(fixture), phi_compact=False)
    block, prof = synth.perturbed_columns(prob, base, raw, ncol, seed=seed, vlos_sigma=2.0e3, first=first)
    assert prof is not None and block.phi is None
    return prob, block, prof


def mali(engine, iterations=5, se_from=3):
    """five MALI iterations, the last two with a statistical equilibrium: the state a final pass starts from"""
    for it in range(iterations):
        engine.formal_sol_gamma()
        if it >= se_from:
            engine.stat_equil()


def envelope_runs(oracle_lib, prob, block, prof, mus, n, J, solver='linear'):
    """the oracle's zero-weight context as it is and with every exp(-dtau) a ulp up / down (tests/envelope.py)"""
    import envelope

    def make():
        return oracle_engine(oracle_lib, prob, block, prof, mus, n, J, solver)
    with np.errstate(all='ignore'):
        return envelope.oracle_runs(oracle_lib, make, 1, what=(_capi.LSX_I,))


def runs_subset(runs, cols=slice(None), angles=slice(None)):
    """the runs of some columns / some angles of a zero-weight context (rays and columns are independent in the oracle)"""
    return {u: [{_capi.LSX_I: s[_capi.LSX_I][cols][:, :, angles]} for s in snaps] for u, snaps in runs.items()}
