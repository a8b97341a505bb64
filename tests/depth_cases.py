"""Shared cases of the depth-resolved final pass (tests/test_depth_rays_host.py, tests/test_depth_rays.py).

The pin: tests/golden/depth_falc_<case>_<block>.npz hold what the unmodified reference builds inside its final pass on
`Falc82().rays(MUS)` (tests/golden/make_depth_golden.py): chiTot, S and the I of every depth of the up-going rays.  The checkers need
nothing new in the oracle:
  chi, S    `restate_chi_S`, a numpy restatement of rh_method.py:601-632 from the problem, the column block, n, J and line profiles
            read back with lsx_get(LSX_PHI) from a zero-weight context on the wanted angles (tests/rays_cases.py);
  I(k)      the oracle's unit entries for one ray (lsx_piecewise_linear_1d; lsx_piecewise_parabolic_1d_impl with the thermalised
            lower boundary of formal_solver.py:205-207 from lsx_oracle_planck), fed chi and S, as they are and with every
            exp(-dtau) an ulp up / down: the bar is the suite's rule for a first formal solution, BASE |x| + 3 |x(+1) - x(-1)|;
  tau, contrib, z_tau1   numpy from the arrays under test themselves.
"""
import dataclasses
import functools
import glob
import os

import numpy as np

import rays_cases as rc
from conftest import GOLDEN
from lightspinner_amd import _capi
from lightspinner_amd import constants as Const
from lightspinner_amd.problem import Engine

MUS = np.array([0.1, 0.6, 1.0])
CASES = ('ca', 'ca_vlos', 'cah')
U = 2.0 ** -53
BASE_I = 1e-11                 # I(k) against the oracle's unit entry, beside the one-ulp-exp envelope (tests/envelope.py)
K_ENVELOPE = 3.0
BASE_CHI_S = 1e-12             # chi, S against the restatement: the suite's base for FALC problems (no exponential of the weights enters)
# the restatement against the reference's recorded chi and S, largest relative deviation per case measured on the CPU with the
# oracle's profiles (tests/test_depth_rays_host.py asserts d_cpu + 1e-12; the GPU test adds d_cpu to its bar against the fixture)
D_CPU = {'ca': {'chi': 0.0, 'S': 0.0}, 'ca_vlos': {'chi': 2.5e-14, 'S': 2.5e-14}, 'cah': {'chi': 0.0, 'S': 0.0}}
DENORM = 2.0 ** -1074          # the spacing of float64 below 2.2e-308: no result down there can be held to a relative bar


@functools.lru_cache(maxsize=None)
def fixture(case):
    """-> {'mus', 'chi', 'S', 'I'}: the arrays [Nspect][nmu][Nspace] of a case, its wavelength blocks put together"""
    paths = sorted(glob.glob(os.path.join(GOLDEN, 'depth_falc_%s_[0-9]*.npz' % case)),
                   key=lambda p: int(p.rsplit('_', 1)[1].split('.')[0]))
    assert paths, 'tests/golden/depth_falc_%s_*.npz are missing (tests/golden/make_depth_golden.py)' % case
    parts = [np.load(p) for p in paths]
    at = 0
    for p in parts:
        assert int(p['la0']) == at and np.array_equal(p['mus'], MUS)
        at += p['chi'].shape[0]
    out = {k: np.concatenate([p[k] for p in parts]) for k in ('chi', 'S', 'I')}
    out['mus'] = MUS.copy()
    for a in out.values():
        a.setflags(write=False)
    return out


def to_lambda_major(a):
    """[nmu][Nspace][nla] (the entry's layout, one column) -> [nla][nmu][Nspace] (the fixture's)"""
    return np.ascontiguousarray(np.moveaxis(np.asarray(a), -1, 0))


def relmax(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / np.abs(b)))


# ---- chi, S: rh_method.py:601-632 -----------------------------------------------------------------------------------------------------
def phi_offsets(prob):
    off, o = {}, 0
    for kr, t in enumerate(prob.trans):
        if t.is_line:
            off[kr] = o
            o += t.Nlambda
    return off


def restate_chi_S(prob, block, n, J, phi, nmu, col=0, la0=0, nla=None):
    """chiTot and S of the up-going direction (rh_method.py:601-632) for one column -> ([nla][nmu][Nspace], same).
    n [NLtot][Nspace], J [Nspect][Nspace] of that column; phi: LSX_PHI of that column, [SNl][nmu][2][Nspace] from a context whose
    rays are the wanted angles (or the compact [SNl][Nspace]: ray independent)."""
    nla = prob.Nspect - la0 if nla is None else nla
    Ns = prob.Nspace
    hc_4pi = 0.25 * Const.HC / np.pi
    hc_k = Const.HC / (Const.KBoltzmann * Const.NM_TO_M)
    poff = phi_offsets(prob)
    T = block.temperature[col]
    chi_out, S_out = np.empty((nla, nmu, Ns)), np.empty((nla, nmu, Ns))
    for q in range(nla):
        la = la0 + q
        wav = prob.wavelength[la]
        chiTot, etaTot = np.zeros((nmu, Ns)), np.zeros((nmu, Ns))
        for kr, t in enumerate(prob.trans):
            if not prob.active[kr, la]:
                continue
            lt = la - t.Nblue
            o = int(prob.lev_off[t.atom])
            ni, nj = n[o + t.i], n[o + t.j]
            if t.is_line:
                row = phi[poff[kr] + lt]
                ph = row[None, :] if prob.phi_compact else row[:, 1, :]          # toFrom = 1: up-going
                Vij = hc_4pi * t.Bij * ph                                      # :279-281
                Vji = (t.Bji / t.Bij) * Vij
                Uji = t.Aji / t.Bji * Vji
            else:
                gij = block.nStar[col, o + t.i] / block.nStar[col, o + t.j] * np.exp(-hc_k / wav / T)      # :453-454
                Vij = np.full((1, Ns), float(t.alpha[lt]))                    # :284-286
                Vji = gij * Vij
                Uji = 2.0 * Const.HC / (Const.NM_TO_M * wav) ** 3 * Vji
            chiTot += ni * Vij - nj * Vji                                      # :613, :625
            etaTot += nj * Uji                                                 # :614, :626
        chiTot += block.bg_chi[col, la]                                        # :630
        sca = block.bg_sca[col, la] if prob.sca_per_lambda else block.bg_sca[col]
        chi_out[q] = chiTot
        S_out[q] = (etaTot + block.bg_eta[col, la] + sca * J[la]) / chiTot     # :632
    return chi_out, S_out


def profiles_at(lib, prob, block, prof, mus):
    """LSX_PHI of a zero-weight context on `mus` bound to `lib` (the oracle on the CPU, the HIP library on the GPU): [ncol] + phi_shape"""
    from lightspinner_amd import synth
    e = Engine(rc.zero_weight_problem(prob, mus), block.ncol, lib=lib)
    synth.load_columns(e, block if prof is None else dataclasses.replace(block, phi=None, wphi=None), prof)
    phi = e.get(_capi.LSX_PHI)
    e.close()
    return phi


# ---- I(k) from chi and S: the oracle's unit entries ------------------------------------------------------------------------------------
def oracle_I(oracle_lib, height, temperature, wavelength, mus, chi, S, solver='linear'):
    """chi, S [nla][nmu][Nspace] of one column, wavelength [nla] -> the up-going I at every depth, same shape: formal_solver.py:144-212
    (linear) or the parabolic rule with the same thermalised lower boundary"""
    nla, nmu, Ns = chi.shape
    c2, S2 = np.ascontiguousarray(chi).reshape(-1, Ns), np.ascontiguousarray(S).reshape(-1, Ns)
    mu = np.tile(np.asarray(mus, dtype=np.float64), nla)
    wav = np.repeat(np.asarray(wavelength, dtype=np.float64), nmu)
    up = np.ones(nla * nmu, dtype=np.int32)
    if solver == 'linear':
        I, _ = oracle_lib.piecewise_linear_1d(height, temperature, mu, up, wav, c2, S2)
    else:
        z = np.asarray(height, dtype=np.float64)
        dtau_uw = (1.0 / mu) * (c2[:, -1] + c2[:, -2]) * 0.5 * abs(z[-1] - z[-2])              # formal_solver.py:205
        planck = oracle_lib.dll.lsx_oracle_planck
        B0 = np.array([planck(float(temperature[-2]), float(w)) for w in wav])                  # :206
        B1 = np.array([planck(float(temperature[-1]), float(w)) for w in wav])
        Istart = B1 - (B0 - B1) / dtau_uw                                                       # :207
        I, _ = oracle_lib.piecewise_parabolic_1d_impl(height, mu, up, Istart, c2, S2)
    return I.reshape(nla, nmu, Ns)


def oracle_I_runs(oracle_lib, *args, **kw):
    """-> {0, +1, -1: I}: the unit entry as it is and with every exp(-dtau) an ulp up / down"""
    out = {}
    try:
        for ulp in (0, 1, -1):
            oracle_lib.dll.lsx_oracle_set_exp_ulp(int(ulp))
            out[ulp] = oracle_I(oracle_lib, *args, **kw)
    finally:
        oracle_lib.dll.lsx_oracle_set_exp_ulp(0)
    return out


def excess_I(I, runs, base=BASE_I):
    """how far I lies outside base |x| + 3 |x(+1) - x(-1)| entry by entry, as a multiple of that bound (<= 1: inside); the largest
    relative deviation and the largest relative envelope for the record"""
    x0 = runs[0]
    env = np.abs(runs[1] - runs[-1])
    bound = base * np.abs(x0) + K_ENVELOPE * env
    dev = np.abs(np.asarray(I) - x0)
    return float(np.max(dev / bound)), float(np.max(dev / np.abs(x0))), float(np.max(env / np.abs(x0)))


# ---- tau, contrib, z_tau1 from the arrays under test -------------------------------------------------------------------------------------
def tau_of(chi, mus, z):
    """chi [nmu][Nspace][nla] -> tau likewise: formal_solver.py:129 summed from the top in index order (np.cumsum, float64)"""
    dz = np.abs(z[:-1] - z[1:])
    zmu = 1.0 / np.asarray(mus, dtype=np.float64)
    dtau = 0.5 * (chi[:, :-1, :] + chi[:, 1:, :]) * zmu[:, None, None] * dz[None, :, None]
    return np.concatenate([np.zeros_like(chi[:, :1, :]), np.cumsum(dtau, axis=1)], axis=1)


def check_tau(tau, chi, mus, z):
    """(Nspace + 8) u tau: sequential summation of positive terms, each with <= 4 roundings plus the 2-ulp reciprocal.
    -> the largest deviation as a multiple of the bound"""
    ref = tau_of(chi, mus, z)
    assert np.all(tau[:, 0, :] == 0.0)
    bound = (chi.shape[1] + 8) * U * ref[:, 1:, :]
    r = float(np.max(np.abs(tau[:, 1:, :] - ref[:, 1:, :]) / bound))
    assert r <= 1.0, 'tau: %.2f x the bound' % r
    return r


def check_contrib(contrib, chi, S, tau, mus):
    """16 u relative where tau <= 700 (plus the spacing of the denormals: a value below 2.2e-308 has no 53 bits to be held to);
    0 <= contrib <= chi S exp(-700) / mu beyond.  No entry is skipped.  -> the largest deviation as a multiple of the bound"""
    mu = np.asarray(mus, dtype=np.float64)[:, None, None]
    assert np.all(contrib >= 0.0)
    thin = tau <= 700.0
    ref = chi * S * np.exp(-np.where(thin, tau, 0.0)) / mu
    bound = 16 * U * ref + 4 * DENORM
    r = float(np.max(np.where(thin, np.abs(contrib - ref) / bound, 0.0)))
    assert r <= 1.0, 'contrib: %.2f x the bound' % r
    cap = chi * S * np.exp(-700.0) / mu
    assert np.all(contrib[~thin] <= cap[~thin])
    return r


def z_tau1_of(tau, z):
    """tau [nmu][Nspace][nla] -> [nmu][nla]: linear interpolation of z to tau = 1 in the first interval that reaches it, NaN if none"""
    nmu, Ns, nla = tau.shape
    hit = tau >= 1.0
    k = np.argmax(hit, axis=1)                               # the first index with tau >= 1 (0 if none: tau[0] = 0 never is)
    none = ~np.any(hit, axis=1)
    k1 = np.maximum(k, 1)
    t1 = np.take_along_axis(tau, k1[:, None, :], axis=1)[:, 0, :]
    t0 = np.take_along_axis(tau, (k1 - 1)[:, None, :], axis=1)[:, 0, :]
    out = z[k1 - 1] + (1.0 - t0) / (t1 - t0) * (z[k1] - z[k1 - 1])
    return np.where(none, np.nan, out)


def check_z_tau1(z_tau1, tau, z):
    """16 u max|z| absolute; NaN exactly where tau never reaches 1"""
    ref = z_tau1_of(tau, z)
    assert np.array_equal(np.isnan(z_tau1), np.isnan(ref))
    ok = ~np.isnan(ref)
    bound = 16 * U * np.max(np.abs(z))
    r = float(np.max(np.abs(z_tau1[ok] - ref[ok]), initial=0.0) / bound)
    assert r <= 1.0, 'z_tau1: %.2f x the bound' % r
    return r


def same(a, b, cols=slice(None), fields=('chi', 'S', 'tau', 'I', 'contrib', 'z_tau1')):
    """two DepthRays hold the same bits (NaN in z_tau1 equal to NaN)"""
    return all(np.array_equal(getattr(a, f), getattr(b, f)[cols], equal_nan=True) for f in fields)
