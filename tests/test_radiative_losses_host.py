"""Radiative flux, net cooling and its division among the transitions (include/lsx_hip_losses.h, lsx_hip_radiative_losses): what
can be checked without a GPU.

The fixture from the unmodified reference (tests/golden/make_losses_golden.py, tests/losses_cases.py) is held against identities
that hold exactly or to rounding, and against numpy restatements of the definitions from the problem, the column and the
fixture's own mean intensity -- the factorisations the kernels' second stage uses (a line through P = phi Jp and Phi = phi W where
the profile does not depend on the ray, a continuum through Jp, g and W).  The frequency weights of the library's grid code, the
arithmetic of RadiativeLosses, the header and the compiler's resource report of the new unit are checked here too."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import depth_cases as dc
import losses_cases as lc
import rates_cases as rt
from conftest import ROOT, golden
from lightspinner_amd import _capi, fixtures
from lightspinner_amd import constants as Const
from lightspinner_amd.problem import Engine, RadiativeLosses

CSRC = os.path.join(ROOT, 'lightspinner_amd', 'csrc')
U = 2.0 ** -53


# ---- the fixture's identities ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', lc.CASES)
def test_the_fixture_identities(case):
    fx = lc.fixture(case)
    prob, block, prof, n, J = lc.state(case)
    idx = fx['la_idx']
    hw, mu = lc.half_weights(prob), np.asarray(prob.muz)
    assert fx['H'].shape == fx['D'].shape == (idx.shape[0], prob.Nspace) and fx['Qt'].shape == (prob.Ntrans, prob.Nspace)
    t0 = next(t for t in prob.trans if t.is_line)
    assert set(range(0, prob.Nspect, 4)) <= set(idx) and set(range(t0.Nblue, t0.Nblue + t0.Nlambda)) <= set(idx)
    # at the top nothing comes down: H[la][0] = Hg[la][0] = sum wmu/2 mu I_top, in the order of the definition: bit for bit
    top = np.zeros(idx.shape[0])
    for m in range(prob.Nrays):
        top += hw[m] * mu[m] * fx['I_top'][idx, m]
    assert np.array_equal(fx['H'][:, 0], top) and np.array_equal(fx['Hg'][:, 0], top)
    # every gross bounds its quantity: Gd -+ D = 2 sum wmu/2 (chi I | eta) >= 0, and so on
    assert np.all(fx['Gd'] > 0) and np.all(np.abs(fx['D']) <= fx['Gd'])
    assert np.all(fx['Hg'] > 0) and np.all(np.abs(fx['H']) <= fx['Hg'])
    assert np.all(fx['Hg'] <= np.max(mu) * fx['J_pass'][idx] * (1 + 8 * U))          # mu <= max mu inside the sum
    assert np.all(fx['Qtg'] > 0) and np.all(np.abs(fx['Qt']) <= fx['Qtg'])
    assert np.all(fx['Qg'] > 0) and np.all(np.abs(fx['Q']) <= fx['Qg']) and np.all(np.abs(fx['F']) <= fx['Fg'])
    # the flux leaves the atmosphere, and the stored weights are the trapezoid rule
    assert fx['F'][0] > 0 and np.array_equal(fx['wnu'], lc.trapezoid_wnu(prob.wavelength))
    # deep down the cancellation the bars are built around: |Q| is a small fraction of its gross
    assert abs(fx['Q'][-1]) < 0.1 * fx['Qg'][-1]


@pytest.mark.parametrize('case', ['ca', 'cah'])
def test_the_definitions_restated_reproduce_the_fixture(case):
    """profiles that do not depend on the ray: D = eta W - chi Jp, a line's Qt through phi Jp and phi W, a continuum's through Jp,
    g and W -- from the problem, the column and the fixture's own Jp.  Measured, relative to the gross: D 5.3e-16, Qt 1.4e-15 (ca);
    D 5.5e-16, Qt 4.2e-15 (cah); the bar is 64 roundings (sums of up to a few hundred terms)"""
    fx = lc.fixture(case)
    prob, block, prof, n, J = lc.state(case)
    assert prob.phi_compact and block.phi is not None
    idx, Jp, W = fx['la_idx'], fx['J_pass'], lc.weight_sum(prob)
    chi, S = dc.restate_chi_S(prob, block, n[0], J[0], block.phi[0], 1)
    chi, S = chi[idx, 0], S[idx, 0]
    D = (S * chi) * W - chi * Jp[idx]
    dD = float(np.max(np.abs(D - fx['D']) / fx['Gd']))
    # Qt: (hc / lambda) 4 pi wla [n_j (Uji W + Vji Jp) - n_i Vij Jp]
    poff, hc_k = dc.phi_offsets(prob), Const.HC / (Const.KBoltzmann * Const.NM_TO_M)
    Qt, line = np.zeros_like(fx['Qt']), 0
    for kr, t in enumerate(prob.trans):
        sl = slice(t.Nblue, t.Nblue + t.Nlambda)
        lam = prob.wavelength[sl]
        act = prob.active[kr, sl].astype(bool)[:, None]
        o = int(prob.lev_off[t.atom])
        ni, nj = n[0, o + t.i][None], n[0, o + t.j][None]
        if t.is_line:
            wla = rt.wlambda(prob, t)[:, None] * block.wphi[0, line][None] / Const.HC
            Vij = 0.25 * Const.HC / np.pi * t.Bij * block.phi[0, poff[kr]:poff[kr] + t.Nlambda]
            Vji = (t.Bji / t.Bij) * Vij
            Uji = t.Aji / t.Bji * Vji
            line += 1
        else:
            wla = (rt.wlambda(prob, t) / lam / Const.HPlanck)[:, None]
            g = (block.nStar[0, o + t.i] / block.nStar[0, o + t.j])[None] * np.exp(-hc_k / lam[:, None] / block.temperature[0][None])
            Vij = np.asarray(t.alpha, dtype=np.float64)[:, None] * np.ones((1, prob.Nspace))
            Vji = g * Vij
            Uji = (2.0 * Const.HC / (Const.NM_TO_M * lam) ** 3)[:, None] * Vji
        e_phot = (Const.HC / (lam * Const.NM_TO_M))[:, None]
        term = e_phot * lc.FOUR_PI * wla * (nj * (Uji * W + Vji * Jp[sl]) - ni * Vij * Jp[sl])
        Qt[kr] = np.sum(np.where(act, term, 0.0), axis=0)
    dQ = float(np.max(np.abs(Qt - fx['Qt']) / fx['Qtg']))
    print('%s: restated against the fixture, relative to the gross: D %.1e, Qt %.1e' % (case, dD, dQ))
    assert dD <= 64 * U and dQ <= 64 * U
    # ... and the positive-coefficient form the GPU tests' bars use is the gross's absorption and stimulated part at most
    coefs = lc.qt_coefficients(prob, block, n[0], block.phi[0], block.wphi[0])
    assert np.all(lc.qt_envelope(coefs, Jp) <= fx['Qtg'] * (1 + 64 * U))


# ---- the frequency weights -----------------------------------------------------------------------------------------------------------
def _weights(hip_lib, lam):
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    w = np.full_like(lam, np.nan)
    dp = C.POINTER(C.c_double)
    return hip_lib.dll.lsx_hip_frequency_weights(lam.shape[0], lam.ctypes.data_as(dp), w.ctypes.data_as(dp)), w


def test_the_trapezoid_weights_against_numpy(hip_lib):
    """the reference's 777-point Ca + H grid, a two-point grid and one point; the sum of the weights is the band's width.  The
    library divides c by lambda * 1e-9 as the restatement does: bit for bit"""
    prob, _, _ = fixtures.load_problem_npz(golden('falc_cah.npz'))
    assert prob.Nspect == 777
    for lam in (prob.wavelength, np.array([121.0, 122.5]), np.array([500.0])):
        rc, w = _weights(hip_lib, lam)
        assert rc == 0 and np.array_equal(w, lc.trapezoid_wnu(lam))
    rc, w = _weights(hip_lib, prob.wavelength)
    nu = Const.CLight / (prob.wavelength * Const.NM_TO_M)
    assert abs(w.sum() - (nu[0] - nu[-1])) <= 1e-12 * nu[0]
    rc, w = _weights(hip_lib, np.array([121.0, 122.5]))
    assert w[0] == w[1] > 0
    for bad in (np.array([500.0, 400.0]), np.array([0.0, 1.0]), np.array([1.0, np.nan])):
        assert _weights(hip_lib, bad)[0] == _capi.LSX_EINVAL
    assert hip_lib.dll.lsx_hip_frequency_weights(0, None, None) == _capi.LSX_EINVAL


# ---- RadiativeLosses ---------------------------------------------------------------------------------------------------------------------
def test_radiative_losses_arithmetic():
    rng = np.random.default_rng(11)
    Qt = rng.normal(size=(2, 3, 5))
    r = RadiativeLosses(np.ones(4), Qt=Qt)
    assert r.F is None and r.H is None and np.array_equal(r.total(), Qt[:, 0] + Qt[:, 1] + Qt[:, 2])
    assert np.array_equal(r.by_transition([2, 0])[2], Qt[:, 2]) and np.array_equal(r.by_transition(1)[1], Qt[:, 1])
    with pytest.raises(ValueError):
        r.by_transition(['a line'])                      # no transitions to look the name up in

    class T:
        def __init__(self, name):
            self.name = name
    trans = [T('Ca II K'), T('Ca II H'), T('Ca II H')]
    one = RadiativeLosses(np.ones(4), Qt=Qt[0], transitions=trans)
    assert np.array_equal(one.total(), Qt[0].sum(axis=0)) and one.total().shape == (5,)
    got = one.by_transition(['Ca II K', trans[2]])
    assert np.array_equal(got['Ca II K'], Qt[0, 0]) and np.array_equal(got[trans[2]], Qt[0, 2])
    with pytest.raises(KeyError):
        one.by_transition('Ca II H')                     # two of them carry the name
    with pytest.raises(KeyError):
        one.by_transition('Mg II k')
    with pytest.raises(ValueError):
        RadiativeLosses(np.ones(4), F=np.zeros((1, 5))).total()


def test_the_oracle_has_no_such_entry_and_the_engine_says_so(oracle_lib):
    prob, block, raw = fixtures.load_problem_npz(golden('falc_ca.npz'))
    e = Engine(prob, 1, lib=oracle_lib)
    e.set_columns(0, block)
    assert not oracle_lib.has_radiative_losses
    with pytest.raises(NotImplementedError, match='lsx_hip_radiative_losses'):
        e.radiative_losses()
    with pytest.raises(NotImplementedError, match='lsx_hip_frequency_weights'):
        e.frequency_weights()
    e.close()


# ---- the entry, its header, its kernels ----------------------------------------------------------------------------------------------------
def test_the_entry_is_exported_and_declared_in_a_header_of_its_own():
    lib = os.path.join(CSRC, 'liblsx_hip.so')
    assert os.path.exists(lib), 'build the HIP library first (make -C lightspinner_amd/csrc)'
    syms = subprocess.run(['nm', '-D', '--defined-only', lib], capture_output=True, text=True, check=True).stdout
    hdr = open(os.path.join(ROOT, 'include', 'lsx_hip_losses.h')).read()
    declared = set(re.findall(r'\b(lsx_hip_[a-z0-9_]+)\s*\(', hdr))
    assert declared == {'lsx_hip_radiative_losses', 'lsx_hip_radiative_losses_work_cap', 'lsx_hip_frequency_weights'}
    for s in declared:
        assert re.search(r'\bT %s\b' % s, syms), s
    assert not any(s.startswith('lsx_hip_') for s in _capi.REQUIRED_SYMBOLS)            # the common ABI is what it was
    assert '#include "lsx_hip_losses.h"' in open(os.path.join(ROOT, 'include', 'lsx_hip.h')).read()
    # units, signs and the limit of the grid are stated
    for phrase in (r'W m\^-2', r'W m\^-3', r'POSITIVE TOWARDS THE OBSERVER', r'POSITIVE MEANS THE GAS LOSES ENERGY', r'dF/dz = Q',
                   r'ONLY AS BOLOMETRIC AS THAT GRID IS', r'\bHz\b'):
        assert re.search(phrase, hdr), phrase


@pytest.mark.parametrize('compiler,std', [('gcc', 'c99'), ('g++', 'c++11')])
def test_the_header_compiles_alone(compiler, std):
    lang = 'c' if compiler == 'gcc' else 'c++'
    r = subprocess.run([compiler, '-std=' + std, '-Wall', '-Wextra', '-pedantic', '-Werror', '-fsyntax-only', '-x', lang,
                        os.path.join(ROOT, 'include', 'lsx_hip_losses.h')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# what DESIGN.md 4.19 states for the pass's instances: waves per SIMD by rays per lane, (linear, parabolic)
OCCUPANCY = {1: (5, 4), 2: (4, 3), 3: (3, 3), 4: (3, 2), 5: (2, 2)}
SECOND_STAGE = ('k_losses_flux', 'k_losses_trans', 'k_losses_transpose')


def test_the_kernels_use_no_scratch_and_have_the_stated_occupancy():
    """build/lsx_losses.ru.log, the compiler's resource report of the new unit"""
    path = os.path.join(CSRC, 'build', 'lsx_losses.ru.log')
    assert os.path.exists(path), 'build the HIP library first (make -C lightspinner_amd/csrc)'
    blocks = re.split(r'remark: [^\n]*Function Name: ', open(path).read())[1:]
    seen, second = {}, set()
    for b in blocks:
        name = b.split()[0]
        val = lambda key: int(re.search(re.escape(key) + r':? (\d+)', b).group(1))
        assert val('ScratchSize [bytes/lane]') == 0, name
        assert val('VGPRs Spill') == 0, name
        assert re.search(r'Dynamic Stack: False', b), name
        m = re.search(r'k_losses_passILi(\d+)ELb([01])E', name)
        if m:
            assert val('LDS Size [bytes/block]') == 1024, name          # the exponential's table, nothing that grows with Nspace
            seen[(int(m.group(1)), int(m.group(2)))] = val('Occupancy [waves/SIMD]')
        else:
            hit = [s for s in SECOND_STAGE if re.search(r'\d+%sE' % s, name)]
            assert len(hit) == 1, name
            assert val('LDS Size [bytes/block]') == 0, name
            second.add(hit[0])
    assert second == set(SECOND_STAGE)
    assert seen == {(nm, par): occ[par] for nm, occ in OCCUPANCY.items() for par in (0, 1)}, seen
