"""Radiative rates from a converged context (include/lsx_hip_rates.h, lsx_hip_radiative_rates): what can be checked without a GPU.

The checker of the GPU tests (tests/rates_cases.py: a fresh oracle engine, one formal solution, lsx_oracle_rates) is held against the
reference's own fs1_Rij / fs1_Rji here; the numpy restatement of a continuum's rates validates itself on the oracle's continuum Rij;
and the rate equations fix what "physical Rji" means before the GPU is involved."""
import os
import re
import subprocess

import numpy as np
import pytest

import rates_cases as rt
from conftest import ROOT, golden
from lightspinner_amd import _capi, fixtures
from lightspinner_amd.problem import Engine, RadiativeRates

CSRC = os.path.join(ROOT, 'lightspinner_amd', 'csrc')


@pytest.mark.parametrize('case', list(rt.GOLDEN_FIXTURES))
def test_the_checker_reproduces_the_reference_first_call(oracle_lib, case):
    """measured, largest relative deviation (Rij, Rji): ca 5e-15, 3e-15; cah 9e-14, 3e-14; c 4e-14, 4e-14; fe 4e-14, 4e-14;
    mg 1.5e-14, 6e-15"""
    prob, block, raw = fixtures.load_problem_npz(golden(rt.GOLDEN_FIXTURES[case]))
    Rij_ref, Rji_ref = rt.golden_rates(raw, prob)
    assert np.all(Rij_ref > 0) and np.all(Rji_ref > 0)          # no golden entry is zero: relative bars entry by entry
    r = rt.oracle_rates(oracle_lib, prob, block)
    dij = float(np.max(np.abs(r[rt.RIJ][0] - Rij_ref) / Rij_ref))
    dji = float(np.max(np.abs(r[rt.RJI_REF][0] - Rji_ref) / Rji_ref))
    print('%s: oracle against the reference: Rij %.1e, Rji %.1e' % (case, dij, dji))
    assert dij <= rt.GOLDEN_BAR and dji <= rt.GOLDEN_BAR


@pytest.mark.parametrize('case', ['ca', 'cah'])
def test_the_continuum_restatement_reproduces_the_oracle(oracle_lib, case):
    """the restatement without g and 2hc / lambda^3 is the oracle's continuum Rij (measured: at most 4.3e-15)"""
    prob, block, raw = fixtures.load_problem_npz(golden(rt.GOLDEN_FIXTURES[case]))
    r = rt.oracle_rates(oracle_lib, prob, block)
    worst = 0.0
    for kr, t in enumerate(prob.trans):
        if t.is_line:
            continue
        mine = rt.continuum_rates(prob, block, kr, r[_capi.LSX_J])[0]
        worst = max(worst, float(np.max(np.abs(mine - r[rt.RIJ][:, kr]) / r[rt.RIJ][:, kr])))
    print('%s: continuum restatement against the oracle: %.1e' % (case, worst))
    assert any(not t.is_line for t in prob.trans) and worst <= 1e-13


def test_the_rate_equations_close_with_the_physical_rji(oracle_lib):
    """converged FALC CaII, one further formal solution: sum_j n_j (R + C)_{j -> i} = n_i sum_j (R + C)_{i -> j} within 2e-3 of the
    gross rate -- twice the loop's stop threshold (test.py:23) -- at every level and depth (measured: 9.9e-4, level 0 at depth 29);
    with the reference's Rji (Vij in the stimulated term) it misses by more than 0.05 (measured: 0.98)"""
    prob, block, prof, n, J = rt.later_state('ca')
    r = rt.oracle_rates(oracle_lib, prob, block, prof, n, J)
    phys = rt.physical_rji(prob, block, r)
    miss = rt.closure(prob, block, n[0], r[rt.RIJ][0], phys[0])
    lev, k = np.unravel_index(np.argmax(miss), miss.shape)
    miss_ref = rt.closure(prob, block, n[0], r[rt.RIJ][0], r[rt.RJI_REF][0])
    print('closure: physical Rji %.2e (level %d, depth %d); reference form %.2e' % (miss.max(), lev, k, miss_ref.max()))
    assert miss.max() <= 2e-3
    assert miss_ref.max() > 0.05


def test_the_oracle_has_no_such_entry_and_the_engine_says_so(oracle_lib):
    prob, block, raw = fixtures.load_problem_npz(golden('falc_ca.npz'))
    e = Engine(prob, 1, lib=oracle_lib)
    e.set_columns(0, block)
    assert not oracle_lib.has_radiative_rates
    with pytest.raises(NotImplementedError, match='lsx_hip_radiative_rates'):
        e.radiative_rates()
    e.close()


def test_net_is_the_net_radiative_bracket():
    rng = np.random.default_rng(7)
    Rij, Rji, Rref = (rng.uniform(1.0, 2.0, size=(3, 5)) for _ in range(3))
    pops = [(rng.uniform(1.0, 2.0, size=5), rng.uniform(1.0, 2.0, size=5)) for _ in range(3)]
    r = RadiativeRates(Rij, Rji, Rref, transitions=['a', 'b', 'c'], populations=pops)
    net = r.net()
    assert net.shape == (3, 5)
    for kr, (ni, nj) in enumerate(pops):
        assert np.array_equal(net[kr], nj * Rji[kr] - ni * Rij[kr])
    with pytest.raises(ValueError):
        RadiativeRates(Rij, Rji, Rref).net()


def test_the_entry_is_exported_and_declared_in_a_header_of_its_own():
    lib = os.path.join(CSRC, 'liblsx_hip.so')
    assert os.path.exists(lib), 'build the HIP library first (make -C lightspinner_amd/csrc)'
    syms = subprocess.run(['nm', '-D', '--defined-only', lib], capture_output=True, text=True, check=True).stdout
    hdr = open(os.path.join(ROOT, 'include', 'lsx_hip_rates.h')).read()
    declared = set(re.findall(r'\b(lsx_hip_[a-z0-9_]+)\s*\(', hdr))
    assert declared == {'lsx_hip_radiative_rates', 'lsx_hip_radiative_rates_work_cap'}
    for s in declared:
        assert re.search(r'\bT %s\b' % s, syms), s
    assert 'lsx_hip_radiative_rates' not in _capi.REQUIRED_SYMBOLS            # the common ABI is what it was
    assert '#include "lsx_hip_rates.h"' in open(os.path.join(ROOT, 'include', 'lsx_hip.h')).read()
    assert re.search(r'accumulates', hdr, re.I) and re.search(r'does not accumulate', hdr)


@pytest.mark.parametrize('compiler,std', [('gcc', 'c99'), ('g++', 'c++11')])
def test_the_header_compiles_alone(compiler, std):
    lang = 'c' if compiler == 'gcc' else 'c++'
    r = subprocess.run([compiler, '-std=' + std, '-Wall', '-Wextra', '-pedantic', '-Werror', '-fsyntax-only', '-x', lang,
                        os.path.join(ROOT, 'include', 'lsx_hip_rates.h')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# what DESIGN.md 4.11 states for the pass's instances: waves per SIMD by rays per lane, (linear, parabolic)
OCCUPANCY = {1: (6, 4), 2: (5, 4), 3: (4, 3), 4: (3, 3), 5: (2, 2)}


def test_the_kernels_use_no_scratch_and_have_the_stated_occupancy():
    """build/lsx_rates.ru.log, the compiler's resource report of the new unit"""
    path = os.path.join(CSRC, 'build', 'lsx_rates.ru.log')
    assert os.path.exists(path), 'build the HIP library first (make -C lightspinner_amd/csrc)'
    blocks = re.split(r'remark: [^\n]*Function Name: ', open(path).read())[1:]
    seen, reduce_seen = {}, False
    for b in blocks:
        name = b.split()[0]
        val = lambda key: int(re.search(re.escape(key) + r':? (\d+)', b).group(1))
        assert val('ScratchSize [bytes/lane]') == 0, name
        assert val('VGPRs Spill') == 0, name
        assert re.search(r'Dynamic Stack: False', b), name
        m = re.search(r'k_rates_passILi(\d+)ELb([01])E', name)
        if m:
            assert val('LDS Size [bytes/block]') == 1024, name          # the exponential's table, nothing that grows with Nspace
            seen[(int(m.group(1)), int(m.group(2)))] = val('Occupancy [waves/SIMD]')
        else:
            assert 'k_rates_reduce' in name, name
            assert val('LDS Size [bytes/block]') == 0, name
            reduce_seen = True
    assert reduce_seen
    assert seen == {(nm, par): occ[par] for nm, occ in OCCUPANCY.items() for par in (0, 1)}, seen
