"""Depth-resolved final pass (include/lsx_hip_depth.h, lsx_hip_depth_rays): what can be checked without a GPU.

The reference pin: tests/golden/depth_falc_<case>_<block>.npz hold chiTot, S and the I of every depth as the unmodified reference
builds them on `Falc82().rays(MUS)` from committed states (tests/golden/make_depth_golden.py).  The checkers of the GPU tests
(tests/depth_cases.py: the oracle's unit entry for I(k) given chi and S, a numpy restatement of rh_method.py:601-632 for chi and S)
are held against it here."""
import os
import re
import subprocess

import numpy as np
import pytest

import depth_cases as dc
import rays_cases as rc
from conftest import ROOT, golden
from lightspinner_amd import _capi, fixtures
from lightspinner_amd.problem import Engine

CSRC = os.path.join(ROOT, 'lightspinner_amd', 'csrc')


@pytest.mark.parametrize('case', dc.CASES)
def test_the_fixture_is_the_reference_final_pass_at_every_depth(oracle_lib, case):
    """the oracle's unit entry, fed the fixture's chi and S, gives the fixture's I(k) inside the rule for a first formal solution
    (measured: ca 1.5e-11 relative at worst, 0.13 x the bound; ca_vlos 5.1e-12, 0.12 x; cah 1.3e-11, 0.10 x), and I[..., 0] is
    rays_falc.npz bit for bit"""
    f = dc.fixture(case)
    prob, block, prof, n, J, mus_rays, I_rays = rc.golden_case(case)
    assert f['chi'].shape == f['S'].shape == f['I'].shape == (prob.Nspect, 3, prob.Nspace)
    assert all(np.all(f[k] > 0) for k in ('chi', 'S', 'I'))
    shared = [int(np.flatnonzero(mus_rays == m)[0]) for m in dc.MUS]
    assert np.array_equal(f['I'][:, :, 0], I_rays[:, shared])
    runs = dc.oracle_I_runs(oracle_lib, block.height[0], block.temperature[0], prob.wavelength, dc.MUS, f['chi'], f['S'])
    r, rel, renv = dc.excess_I(f['I'], runs)
    print('%s: the oracle on the fixture chi, S against the fixture I(k): %.2e relative at worst, envelope up to %.2e, %.3f x the bound'
          % (case, rel, renv, r))
    assert r <= 1.0
    tau = dc.tau_of(np.moveaxis(f['chi'], 0, -1), dc.MUS, block.height[0])
    assert np.all(tau[:, -1, :] >= 17.3)                    # tau = 1 is reached at every wavelength and angle of these cases


@pytest.mark.parametrize('case', dc.CASES)
def test_the_numpy_restatement_of_chi_and_S_is_the_reference(oracle_lib, case):
    """rh_method.py:601-632 restated in numpy (tests/depth_cases.py) from the oracle's profiles at MUS, against the recorded arrays:
    the largest relative deviation d_cpu per case and array is what depth_cases.D_CPU states (measured: ca and cah 0, bit for bit;
    ca_vlos 2.46e-14 chi, 4.75e-15 S)"""
    f = dc.fixture(case)
    prob, block, prof, n, J, _, _ = rc.golden_case(case)
    phi = dc.profiles_at(oracle_lib, prob, block, prof, dc.MUS)
    chi, S = dc.restate_chi_S(prob, block, n[0], J[0], phi[0], 3)
    for name, mine in (('chi', chi), ('S', S)):
        d = dc.relmax(mine, f[name])
        print('%s %s: restatement against the reference %.2e (stated d_cpu %.2e)' % (case, name, d, dc.D_CPU[case][name]))
        assert d <= dc.D_CPU[case][name] <= 1e-12              # (the stated figure is the measured one, and it is small)
        assert d <= dc.D_CPU[case][name] + 1e-12


def test_the_window_of_the_restatement_is_a_slice():
    prob, block, prof, n, J, _, _ = rc.golden_case('ca')
    phi = block.phi[0]
    a = dc.restate_chi_S(prob, block, n[0], J[0], phi, 1)
    b = dc.restate_chi_S(prob, block, n[0], J[0], phi, 1, la0=37, nla=5)
    assert np.array_equal(a[0][37:42], b[0]) and np.array_equal(a[1][37:42], b[1])
    f = dc.fixture('ca')                           # ... of the reference's arrays, bit for bit on this case (d_cpu = 0)
    assert np.array_equal(b[0][:, 0], f['chi'][37:42, 0]) and np.array_equal(b[1][:, 0], f['S'][37:42, 0])


def test_tau_contrib_and_z_tau1_checkers_on_a_hand_made_ray_and_on_the_fixture():
    """the checkers accept what numpy computes and refuse it a few ulp off: by hand, then on a line core of the fixture, where tau
    runs from 0 past 700 and the contribution function into the denormals"""
    prob, block, _, _, _, _, _ = rc.golden_case('ca')
    f = dc.fixture('ca')
    la = int(np.argmax(f['chi'][:, 0, 40]))                          # the most opaque wavelength at mid height
    chi, S = (np.moveaxis(f[k][la:la + 1], 0, -1) for k in ('chi', 'S'))      # [nmu][Nspace][1]
    zf = block.height[0]
    tau = dc.tau_of(chi, dc.MUS, zf)
    assert tau.max() > 700 and tau[:, 1, :].min() < 1
    contrib = chi * S * np.exp(-tau) / dc.MUS[:, None, None]
    dc.check_tau(tau, chi, dc.MUS, zf)
    dc.check_contrib(contrib, chi, S, tau, dc.MUS)
    dc.check_z_tau1(dc.z_tau1_of(tau, zf), tau, zf)
    with pytest.raises(AssertionError):
        dc.check_tau(tau * (1 + 1e-13), chi, dc.MUS, zf)
    with pytest.raises(AssertionError):
        dc.check_contrib(contrib * (1 + 1e-14), chi, S, tau, dc.MUS)
    with pytest.raises(AssertionError):
        dc.check_z_tau1(dc.z_tau1_of(tau, zf) + 1e-6, tau, zf)
    z = np.array([3.0, 2.0, 1.0, 0.0])
    chi = np.array([0.2, 0.6, 1.4, 2.0]).reshape(1, 4, 1)
    tau = dc.tau_of(chi, [0.5], z)
    assert np.allclose(tau[0, :, 0], [0.0, 0.8, 2.8, 6.2])
    zt = dc.z_tau1_of(tau, z)
    assert np.allclose(zt, 2.0 - 0.1) and np.isnan(dc.z_tau1_of(0.1 * tau, z)).all()
    S = np.full_like(chi, 2.0)
    dc.check_tau(tau, chi, [0.5], z)
    dc.check_contrib(chi * S * np.exp(-tau) / 0.5, chi, S, tau, [0.5])
    dc.check_z_tau1(zt, tau, z)
    with pytest.raises(AssertionError):
        dc.check_tau(tau * (1 + 1e-14), chi, [0.5], z)
    with pytest.raises(AssertionError):
        dc.check_contrib(chi * S * np.exp(-tau) / 0.5 * (1 + 1e-14), chi, S, tau, [0.5])


def test_the_entries_are_exported_and_declared_in_a_header_of_their_own():
    lib = os.path.join(CSRC, 'liblsx_hip.so')
    assert os.path.exists(lib), 'build the HIP library first (make -C lightspinner_amd/csrc)'
    syms = subprocess.run(['nm', '-D', '--defined-only', lib], capture_output=True, text=True, check=True).stdout
    text = open(os.path.join(ROOT, 'include', 'lsx_hip_depth.h')).read()
    declared = set(re.findall(r'\b(lsx_hip_[a-z0-9_]+)\s*\(', text))
    assert declared == {'lsx_hip_depth_rays', 'lsx_hip_depth_rays_work_cap'}
    exported = set(re.findall(r'\bT (lsx_hip_depth[a-z0-9_]*)\b', syms))
    assert exported == declared
    assert '#include "lsx_hip_depth.h"' in open(os.path.join(ROOT, 'include', 'lsx_hip.h')).read()
    assert not any(s.startswith('lsx_hip_depth') for s in _capi.REQUIRED_SYMBOLS)           # the common ABI is what it was
    assert 'lsx_hip_depth' not in open(os.path.join(ROOT, 'include', 'lsx.h')).read()


@pytest.mark.parametrize('compiler,std', [('gcc', 'c99'), ('g++', 'c++11')])
def test_the_header_compiles_alone(compiler, std):
    lang = 'c' if compiler == 'gcc' else 'c++'
    r = subprocess.run([compiler, '-std=' + std, '-Wall', '-Wextra', '-pedantic', '-Werror', '-fsyntax-only', '-x', lang,
                        os.path.join(ROOT, 'include', 'lsx_hip_depth.h')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_oracle_has_no_such_entry_and_the_engine_says_so(oracle_lib):
    prob, block, raw = fixtures.load_problem_npz(golden('falc_ca.npz'))
    e = Engine(prob, 1, lib=oracle_lib)
    e.set_columns(0, block)
    assert not oracle_lib.has_depth_rays
    with pytest.raises(NotImplementedError, match='lsx_hip_depth_rays'):
        e.depth_rays([1.0])
    e.close()


# what DESIGN.md 4.12 states for the kernel's instances: waves per SIMD by angles per pass, (linear, parabolic)
OCCUPANCY = {1: (3, 3), 2: (2, 2), 4: (2, 2)}


def test_the_kernels_use_no_scratch_and_have_the_stated_occupancy():
    """build/lsx_depth.ru.log, the compiler's resource report of the new unit"""
    path = os.path.join(CSRC, 'build', 'lsx_depth.ru.log')
    assert os.path.exists(path), 'build the HIP library first (make -C lightspinner_amd/csrc)'
    text = open(path).read()
    blocks = re.split(r'remark: [^\n]*Function Name: ', text)[1:]
    seen = {}
    for b in blocks:
        name = b.split()[0]
        m = re.search(r'k_depth_raysILi(\d+)ELb([01])E', name)
        assert m, name
        val = lambda key: int(re.search(re.escape(key) + r':? (\d+)', b).group(1))
        assert val('ScratchSize [bytes/lane]') == 0, name
        assert val('VGPRs Spill') == 0, name
        assert re.search(r'Dynamic Stack: False', b), name
        assert val('LDS Size [bytes/block]') == 1536, name          # the exponential's and the Voigt function's tables, nothing else
        seen[(int(m.group(1)), int(m.group(2)))] = val('Occupancy [waves/SIMD]')
    want = {(nm, par): occ[par] for nm, occ in OCCUPANCY.items() for par in (0, 1)}
    assert seen == want, seen
