"""Emergent spectra at arbitrary wavelengths (include/lsx_hip_spectrum.h, lsx_hip_spectrum): what can be checked without a GPU.

The reference pin: tests/golden/spectrum_falc.npz holds what the unmodified reference computes on
compute_wavelength_grid(extraWavelengths=w) from committed states (tests/golden/make_spectrum_golden.py).  The checker of the GPU
tests (tests/spectrum_cases.py: a zero-weight oracle context on the re-gridded problem) is held against it here."""
import os
import re
import subprocess

import numpy as np
import pytest

import rays_cases as rc
import spectrum_cases as sc
from conftest import ROOT, golden
from lightspinner_amd import _capi, fixtures
from lightspinner_amd.problem import Engine

CSRC = os.path.join(ROOT, 'lightspinner_amd', 'csrc')


@pytest.mark.parametrize('case', sc.CASES)
def test_the_oracle_on_the_regridded_problem_is_the_reference(oracle_lib, case):
    """bar: rays_cases.GOLDEN_BAR (1e-11 CaII, 3e-11 Ca + H).  Measured over the seven angles: ca_vlos 2.2e-13, cah 3.9e-13"""
    prob, block, prof, n, J, mus, f = sc.fixture_case(case)
    nla = f['w'].shape[0]
    assert f['I'].shape == (nla, mus.shape[0]) and f['bg_chi'].shape == f['bg_eta'].shape == (nla, prob.Nspace)
    assert f['alpha'].shape == (prob.Ntrans - prob.Nlines, nla) and np.all(f['I'] > 0)
    mine = sc.oracle_spectrum(oracle_lib, prob, block, prof, mus, n, J, f['w'], f['alpha'], (f['bg_chi'][None], f['bg_eta'][None]))[0]
    d = rc.relmax(mine, f['I'])
    print('%s: the oracle on the re-gridded problem against the reference at %d extra wavelengths: %.2e (bar %.0e)'
          % (case, nla, d, rc.GOLDEN_BAR[case]))
    assert d <= rc.GOLDEN_BAR[case]


@pytest.mark.parametrize('case', sc.CASES)
def test_the_windows_of_regrid_are_the_reference_windows(case):
    prob, block, prof, n, J, mus, f = sc.fixture_case(case)
    wu = np.union1d(prob.wavelength, f['w'])
    win = sc.windows(prob, wu)
    assert [a for a, _ in win] == list(f['Nblue']) and [b for _, b in win] == list(f['Nlambda'])
    p2 = sc.regrid(prob, block, J, f['w'], f['alpha'])[0]
    assert all(np.array_equal(np.flatnonzero(p2.active[kr]), np.arange(t.Nblue, t.Nblue + t.Nlambda)) for kr, t in enumerate(p2.trans))
    assert any(b2 > t.Nlambda for (_, b2), t in zip(win, prob.trans))          # some windows did grow


def own_alpha(prob):
    out = []
    for t in prob.trans:
        if not t.is_line:
            a = np.zeros(prob.Nspect)
            a[t.Nblue:t.Nblue + t.Nlambda] = t.alpha
            out.append(a)
    return np.stack(out) if out else None


def test_on_the_own_grid_the_regridded_problem_is_the_problem(oracle_lib):
    prob, block, prof, n, J, mus, _ = rc.golden_case('ca_vlos')
    p2, b2, J2, rows = sc.regrid(prob, block, J, prob.wavelength, own_alpha(prob))
    assert np.array_equal(p2.wavelength, prob.wavelength) and np.array_equal(rows, np.arange(prob.Nspect))
    assert np.array_equal(J2, J) and np.array_equal(b2.bg_chi, block.bg_chi) and np.array_equal(p2.active, prob.active)
    a = sc.oracle_spectrum(oracle_lib, prob, block, prof, mus[:3], n, J, prob.wavelength, own_alpha(prob))
    b = rc.oracle_rays(oracle_lib, prob, block, prof, mus[:3], n, J)
    assert np.array_equal(a, b)
    # a single wavelength gives the bits it has inside a window
    w = np.linspace(854.1, 854.3, 9)
    al = sc.interp_alpha(prob, w)
    many = sc.oracle_spectrum(oracle_lib, prob, block, prof, mus[:3], n, J, w, al)
    one = sc.oracle_spectrum(oracle_lib, prob, block, prof, mus[:3], n, J, w[4:5], al[:, 4:5])
    assert np.array_equal(one[:, 0], many[:, 4])


def test_the_bracket_rule_against_np_interp():
    """(l, t) at the first, an interior and the last grid point (exact), below and above the grid (held constant), and in a bracket
    that spans a tile boundary of the device's streams (64 / Nrays wavelengths a tile): inside 4u of np.interp on the case's own J.
    (Both forms round three times on positive data; np.interp's y0 + (x - x0) slope also carries u |y1 - y0|, so the figure over ALL
    brackets of the grid is printed, not held to 4u: J changes by orders of magnitude across some of them.)"""
    prob, _, _, _, J, _, _ = rc.golden_case('ca_vlos')
    lam, X = prob.wavelength, J[0]
    N, L = lam.shape[0], 64 // prob.Nrays
    interp = lambda w: np.stack([np.interp(w, lam, X[:, k]) for k in range(X.shape[1])], axis=1)
    l, t = sc.bracket(lam, [lam[0], lam[100], lam[-1]])
    assert list(l) == [0, 100, N - 2] and list(t) == [0.0, 0.0, 1.0]
    assert np.array_equal(sc.interp_rule(lam, X, [lam[0], lam[100], lam[-1]]), X[[0, 100, N - 1]])
    assert np.array_equal(interp([lam[0], lam[100], lam[-1]]), X[[0, 100, N - 1]])
    l, t = sc.bracket(lam, [0.5 * lam[0], 2.0 * lam[-1]])
    assert list(l) == [0, N - 2] and list(t) == [0.0, 1.0]
    assert np.array_equal(sc.interp_rule(lam, X, [0.5 * lam[0], 2.0 * lam[-1]]), X[[0, N - 1]])
    assert np.array_equal(interp([0.5 * lam[0], 2.0 * lam[-1]]), X[[0, N - 1]])
    w = lam[L - 1] + np.array([0.3, 0.5, 0.9]) * (lam[L] - lam[L - 1])          # grid points L - 1 and L lie in two tiles
    l, t = sc.bracket(lam, w)
    assert np.all(l == L - 1) and np.all((0 < t) & (t < 1))
    d = float(np.max(np.abs(sc.interp_rule(lam, X, w) - interp(w)) / np.abs(interp(w))))
    print('the rule against np.interp across a tile boundary: %.2e (4u = %.2e)' % (d, 4 * sc.U))
    assert d <= 4 * sc.U
    w = np.sort(np.concatenate([0.5 * (lam[1:] + lam[:-1]), lam[:-1] + 0.9 * np.diff(lam)]))
    l, t = sc.bracket(lam, w)
    assert np.all((0 <= t) & (t <= 1)) and np.all((lam[l] <= w) & (w <= lam[l + 1]))
    print('... in every bracket of the grid: %.2e' % float(np.max(np.abs(sc.interp_rule(lam, X, w) - interp(w)) / np.abs(interp(w)))))
    one = sc.bracket(lam[:1], [3.0, 900.0])
    assert list(one[0]) == [0, 0] and list(one[1]) == [0.0, 0.0]


def test_the_entries_are_exported_and_declared_in_a_header_of_their_own():
    lib = os.path.join(CSRC, 'liblsx_hip.so')
    assert os.path.exists(lib), 'build the HIP library first (make -C lightspinner_amd/csrc)'
    syms = subprocess.run(['nm', '-D', '--defined-only', lib], capture_output=True, text=True, check=True).stdout
    text = open(os.path.join(ROOT, 'include', 'lsx_hip_spectrum.h')).read()
    declared = set(re.findall(r'\b(lsx_hip_[a-z0-9_]+)\s*\(', text))
    assert declared == {'lsx_hip_spectrum', 'lsx_hip_spectrum_work_cap'}
    exported = set(re.findall(r'\bT (lsx_hip_spectrum[a-z0-9_]*)\b', syms))
    assert exported == declared
    assert '#include "lsx_hip_spectrum.h"' in open(os.path.join(ROOT, 'include', 'lsx_hip.h')).read()
    assert not any(s.startswith('lsx_hip_spectrum') for s in _capi.REQUIRED_SYMBOLS)        # the common ABI is what it was
    assert 'lsx_hip_spectrum' not in open(os.path.join(ROOT, 'include', 'lsx.h')).read()


@pytest.mark.parametrize('compiler,std', [('gcc', 'c99'), ('g++', 'c++11')])
def test_the_header_compiles_alone(compiler, std):
    lang = 'c' if compiler == 'gcc' else 'c++'
    r = subprocess.run([compiler, '-std=' + std, '-Wall', '-Wextra', '-pedantic', '-Werror', '-fsyntax-only', '-x', lang,
                        os.path.join(ROOT, 'include', 'lsx_hip_spectrum.h')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_oracle_has_no_such_entry_and_the_engine_says_so(oracle_lib):
    prob, block, raw = fixtures.load_problem_npz(golden('falc_ca.npz'))
    e = Engine(prob, 1, lib=oracle_lib)
    e.set_columns(0, block)
    assert not oracle_lib.has_spectrum
    with pytest.raises(NotImplementedError, match='lsx_hip_spectrum'):
        e.emergent_spectrum([1.0], [500.0], alpha=np.zeros((prob.Ntrans - prob.Nlines, 1)))
    e.close()


def test_the_kernels_use_no_scratch():
    """build/lsx_spectrum.ru.log, the compiler's resource report of the new unit: every kernel without scratch, without a spilled
    vector register and without a dynamic stack"""
    path = os.path.join(CSRC, 'build', 'lsx_spectrum.ru.log')
    if not os.path.exists(path):
        pytest.skip('no resource report: the library was not built by this tree\'s Makefile')
    blocks = re.split(r'remark: [^\n]*Function Name: ', open(path).read())[1:]
    names = [b.split()[0] for b in blocks]
    assert sum('k_spectrumILi' in x for x in names) == 7 and any('k_spectrum_transpose' in x for x in names), names
    for b, name in zip(blocks, names):
        val = lambda key: int(re.search(re.escape(key) + r':? (\d+)', b).group(1))
        assert val('ScratchSize [bytes/lane]') == 0, name
        assert val('VGPRs Spill') == 0, name
        assert re.search(r'Dynamic Stack: False', b), name
