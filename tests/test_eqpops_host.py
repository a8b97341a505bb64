"""The LTE populations without a GPU (include/lsx_hip_eqpops.h): a numpy restatement of the reference's lte_pops against the
committed fixtures bit for bit; the formulas of lsx_eqpops_dev.h compiled for the CPU (liblsx_eqpops_host.so) against that
restatement and the fixtures inside the bar of tests/eqpops_cases.py; made-up atoms; the stand-alone sanitizer program; and every
LSX_EINVAL, none of which needs a device."""
import os
import subprocess

import numpy as np
import pytest

import eqpops_cases as ec
from setup_cases import Ledger


@pytest.fixture(scope='module')
def host():
    return ec.HostLib()


CASES = {c.name: c for c in ec.all_cases()}


@pytest.mark.parametrize('name', sorted(CASES))
def test_numpy_restatement_is_the_reference_bit_for_bit(name):
    """FALC, the second atmosphere, the 164 perturbed points and the five atoms on the edge atmosphere: hGround and nStar"""
    c = CASES[name]
    r = ec.numpy_result(c)
    for a in range(len(c.atoms)):
        if c.ref[a] is not None:
            assert np.array_equal(r.nStar[a], c.ref[a]), (name, c.atoms[a].name)
    assert np.array_equal(r.nStar[0][:, 0], c.hGround), name


def test_the_perturbation_moves_hground_far_beyond_the_bar():
    """a value taken from the base column by mistake fails: hGround[k] moves by 2.3e-7 ... 7.2e-2 relative, the bar is below 1e-13"""
    c, base = CASES['rf_164'], CASES['falc_atm0']
    move = np.abs(c.hGround / base.hGround - 1.0)
    assert 1e-7 < move.min() and move.max() < 0.1
    assert ec.bar(c.atoms[0], c.T)[0].max() < 1e-13 < 1e-6 * move.min()


@pytest.mark.parametrize('name', sorted(CASES))
def test_host_build_against_the_fixtures_and_the_restatement(host, name):
    c = CASES[name]
    r = host.of_case(c)
    led = Ledger('host ' + name)
    ec.check_case(led, c, r)
    ref = ec.numpy_result(c)
    for a, atom in enumerate(c.atoms):
        ec.check(led, 'vs numpy', r.nStar[a], ref.nStar[a], atom, c.T)
    assert np.array_equal(r.nTotal, ref.nTotal)
    led.report()


def test_made_up_atoms(host):
    toys = ec.toy_atoms()
    T, ne, nH = ec.toy_atmosphere()
    led = Ledger('host toys')
    names = list(toys)
    atoms, ab = [toys[n][0] for n in names], [toys[n][1] for n in names]
    rc, r = host.eq_pops(atoms, ab, T, ne, nH)
    assert rc == 0, host.error()
    for a, n in enumerate(names):
        want = ec.lte_numpy(atoms[a], T, ne, ab[a] * nH)
        ec.check(led, n, r.nStar[a], np.moveaxis(want, 0, 1), atoms[a], T)
        assert np.array_equal(r.nTotal[:, a], ab[a] * nH)
        # an atom alone gives what it gives among the others
        rc1, r1 = host.eq_pops([atoms[a]], [ab[a]], T, ne, nH, want_nTotal=False)
        assert rc1 == 0 and r1.nTotal is None and np.array_equal(r1.nStar[0], r.nStar[a]), n
    assert np.array_equal(r.nStar[names.index('one')][:, 0], nH)                 # one level: nStar = nTotal exactly
    assert np.all(r.nStar[names.index('absent')] == 0.0)                          # zero abundance
    st = r.nStar[names.index('stages')]
    assert np.all(st > 0.0) and np.allclose(st.sum(axis=1), ab[names.index('stages')] * nH, rtol=1e-13)
    led.report()


def test_formulas_under_asan_ubsan():
    """one to five atoms, atoms of 1, 2 and 12 levels, dZ 0 ... 3, 400 K and 1e6 K, the refusals: in a stand-alone program"""
    subprocess.check_call(['make', '-s', '-C', ec.CSRC, 'eqpopssan'])
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:halt_on_error=1', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')
    out = subprocess.run([os.path.join(ec.CSRC, 'lsx_eqpops_san')], capture_output=True, text=True, timeout=600, env=env)
    tail = out.stdout[-1500:] + '\n' + out.stderr[-3000:]
    assert out.returncode == 0, tail
    assert 'EQPOPS SANITIZED RUN COMPLETE' in out.stdout, tail


def test_argument_checks(host):
    from lightspinner_amd.eqpops import atoms_to_c
    c = CASES['falc_atm0']
    T, ne, nH = c.T, c.ne, c.nH
    ok = lambda atoms, ab, *arrs, **kw: host.eq_pops(atoms, ab, *arrs, **kw)[0]
    assert ok(c.atoms, c.ab, T, ne, nH) == 0
    for bad in (0.0, -1.0, np.nan, np.inf, -np.inf):
        for which in range(3):
            arrs = [T.copy(), ne.copy(), nH.copy()]
            arrs[which][0, 40] = bad
            want = 0 if (which == 2 and bad == 0.0) else ec.EINVAL            # nHTot = 0 is allowed
            assert ok(c.atoms, c.ab, *arrs) == want, (bad, which)
            if want:
                assert 'depth 40' in host.error()

    def atom(**kw):
        a = c.atoms[1]
        d = dict(E_SI=a.E_SI.copy(), g=a.g.copy(), stage=a.stage.copy())
        for k, (i, v) in kw.items():
            d[k][i] = v
        return ec.Atom(d['E_SI'], d['g'], d['stage'])
    for bad_atom in (atom(g=(2, 0.0)), atom(g=(0, -2.0)), atom(g=(3, np.nan)), atom(E_SI=(4, np.inf)), atom(E_SI=(0, np.nan)),
                     atom(stage=(5, 0))):
        assert ok([c.atoms[0], bad_atom], c.ab, T, ne, nH) == ec.EINVAL
        assert 'atom 1' in host.error()
    for bad_ab in (-1e-6, np.nan, np.inf):
        assert ok(c.atoms, [1.0, bad_ab], T, ne, nH) == ec.EINVAL and 'abundance' in host.error()
    # counts and null pointers, straight at the entry
    carr, nlev, _keep = atoms_to_c(c.atoms, c.ab)
    nStar, nTot = np.zeros((1, sum(nlev), 82)), np.zeros((1, 2, 82))
    assert host.raw(82, 2, carr, 1, T, ne, nH, nStar, nTot) == 0
    assert host.raw(82, 0, carr, 1, T, ne, nH, nStar, nTot) == ec.EINVAL
    assert host.raw(82, -1, carr, 1, T, ne, nH, nStar, nTot) == ec.EINVAL
    assert host.raw(82, 2, None, 1, T, ne, nH, nStar, nTot) == ec.EINVAL
    assert host.raw(82, 2, carr, 0, T, ne, nH, nStar, nTot) == ec.EINVAL and 'ncol' in host.error()
    for hole in range(4):
        arrs = [T, ne, nH, nStar]
        arrs[hole] = None
        assert host.raw(82, 2, carr, 1, *arrs, nTot) == ec.EINVAL
    carr[1].Nlevel = 0
    assert host.raw(82, 2, carr, 1, T, ne, nH, nStar, nTot) == ec.EINVAL and 'Nlevel' in host.error()
    carr[1].Nlevel = 6
    carr[1].levels = None
    assert host.raw(82, 2, carr, 1, T, ne, nH, nStar, nTot) == ec.EINVAL
