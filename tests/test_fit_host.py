"""The field fit on the CPU (include/lsx_hip_fit.h): lsx_fit_dev.h compiled into liblsx_fit_host.so (make fithost), fed with the host
library's response and Stokes window (tests/stokes_response_cases.py), against numpy in longdouble; the damped step by its backward
error; drivers.fit_field_columns on a host backend recovering a known field; the stand-alone sanitizer program; the exported names.
Bars: tests/fit_cases.py -- (M + 2 Nspace + 8) u x the absolute sum per entry of chi2, grad, hess; P (3 P + 1) u for the normwise
backward error of the Cholesky solve (Higham, Accuracy and Stability, Thm 10.4 with the norm factor)."""
import os
import re
import subprocess

import numpy as np
import pytest

import fit_cases as fc
import stokes_cases as sc
import stokes_response_cases as rc
from conftest import ROOT
from lightspinner_amd import drivers, fit


@pytest.fixture(scope='module')
def host():
    return rc.HostLib()


@pytest.fixture(scope='module')
def fithost():
    return fc.FitHostLib()


def test_hat_basis():
    for Ns, n in ((3, 2), (5, 3), (13, 8), (13, 1), (82, 5)):
        b = fit.hat_basis(np.arange(Ns), np.linspace(0, Ns - 1, n) if n > 1 else [3.0])
        assert b.shape == (n, Ns) and np.all(b >= 0) and np.max(np.abs(b.sum(axis=0) - 1.0)) <= 4 * sc.U
    b = fit.hat_basis([0.0, 1.0, 2.0, 3.0, 4.0], [1.0, 3.0])
    assert np.array_equal(b, [[1, 1, 0.5, 0, 0], [0, 0, 0.5, 1, 1]])           # constant outside the nodes
    h = fit.hat_basis(-np.arange(5.0) ** 2, [-16.0, -4.0, 0.0])               # any monotonic coordinate
    assert np.array_equal(h[:, 2], [0, 1, 0]) and np.array_equal(h[:, 4], [1, 0, 0])
    for bad in ([], [1.0, 1.0], [2.0, 1.0], [np.nan]):
        with pytest.raises(ValueError):
            fit.hat_basis(np.arange(4), bad)
    bas, nn = fit.stack_basis(B=b, chiB=np.ones(5))
    assert bas.shape == (3, 5) and nn == (2, 0, 1)


# Ns, ncol, window, angles, nnode, weights, base given, pattern set: every value of the issue's lists occurs
CASES = [(3, 1, (0, 1), [0], (1, 0, 0), None, False, 'triplet'),
         (3, 1, (7, 1), [0, 1, 2], (0, 2, 0), 'given', True, 'triplet'),
         (5, 3, (0, 63), [0], (2, 2, 2), 'masked', False, 'largest'),
         (5, 3, (7, 64), [0, 1, 2], (3, 3, 3), None, True, 'blend'),
         (5, 1, (7, 63), [1], (2, 2, 2), 'given', False, 'all'),
         (5, 1, (0, 64), [0], (0, 2, 0), None, False, 'blend'),
         (13, 1, (0, 65), [0, 1, 2], (3, 3, 3), 'given', False, 'largest'),
         (13, 1, (7, 65), [0], (8, 8, 8), 'masked', True, 'triplet'),
         (13, 1, (0, 130), [0, 1, 2], (8, 8, 8), 'given', False, 'triplet'),
         (13, 3, (7, 130), [0], (2, 2, 2), None, False, 'blend')]


@pytest.mark.parametrize('Ns,ncol,win,ms,nnode,wkind,given,pats', CASES)
def test_normal_equations(host, fithost, Ns, ncol, win, ms, nnode, wkind, given, pats):
    prob, block, prof, J = sc.problem(Ns, ncol, vlos=True)
    fld = sc.field(Ns, ncol)
    la0, nla = win
    mus = fc.MUS[ms]
    be = fc.HostBackend(host, fithost, prob, block, prof, block.n, J, sc.PATTERN_SETS[pats], la0, nla)
    basis, base = fc.basis_of(Ns, nnode), fc.base_of(fld, nnode, given)
    truth = fc.nodes_of(fld, Ns, nnode, base)
    _, obs = be.response(fithost.expand(Ns, nnode, basis, base, truth), mus, nnode, fc.AMPS)
    nodes = fc.off_truth(truth, nnode)
    w = fc.weights_of(wkind, obs.shape)
    ne = be.fit_field_normal(mus, basis, nnode, nodes, obs, weight=w, base=base)
    assert np.array_equal(ne.field, fithost.expand(Ns, nnode, basis, base, nodes))
    for p, n in enumerate(nnode):
        if n == 0:
            assert np.array_equal(ne.field[:, p], fld[p])
    rf, S = be.response(ne.field, mus, nnode, fc.AMPS)
    val, bar = fc.yardstick(nnode, rf, S, obs, w, basis)
    x = fc.inside(dict(chi2=ne.chi2, grad=ne.grad, hess=ne.hess), val, bar)
    sig = fc.grad_signal(val, bar)
    print('Ns %d, M %d, P %d: deviation / bar %s, largest |grad| / bar %.3g' % (Ns, 4 * nla * len(mus), sum(nnode), x, sig))
    assert max(x.values()) <= 1.0 and sig >= fc.SIGNAL
    assert fc.same(ne.hess, np.swapaxes(ne.hess, 1, 2))
    assert fc.same(be.fit_field_chi2(mus, basis, nnode, nodes, obs, weight=w, base=base)[0], ne.chi2)
    if w is not None:                     # a masked point's obs does not enter
        o2 = np.where(w > 0, obs, obs * 3.0 + 1.0)
        n2 = be.fit_field_normal(mus, basis, nnode, nodes, o2, weight=w, base=base)
        assert all(fc.same(getattr(n2, k), getattr(ne, k)) for k in ('chi2', 'grad', 'hess'))


def _systems(host, fithost, nnode, Ns=13):
    prob, block, prof, J = sc.problem(Ns, 1, vlos=True)
    fld = sc.field(Ns, 1)
    be = fc.HostBackend(host, fithost, prob, block, prof, block.n, J, sc.PATTERN_SETS['blend'], *fc.RECOVERY_WINDOW)
    basis = fc.basis_of(Ns, nnode)
    base = fc.base_of(fld, nnode, False)
    truth = fc.nodes_of(fld, Ns, nnode, base)
    _, obs = be.response(fithost.expand(Ns, nnode, basis, base, truth), fc.MUS[:1], nnode, fc.AMPS)
    nodes = fc.off_truth(truth, nnode)
    return be.fit_field_normal(fc.MUS[:1], basis, nnode, nodes, obs, weight=fc.recovery_weight(obs), base=base), nodes


@pytest.mark.parametrize('nnode', fc.NNODES)
def test_step(host, fithost, nnode):
    """the systems are the fit's own, P = 1, 2, 6, 9, 24: unclamped, then with an active bound; singular and NaN systems"""
    ne, nodes = _systems(host, fithost, nnode)
    P = sum(nnode)
    H, g = ne.hess[0], ne.grad[0]
    for lam in (1e-2, 1e-6 if P < 24 else 1e-3, 10.0):
        trial, pred, st, delta = fithost.step(H, g, lam, nodes)
        assert st[0] == 0
        be_, tr_ok, pr = fc.step_checks(P, H, g, lam, nodes[0], -np.inf, np.inf, trial[0], pred[0], delta[0])
        assert be_ <= 1.0 and tr_ok and pr <= 1.0, (lam, be_, tr_ok, pr)
        assert pred[0] > 0
        lo, hi = nodes[0] - 0.25 * np.abs(delta[0]), nodes[0] + 0.5 * np.abs(delta[0])          # every bound is active
        t2, p2, s2, d2 = fithost.step(H, g, lam, nodes, lo, hi)
        assert s2[0] == 0 and np.array_equal(d2, delta) and not np.array_equal(t2, trial)
        be_, tr_ok, pr = fc.step_checks(P, H, g, lam, nodes[0], lo, hi, t2[0], p2[0], d2[0])
        assert tr_ok and pr <= 1.0 and np.all((t2[0] >= lo) & (t2[0] <= hi))
    for bad in ('zero', 'nan', 'negative'):
        Hb = H.copy()
        if bad == 'zero':
            Hb[-1, :] = Hb[:, -1] = 0.0
        elif bad == 'nan':
            Hb[0, 0] = np.nan
        else:
            Hb[0, 0] = -Hb[0, 0]
        t, p, s, _ = fithost.step(np.stack([H, Hb]), np.stack([g, g]), 1e-2, np.stack([nodes[0], nodes[0]]))
        assert list(s) == [0, 1] and p[1] == 0.0 and np.array_equal(t[1], nodes[0]) and np.all(np.isfinite(t[0]))


@pytest.mark.parametrize('Ns,nn,mus', fc.RECOVERY_CASES + [(13, 2, 'three columns')])
def test_the_loop_recovers_a_known_field(host, fithost, Ns, nn, mus):
    ncol = 3 if mus == 'three columns' else 1
    mus = np.array([1.0] if ncol == 3 else mus)
    (prob, block, prof, J), pats, fld, nnode, basis, truth, start = fc.recovery(Ns, ncol, nn)
    be = fc.HostBackend(host, fithost, prob, block, prof, block.n, J, pats, *fc.RECOVERY_WINDOW)
    _, obs = be.response(np.stack(fld, axis=1), mus, nnode, fc.AMPS)
    w = fc.recovery_weight(obs)
    seen = []
    r = drivers.fit_field_columns(be, obs, mus, basis, start, nnode, weight=w, amplitudes=fc.AMPS, log=seen.append, **fc.RECOVERY_LOOP)
    print('Ns %d, %d nodes, %d angles, %d columns: chi2 %s -> %s in %s iterations, node error %.3g, lambda %s'
          % (Ns, nn, len(mus), ncol, r.history[0], r.chi2, r.iterations, np.max(np.abs(r.nodes - truth)), r.lam))
    fc.check_recovery(r, truth)
    assert np.array_equal(r.field, fithost.expand(Ns, nnode, basis, None, r.nodes)) and r.nnode == nnode
    assert be.calls['normal'] == be.calls['step'] == len(r.history) - 1 == len(seen) and be.calls['chi2'] == len(r.history)
    if ncol == 3:
        # a done column is not moved by the others' iterations
        for c in range(3):
            n_c = int(r.iterations[c])
            assert np.all(r.history[n_c:, c] == r.history[n_c, c])


def test_the_loop_freezes_done_columns_and_reports_the_ceiling():
    """a scripted backend: column 0 settles at once, column 1 never improves (lambda climbs to its ceiling), column 2 keeps
    improving to max_iter; the loop only compares and scales"""
    class Scripted:
        def __init__(self):
            self.asked = []

        def fit_field_chi2(self, mus, basis, nnode, nodes, obs, weight=None, base=None):
            x = np.asarray(nodes)[:, 0]
            self.asked.append(x.copy())
            return np.array([1.0 - 1e-14 * x[0], 2.0 + np.abs(x[1]), 4.0 * 0.5 ** x[2]]), np.zeros((3, 3, 2))

        def fit_field_normal(self, mus, basis, nnode, nodes, obs, weight=None, base=None, amplitudes=None):
            return fit.FieldNormal(None, np.ones((3, 1)), np.ones((3, 1, 1)), None)

        def fit_field_step(self, hess, grad, lam, nodes, lo=None, hi=None):
            return np.asarray(nodes) + 1.0, np.ones(3), np.zeros(3, dtype=np.int32)

    be = Scripted()
    r = drivers.fit_field_columns(be, None, [1.0], np.ones((1, 2)), np.zeros((3, 1)), (1, 0, 0), lambda0=1.0, lambda_max=1e3, max_iter=6)
    assert list(r.status) == [fit.CONVERGED, fit.LAMBDA_CEILING, fit.MAX_ITER] and list(r.iterations) == [1, 4, 6]
    assert r.nodes[0, 0] == 1.0 and r.nodes[1, 0] == 0.0 and r.nodes[2, 0] == 6.0
    assert r.lam[1] == 1e4 and abs(r.lam[2] / 1e-6 - 1.0) < 1e-12 and r.history.shape == (7, 3)
    for a in be.asked[2:]:
        assert a[0] == 1.0                   # the frozen column is asked about its own nodes
    assert np.array_equal(r.parameter('B'), r.nodes) and r.parameter('chiB').shape == (3, 0)


def test_the_sanitizer_program():
    """make fitsan: the normal equations and the step on the smallest and the largest shape under ASan and UBSan, stand-alone"""
    subprocess.check_call(['make', '-s', '-C', sc.CSRC, 'fitsan'])
    out = subprocess.run([os.path.join(sc.CSRC, 'lsx_fit_san')], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and 'lsx_fit_san: ok' in out.stdout and 'runtime error' not in out.stderr, out.stdout + out.stderr


def test_names_and_resources():
    """the header declares four entries, none of the Stokes pass's or the response's names; the library exports exactly those with the
    fit's prefix; the compiler's report of the unit: no scratch, no spilled vector register, no dynamic stack"""
    hdr = open(os.path.join(ROOT, 'include', 'lsx_hip_fit.h')).read()
    declared = sorted(set(re.findall(r'\b(lsx_hip_\w+)\s*\(', re.sub(r'/\*.*?\*/', '', hdr, flags=re.S))))
    want = ['lsx_hip_fit_field_chi2', 'lsx_hip_fit_field_normal', 'lsx_hip_fit_field_step', 'lsx_hip_fit_field_work_cap']
    assert declared == want
    assert not [n for n in declared if n.startswith('lsx_hip_stokes') or n.startswith('lsx_hip_response_stokes')]
    assert '#include "lsx_hip_fit.h"' in open(os.path.join(ROOT, 'include', 'lsx_hip.h')).read()
    from lightspinner_amd import _capi
    assert not [n for n in _capi.REQUIRED_SYMBOLS if 'fit_field' in n]
    so = os.path.join(sc.CSRC, 'liblsx_hip.so')
    log = os.path.join(sc.CSRC, 'build', 'lsx_fit.ru.log')
    if not (os.path.exists(so) and os.path.exists(log)):
        subprocess.check_call(['make', '-s', '-j', '8', '-C', sc.CSRC])
    syms = subprocess.run(['nm', '-D', '--defined-only', so], capture_output=True, text=True, check=True).stdout
    assert sorted(n for n in re.findall(r' T (\w+)', syms) if n.startswith('lsx_hip_fit')) == want
    blocks = re.split(r'remark: Function Name: ', open(log).read())[1:]
    names = [b.split()[0] for b in blocks]
    assert len(names) == 3 and all(any(k in n for n in names) for k in ('k_fit_jac', 'k_fit_reduce', 'k_fit_step')), names
    for b in blocks:
        get = lambda key: re.search(re.escape(key) + r': (\S+)', b).group(1)
        assert (get('ScratchSize [bytes/lane]'), get('VGPRs Spill'), get('Dynamic Stack')) == ('0', '0', 'False'), b.split()[0]
