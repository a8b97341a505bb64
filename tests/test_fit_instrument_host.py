"""The instrument of the field fit on the CPU (include/lsx_hip_fit_instrument.h): fit.Instrument and its constructors; lsxfit::smear and
the normal equations through it (lsx_fit_host_smear, lsx_fit_host_normal_inst of liblsx_fit_host.so, make fithost) against numpy in
longdouble; the identity against the entry without an instrument; an exact zero; drivers.fit_field_columns on a host backend recovering
a known field through a smearing, undersampling instrument; the stand-alone sanitizer program.
Bars: tests/fit_instrument_cases.py -- (M' + 2 Nspace + 2 width + 8) u x the absolute sum per entry of chi2, grad, hess; (width + 1) u
x the absolute sum for the smear alone."""
import math
import os
import subprocess

import numpy as np
import pytest

import fit_cases as fc
import fit_instrument_cases as ic
import stokes_cases as sc
import stokes_response_cases as rc
from lightspinner_amd import drivers, fit

U = sc.U
# the closed form of Instrument.gaussian against Gauss-Legendre quadrature of the same integrals in longdouble: the largest deviation of
# a row-normalised weight, relative to the row's largest weight, measured on this test's instruments (DESIGN.md "How the instrument is
# pinned"): 4.2e-15 (leggauss gives its nodes and weights in float64: that is the floor of the comparison).  The assertion is 10 x
# that: a tripwire against a regression of the formula, not a claim of accuracy.
GAUSS_MEASURED = 4.2e-15


@pytest.fixture(scope='module')
def host():
    return rc.HostLib()


@pytest.fixture(scope='module')
def fithost():
    return ic.FitInstHostLib()


def _grids():
    rng = np.random.default_rng(5)
    even = 500.0 + 0.002 * np.arange(44)
    uneven = 854.0 + np.cumsum(rng.uniform(0.5, 2.0, 65)) * 0.004
    return [even, uneven, even[:2], uneven[:3]]


def test_from_matrix_and_sampling():
    rng = np.random.default_rng(2)
    K = np.zeros((9, 20))
    for o in range(9):
        lo, n = int(rng.integers(0, 17)), int(rng.integers(1, 4))
        K[o, lo:lo + n] = rng.uniform(-1.0, 1.0, n)
    K[0, 0], K[8, 19], K[4] = 0.5, -0.25, 0.0              # a band at each end, an empty row
    dense = rng.uniform(-1.0, 1.0, (4, 7))
    for A in (K, dense, np.array([[2.0]])):
        inst = fit.Instrument.from_matrix(A)
        assert np.array_equal(inst.matrix(), A) and inst.nobs == A.shape[0] and 1 <= inst.width <= A.shape[1]
        assert np.all(inst.first >= 0) and np.all(inst.first + inst.width <= A.shape[1])
    assert fit.Instrument.from_matrix(dense).width == 7
    assert np.array_equal(fit.Instrument.identity(6).matrix(), np.eye(6)) and fit.Instrument.identity(6).width == 1
    for grid in _grids():
        pix = np.r_[grid[0], np.random.default_rng(3).uniform(grid[0], grid[-1], 40), grid[-1], grid[len(grid) // 2]]
        inst = fit.Instrument.sampling(grid, pix)
        assert inst.width == 2 and inst.nobs == pix.shape[0]
        eye = np.eye(grid.shape[0])
        assert np.array_equal(inst.matrix(), np.stack([np.interp(pix, grid, e) for e in eye], axis=1))
    with pytest.raises(ValueError):
        fit.Instrument([0, 3], np.ones((2, 2)), 4)          # reads past the window
    with pytest.raises(ValueError):
        fit.Instrument([0], [[np.nan]], 4)
    with pytest.raises(ValueError):
        fit.Instrument([0], np.ones((1, 5)), 4)


def _gauss_cases():
    out = []
    for grid in _grids()[:2]:
        h = ic.spacing(grid)
        for n, f in ((2 * grid.shape[0] // 3, 2.0), (30, 2.0), (15, 8.0), (11, 0.3), (2 * grid.shape[0] + 1, 1.0)):
            out.append((grid, ic.uniform_pixels(grid, n), f * h))
    return out


def _quadrature(grid, pix, fwhm, nsigma=4.0, order=40):
    """the raw weights by Gauss-Legendre quadrature per clipped interval, in longdouble, then row-normalised"""
    LD = np.longdouble
    xs, ws = (np.asarray(a, dtype=LD) for a in np.polynomial.legendre.leggauss(order))
    g = np.asarray(grid, dtype=LD)
    sigma = LD(fwhm) / (2 * np.sqrt(2 * np.log(LD(2))))
    K = np.zeros((len(pix), len(g)), dtype=LD)
    for o, c in enumerate(np.asarray(pix, dtype=LD)):
        # (the same integrals: the cut at nsigma sigma is the float64 number the constructor forms)
        s64 = float(fwhm) / (2.0 * math.sqrt(2.0 * math.log(2.0)))
        a, b = LD(max(float(g[0]), float(c) - nsigma * s64)), LD(min(float(g[-1]), float(c) + nsigma * s64))
        for j in range(len(g) - 1):
            lo, hi = max(g[j], a), min(g[j + 1], b)
            if hi <= lo:
                continue
            # (the integrand is smooth on an interval; split it at the centre's side so that order 40 resolves a narrow Gaussian)
            for l0, l1 in ((lo, min(max(c, lo), hi)), (min(max(c, lo), hi), hi)):
                if l1 <= l0:
                    continue
                lam = 0.5 * (l1 - l0) * xs + 0.5 * (l1 + l0)
                gl = np.exp(-0.5 * ((lam - c) / sigma) ** 2) / (sigma * np.sqrt(2 * LD(np.pi))) * (0.5 * (l1 - l0)) * ws
                hgt = g[j + 1] - g[j]
                K[o, j] += np.sum(gl * (g[j + 1] - lam) / hgt)
                K[o, j + 1] += np.sum(gl * (lam - g[j]) / hgt)
    return K / K.sum(axis=1, keepdims=True)


def test_gaussian():
    worst = 0.0
    for grid, pix, fwhm in _gauss_cases():
        inst = fit.Instrument.gaussian(grid, pix, fwhm)
        K = inst.matrix()
        assert np.max(np.abs(np.sum(np.asarray(K, dtype=np.longdouble), axis=1) - 1.0)) <= inst.width * U
        # a spectrum linear in wavelength is reproduced at every pixel whose +- nsigma sigma lies inside the grid: the hats reproduce
        # linear functions and the cut Gaussian is symmetric
        sigma = fwhm / (2.0 * np.sqrt(2.0 * np.log(2.0)))
        inner = (pix - 4.0 * sigma >= grid[0]) & (pix + 4.0 * sigma <= grid[-1])
        assert inner.any()
        lin = (np.asarray(K, dtype=np.longdouble) @ np.asarray(grid, dtype=np.longdouble))
        bar = (inst.width + 2) * U * (np.abs(K) @ np.abs(grid))
        assert np.all(np.abs(lin - pix)[inner] <= bar[inner]), np.max((np.abs(lin - pix) / bar)[inner])
        dev = float(np.max(np.abs(K - _quadrature(grid, pix, fwhm)) / np.max(K, axis=1, keepdims=True)))
        worst = max(worst, dev)
    print('Instrument.gaussian against quadrature: largest deviation / the row\'s largest weight %.3g' % worst)
    assert worst <= 10.0 * GAUSS_MEASURED
    grid = _grids()[0]
    for bad in (dict(grid=grid[::-1]), dict(grid=np.r_[grid[:3], grid[2:]]), dict(pixels=[grid[0] - 1e-9]), dict(pixels=[grid[-1] + 1e-9]),
                dict(fwhm=0.0), dict(fwhm=-1.0), dict(fwhm=np.nan), dict(pixels=[np.nan]), dict(grid=np.r_[grid[:-1], np.inf]),
                dict(fwhm=np.inf)):
        kw = dict(dict(grid=grid, pixels=grid[3:6], fwhm=0.004), **bad)
        with pytest.raises(ValueError):
            fit.Instrument.gaussian(kw['grid'], kw['pixels'], kw['fwhm'])
    for bad in (dict(grid=grid[::-1]), dict(pixels=[grid[0] - 1e-9]), dict(pixels=[np.nan])):
        kw = dict(dict(grid=grid, pixels=grid[3:6]), **bad)
        with pytest.raises(ValueError):
            fit.Instrument.sampling(kw['grid'], kw['pixels'])


def _setup(host, fithost, Ns, ncol, win, ms, nnode, wkind, given, pats, kind):
    prob, block, prof, J = sc.problem(Ns, ncol, vlos=True)
    fld = sc.field(Ns, ncol)
    la0, nla = win
    mus = fc.MUS[ms]
    be = ic.InstHostBackend(host, fithost, prob, block, prof, block.n, J, sc.PATTERN_SETS[pats], la0, nla)
    inst = ic.instrument_of(kind, ic.window_grid(prob, la0, nla))
    basis, base = fc.basis_of(Ns, nnode), fc.base_of(fld, nnode, given)
    truth = fc.nodes_of(fld, Ns, nnode, base)
    obs = fithost.smear(be.stokes(fithost.expand(Ns, nnode, basis, base, truth), mus), inst)
    return be, inst, mus, basis, base, truth, fc.off_truth(truth, nnode), obs


@pytest.mark.parametrize('Ns,ncol,win,ms,nnode,wkind,given,pats,kind', ic.CASES)
def test_normal_equations(host, fithost, Ns, ncol, win, ms, nnode, wkind, given, pats, kind):
    be, inst, mus, basis, base, truth, nodes, obs = _setup(host, fithost, Ns, ncol, win, ms, nnode, wkind, given, pats, kind)
    assert obs.shape == (ncol, 4, inst.nobs, len(mus))
    if kind in ('band', 'gaussian', 'sampling') and win[1] > 1:
        assert (inst.first == 0).any() and (inst.first == win[1] - inst.width).any()
    w = fc.weights_of(wkind, obs.shape)
    ne = be.fit_field_normal(mus, basis, nnode, nodes, obs, weight=w, base=base, instrument=inst)
    rf, S = be.response(ne.field, mus, nnode, fc.AMPS)
    assert ic.smear_excess(fithost.smear(S, inst), S, inst) <= 1.0
    val, bar = ic.yardstick(nnode, rf, S, obs, w, basis, inst)
    x = fc.inside(dict(chi2=ne.chi2, grad=ne.grad, hess=ne.hess), val, bar)
    sig = fc.grad_signal(val, bar)
    plain = fc.inside(dict(chi2=ne.chi2, grad=ne.grad, hess=ne.hess), *ic.yardstick(nnode, rf, S, obs, w, basis, inst, plain_residual=True))
    print('Ns %d, nla %d, %s: nobs %d, width %d, M\' %d, P %d: deviation / bar %s, largest |grad| / bar %.3g (with |r| for the residual: %s)'
          % (Ns, win[1], kind, inst.nobs, inst.width, 4 * inst.nobs * len(mus), sum(nnode), x, sig, plain))
    assert max(x.values()) <= 1.0 and sig >= fc.SIGNAL
    assert fc.same(ne.hess, np.swapaxes(ne.hess, 1, 2))
    assert fc.same(be.fit_field_chi2(mus, basis, nnode, nodes, obs, weight=w, base=base, instrument=inst)[0], ne.chi2)
    if w is not None:                     # a masked pixel's obs does not enter
        n2 = be.fit_field_normal(mus, basis, nnode, nodes, np.where(w > 0, obs, obs * 3.0 + 1.0), weight=w, base=base, instrument=inst)
        assert all(fc.same(getattr(n2, k), getattr(ne, k)) for k in ('chi2', 'grad', 'hess'))
    if kind == 'identity':                # today's entry, as numbers (0.0 + 1.0 x loses the sign of a zero)
        n0 = fc.HostBackend.fit_field_normal(be, mus, basis, nnode, nodes, obs, weight=w, base=base)
        assert all(np.array_equal(getattr(n0, k), getattr(ne, k)) for k in ('chi2', 'grad', 'hess'))
        n1 = be.fit_field_normal(mus, basis, nnode, nodes, obs, weight=w, base=base, instrument=None)
        assert all(fc.same(getattr(n0, k), getattr(n1, k)) for k in ('chi2', 'grad', 'hess'))


@pytest.mark.parametrize('kind', ['a', 'b'])
def test_an_exact_zero(host, fithost, kind):
    """obs made by the smear from the Stokes vector of the field expanded from the nodes: chi2 there is 0.0, grad all zeros"""
    (prob, block, prof, J), pats, fld, nnode, basis, truth, start = fc.recovery(13, 3, 2)
    la0, nla = fc.RECOVERY_WINDOW
    be = ic.InstHostBackend(host, fithost, prob, block, prof, block.n, J, pats, la0, nla)
    inst = ic.recovery_instrument(ic.window_grid(prob, la0, nla), kind)
    mus = fc.MUS[:2]
    obs = fithost.smear(be.stokes(fithost.expand(13, nnode, basis, None, truth), mus), inst)
    ne = be.fit_field_normal(mus, basis, nnode, truth, obs, weight=fc.recovery_weight(obs), instrument=inst)
    assert np.all(ne.chi2 == 0.0) and not np.any(ne.grad) and np.all(np.diagonal(ne.hess, axis1=1, axis2=2) > 0)
    assert np.all(be.fit_field_chi2(mus, basis, nnode, truth, obs, instrument=inst)[0] == 0.0)


@pytest.mark.parametrize('kind', ['a', 'b'])
@pytest.mark.parametrize('Ns,nn,mus', fc.RECOVERY_CASES + [(13, 2, 'three columns')])
def test_the_loop_recovers_a_known_field_through_an_instrument(host, fithost, Ns, nn, mus, kind):
    ncol = 3 if mus == 'three columns' else 1
    mus = np.array([1.0] if ncol == 3 else mus)
    (prob, block, prof, J), pats, fld, nnode, basis, truth, start = fc.recovery(Ns, ncol, nn)
    la0, nla = fc.RECOVERY_WINDOW
    be = ic.InstHostBackend(host, fithost, prob, block, prof, block.n, J, pats, la0, nla)
    inst = ic.recovery_instrument(ic.window_grid(prob, la0, nla), kind)
    assert inst.nobs == {'a': 30, 'b': 15}[kind] < nla
    obs = fithost.smear(be.stokes(np.stack(fld, axis=1), mus), inst)
    w = fc.recovery_weight(obs)
    r = drivers.fit_field_columns(be, obs, mus, basis, start, nnode, weight=w, amplitudes=fc.AMPS, instrument=inst, **fc.RECOVERY_LOOP)
    print('(%s) Ns %d, %d nodes, %d angles, %d columns: chi2 %s -> %s in %s iterations, node error %.3g'
          % (kind, Ns, nn, len(mus), ncol, r.history[0], r.chi2, r.iterations, np.max(np.abs(r.nodes - truth))))
    fc.check_recovery(r, truth)
    assert be.calls['normal'] == be.calls['step'] == len(r.history) - 1 and be.calls['chi2'] == len(r.history)


def test_the_sanitizer_program():
    """make fitinstsan: the smear and the normal equations through it on the smallest and the largest shape, a band at each end, under
    ASan and UBSan, stand-alone"""
    subprocess.check_call(['make', '-s', '-C', sc.CSRC, 'fitinstsan'])
    out = subprocess.run([os.path.join(sc.CSRC, 'lsx_fit_inst_san')], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and 'lsx_fit_inst_san: ok' in out.stdout and 'runtime error' not in out.stderr, out.stdout + out.stderr


def test_host_refusals(fithost):
    """lsx_fit_host_smear's rules are the instrument's (include/lsx_hip_fit_instrument.h)"""
    x, out = np.ones((1, 4, 2)), np.empty((1, 3, 2))
    ip = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    call = lambda nobs, width, first, weight: fithost.dll.lsx_fit_host_smear(4, 2, 1, nobs, width, None if first is None else ic._i(first),
                                                                             ic._p(weight), ic._p(x), ic._p(out))
    w = np.ones((3, 2))
    assert call(3, 2, ip([0, 1, 2]), w) == sc.LSX_OK and np.all(out == 2.0)
    for bad in ((0, 2, ip([0, 1, 2]), w), (3, 0, ip([0, 1, 2]), w), (3, 5, ip([0, 0, 0]), np.ones((3, 5))), (3, 2, ip([0, 1, 3]), w),
                (3, 2, ip([-1, 1, 2]), w), (3, 2, None, w), (3, 2, ip([0, 1, 2]), None), (3, 2, ip([0, 1, 2]), np.where(np.eye(3, 2) > 0, np.inf, w))):
        assert call(*bad) == sc.LSX_EINVAL, bad[:2]


def test_names_and_resources():
    """lsx_hip_fit_instrument.h declares three entries and the library exports exactly those under their prefix; lsx_hip_fit.h holds the
    struct and includes it; the compiler's report of the unit: one kernel, no scratch, no spilled vector register, no dynamic stack,
    no LDS (the weights come from the cache)"""
    import re
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, 'include', 'lsx_hip_fit_instrument.h')).read()
    declared = sorted(set(re.findall(r'\b(lsx_hip_\w+)\s*\(', re.sub(r'/\*.*?\*/', '', hdr, flags=re.S))))
    want = ['lsx_hip_instrument_apply', 'lsx_hip_instrument_fit_chi2', 'lsx_hip_instrument_fit_normal']
    assert declared == want
    fit_h = open(os.path.join(ROOT, 'include', 'lsx_hip_fit.h')).read()
    assert 'typedef struct lsx_fit_instrument' in fit_h and '#include "lsx_hip_fit_instrument.h"' in fit_h
    from lightspinner_amd import _capi
    assert not [n for n in _capi.REQUIRED_SYMBOLS if 'instrument' in n]                 # the common ABI is what it was
    so = os.path.join(sc.CSRC, 'liblsx_hip.so')
    log = os.path.join(sc.CSRC, 'build', 'lsx_fit_instrument.ru.log')
    if not (os.path.exists(so) and os.path.exists(log)):
        subprocess.check_call(['make', '-s', '-j', '8', '-C', sc.CSRC])
    syms = subprocess.run(['nm', '-D', '--defined-only', so], capture_output=True, text=True, check=True).stdout
    assert sorted(n for n in re.findall(r' T (\w+)', syms) if n.startswith('lsx_hip_instrument')) == want
    blocks = re.split(r'remark: Function Name: ', open(log).read())[1:]
    assert len(blocks) == 1 and 'k_fit_smear' in blocks[0].split()[0], [b.split()[0] for b in blocks]
    get = lambda key: re.search(re.escape(key) + r': (\S+)', blocks[0]).group(1)
    assert (get('ScratchSize [bytes/lane]'), get('VGPRs Spill'), get('Dynamic Stack'), get('LDS Size [bytes/block]')) == ('0', '0', 'False', '0')
