"""What the depth-scale tests share (tests/test_scales_host.py, tests/test_scales.py): the fixture of
tests/golden/make_scales_golden.py, the tables (those of the background fixture), and the bar.

The bar, entry by entry, with the numbers of tests/background_cases.py and no others:
    |x - ref| <= BASE s + K_ENVELOPE |ref(+1) - ref(-1)|
where ref(+-1) is the REFERENCE with every exp / log / log10 of witt's namespace moved by one unit in the last place, s = |ref|
for cmass, tau_ref and chi_ref, and s = |ref| + |ref[0]| for a shifted height (ref[0] = -hTau1 exactly, and heights pass through 0,
where a relative bar means nothing).  A bound above VACUOUS s anywhere fails the check.  No entry is skipped.  The geometric scale's
height is its input, bit for bit."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from conftest import ROOT, golden

from background_cases import BASE, K_ENVELOPE, VACUOUS, CSRC, tables  # noqa: F401

from lightspinner_amd import _capi

GEO, CM, TAU = 0, 1, 2
QUANTITIES = ('height', 'cmass', 'tau_ref', 'chi_c')


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(golden('scales_falc.npz')))


def cases():
    return [str(n) for n in fixture()['cases']]


class Case:
    def __init__(self, name):
        d = fixture()
        self.name, self.scale = name, int(d[name + '_scale'])
        self.ds, self.T, self.nH, self.ne = (d['%s_%s' % (name, k)] for k in ('depth_scale', 'temperature', 'nHTot', 'ne'))
        self.ref = {q: d['%s_%s' % (name, q)] for q in QUANTITIES}      # [3][N]: shift 0, +1, -1
        self.N = self.ds.shape[0]


def gravity():
    return 10 ** float(fixture()['logG'])


def inside(x, ref3, what, height_shifted=False):
    """asserts the bar for one quantity of one column; ref3 [3][N]; -> the largest deviation as a fraction of the bound"""
    x, ref3 = np.asarray(x, dtype=np.float64), np.asarray(ref3, dtype=np.float64)
    ref, env = ref3[0], np.abs(ref3[1] - ref3[2])
    assert x.shape == ref.shape, (what, x.shape, ref.shape)
    assert np.all(np.isfinite(x)), what
    s = np.abs(ref) + (np.abs(ref[0]) if height_shifted else 0.0)
    bound = BASE * s + K_ENVELOPE * env
    assert np.all(bound <= VACUOUS * s), (what, 'vacuous bound', float(np.max(bound / np.maximum(s, 1e-300))))
    err = np.abs(x - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        frac = np.where(err > 0, err / bound, 0.0)
    worst = float(np.max(frac))
    print('%-24s worst deviation %.3g of the bound (largest deviation relative to s %.3g, largest bound relative to s %.3g)%s'
          % (what, worst, float(np.max(err / np.maximum(s, 1e-300))), float(np.max(bound / np.maximum(s, 1e-300))),
             '  bit-equal' if np.array_equal(x, ref) else ''))
    bad = np.argwhere(err > bound)
    assert bad.size == 0, (what, 'outside the bar at', bad[:5].ravel().tolist(), 'worst fraction', worst)
    return worst


def check_case(case, height, cmass, tau, chi, tag=''):
    """the whole bar of a case -> {quantity: worst fraction}"""
    out = {}
    if case.scale == GEO:
        assert np.array_equal(height, case.ds), (case.name, 'geometric height is not its input')
        assert np.array_equal(case.ref['height'][0], case.ds)
    else:
        out['height'] = inside(height, case.ref['height'], '%s%s height' % (tag, case.name), height_shifted=True)
    out['cmass'] = inside(cmass, case.ref['cmass'], '%s%s cmass' % (tag, case.name))
    out['tau_ref'] = inside(tau, case.ref['tau_ref'], '%s%s tau_ref' % (tag, case.name))
    if chi is not None:
        out['chi_ref'] = inside(chi, case.ref['chi_c'], '%s%s chi_ref' % (tag, case.name))
    return out


class HostLib:
    """liblsx_scales_host.so: the formulas of lsx_scales_dev.h (and of lsx_background_dev.h) compiled for the CPU (`make scaleshost`)"""

    def __init__(self):
        subprocess.check_call(['make', '-s', '-C', CSRC, 'scaleshost'])
        self.dll = d = C.CDLL(os.path.join(CSRC, 'liblsx_scales_host.so'))
        dp, tp = C.POINTER(C.c_double), C.POINTER(_capi.LsxEosTables)
        d.lsx_scales_host_error.restype = C.c_char_p
        d.lsx_scales_host_check.argtypes = [C.c_int32, C.c_int64, C.c_int32, dp, dp, dp, dp, C.c_double]
        d.lsx_scales_host_tau1.argtypes = [C.c_int32, dp, dp]
        d.lsx_scales_host_tau1.restype = C.c_double
        d.lsx_scales_host_integrate.argtypes = [C.c_int32, C.c_int64, C.c_int32, C.c_double, dp, dp, dp, dp, C.c_double, dp, dp, dp, dp]
        d.lsx_scales_host_convert.argtypes = [tp, C.c_int32, C.c_int64, C.c_int32, dp, dp, dp, dp, C.c_double, dp, dp, dp, dp]

    @staticmethod
    def _in(a, Ns):
        return None if a is None else _capi.f64(np.asarray(a, dtype=np.float64).reshape(-1, Ns))

    def error(self):
        return self.dll.lsx_scales_host_error().decode()

    def check(self, scale, Ns, ds, T, nH, ne, g):
        ds, T, nH, ne = (self._in(a, Ns) for a in (ds, T, nH, ne))
        opt = lambda a: None if a is None else _capi._ptr(a)
        return self.dll.lsx_scales_host_check(scale, ds.shape[0], Ns, opt(ds), opt(T), opt(nH), opt(ne), g)

    def tau1(self, tau, height):
        tau, height = _capi.f64(tau), _capi.f64(height)
        return self.dll.lsx_scales_host_tau1(tau.shape[0], _capi._ptr(tau), _capi._ptr(height))

    def integrate(self, scale, wph, ds, T, nH, ne, g, chi):
        """-> rc, height, cmass, tau [ncol][Ns]"""
        Ns = np.asarray(ds).shape[-1]
        ds, T, nH, ne, chi = (self._in(a, Ns) for a in (ds, T, nH, ne, chi))
        h, cm, tau = (np.zeros_like(ds) for _ in range(3))
        rc = self.dll.lsx_scales_host_integrate(scale, ds.shape[0], Ns, wph, _capi._ptr(ds), _capi._ptr(T), _capi._ptr(nH), None if ne is None else _capi._ptr(ne), g,
                                                _capi._ptr(chi), _capi._ptr(h), _capi._ptr(cm), _capi._ptr(tau))
        return rc, h, cm, tau

    def convert(self, tab, scale, ds, T, nH, ne, g):
        """-> rc, height, cmass, tau, chi [ncol][Ns]"""
        Ns = np.asarray(ds).shape[-1]
        ds, T, nH, ne = (self._in(a, Ns) for a in (ds, T, nH, ne))
        h, cm, tau, chi = (np.zeros_like(ds) for _ in range(4))
        t, _keep = tab.to_c()
        rc = self.dll.lsx_scales_host_convert(C.byref(t), scale, ds.shape[0], Ns, _capi._ptr(ds), _capi._ptr(T), _capi._ptr(nH), None if ne is None else _capi._ptr(ne), g,
                                              _capi._ptr(h), _capi._ptr(cm), _capi._ptr(tau), _capi._ptr(chi))
        return rc, h, cm, tau, chi
