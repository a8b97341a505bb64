"""What the background tests share (tests/test_background_host.py, tests/test_background.py): the fixture of
tests/golden/make_background_golden.py, the tables made from it, and the bar.

The bar, entry by entry:  |x - x_ref| <= 1e-12 |x_ref| + 3 |x_ref(+1) - x_ref(-1)|  where x_ref(+-1) is the REFERENCE with every
exp / log / log10 of witt's namespace moved by one unit in the last place (the suite's one-ulp envelope, tests/envelope.py, taken
from the reference, not from the code under test).  A bound above 1e-8 |x| anywhere fails the check as vacuous."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from conftest import ROOT, golden

from lightspinner_amd import _capi
from lightspinner_amd.background import EosTables

CSRC = os.path.join(ROOT, 'lightspinner_amd', 'csrc')
BASE, K_ENVELOPE, VACUOUS = 1e-12, 3.0, 1e-8
U = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def fixture():
    return dict(np.load(golden('background_eos.npz')))


def tables(iter_cap=0):
    d = fixture()
    return EosTables(d['tpf'], d['pf'], d['eion'], d['nstage'], d['abund'], d['amass'], float(d['weight_per_H']), iter_cap=iter_cap)


def inside(x, ref, env, what):
    """asserts the bar; -> the largest deviation as a fraction of the bound"""
    x, ref, env = (np.asarray(a, dtype=np.float64) for a in (x, ref, env))
    assert x.shape == ref.shape == env.shape, (what, x.shape, ref.shape, env.shape)
    assert np.all(np.isfinite(x)), what
    bound = BASE * np.abs(ref) + K_ENVELOPE * env
    assert np.all(bound <= VACUOUS * np.abs(x)), (what, 'vacuous bound', float(np.max(bound / np.maximum(np.abs(x), 1e-300))))
    err = np.abs(x - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        frac = np.where(err > 0, err / bound, 0.0)
    worst = float(np.max(frac)) if frac.size else 0.0
    print('%-28s worst deviation %.3g of the bound (largest relative deviation %.3g, largest relative bound %.3g)'
          % (what, worst, float(np.max(err / np.maximum(np.abs(ref), 1e-300))), float(np.max(bound / np.maximum(np.abs(ref), 1e-300)))))
    bad = np.argwhere(err > bound)
    assert bad.size == 0, (what, 'outside the bar at', bad[:5].tolist(), 'worst fraction', worst)
    return worst


def rel_env(code16):
    """the fixture's float16 relative envelope widths -> float64 relative widths"""
    return code16.astype(np.float64) / float(fixture()['env_scale'])


def falc_env_for(wavelength):
    """relative envelope of chi [nw][82] for wavelengths of the FALC grids"""
    d = fixture()
    idx = np.searchsorted(d['falc_env_wavelength'], wavelength)
    assert np.array_equal(d['falc_env_wavelength'][idx], wavelength)
    return rel_env(d['falc_chi_env16'][idx])


class HostLib:
    """liblsx_bg_host.so: the formulas of lsx_background_dev.h compiled for the CPU (`make bghost`)"""

    def __init__(self):
        subprocess.check_call(['make', '-s', '-C', CSRC, 'bghost'])
        self.dll = d = C.CDLL(os.path.join(CSRC, 'liblsx_bg_host.so'))
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        tp = C.POINTER(_capi.LsxEosTables)
        d.lsx_bg_host_error.restype = C.c_char_p
        d.lsx_bg_host_derived.argtypes = [tp, dp]
        d.lsx_bg_host_eos.argtypes = [tp, C.c_int64, dp, dp, dp, dp, dp, ip]
        d.lsx_bg_host_opacity.argtypes = [C.c_int64, dp, dp, dp, dp, C.c_int32, dp, dp, dp]

    def derived(self, tab):
        out = np.zeros(3)
        t, _keep = tab.to_c()
        assert self.dll.lsx_bg_host_derived(C.byref(t), _capi._ptr(out)) == 0, self.dll.lsx_bg_host_error()
        return out

    def eos(self, tab, T, nH):
        """-> rc, pgas, pe, partials [n][17], status"""
        T, nH = _capi.f64(T).reshape(-1), _capi.f64(nH).reshape(-1)
        n = T.shape[0]
        pg, pe, part, st = np.zeros(n), np.zeros(n), np.zeros((n, 17)), np.zeros(n, dtype=np.int32)
        t, _keep = tab.to_c()
        rc = self.dll.lsx_bg_host_eos(C.byref(t), n, _capi._ptr(T), _capi._ptr(nH), _capi._ptr(pg), _capi._ptr(pe), _capi._ptr(part),
                                      st.ctypes.data_as(C.POINTER(C.c_int32)))
        return rc, pg, pe, part, st

    def opacity(self, T, pg, pe, part, wavelength):
        """-> chi, eta [n][nla]"""
        T, w = _capi.f64(T).reshape(-1), _capi.f64(wavelength).reshape(-1)
        chi, eta = np.zeros((T.shape[0], w.shape[0])), np.zeros((T.shape[0], w.shape[0]))
        rc = self.dll.lsx_bg_host_opacity(T.shape[0], _capi._ptr(T), _capi._ptr(_capi.f64(pg)), _capi._ptr(_capi.f64(pe)),
                                          _capi._ptr(_capi.f64(part)), w.shape[0], _capi._ptr(w), _capi._ptr(chi), _capi._ptr(eta))
        assert rc == 0
        return chi, eta


def planck(temp, wav):
    """utils.py:17-22"""
    HC, KB, NM = 6.6260755E-34 * 2.99792458E+08, 1.380658E-23, 1.0E-09
    return (2.0 * HC) / (NM * wav) ** 3 / (np.exp(HC / (KB * NM * wav) / temp) - 1.0)
