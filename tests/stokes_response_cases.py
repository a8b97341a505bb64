"""What the tests of the Stokes response functions share (tests/test_stokes_response_host.py, tests/test_stokes_response.py;
include/lsx_hip_stokes_response.h).  Built on tests/stokes_cases.py: its columns, patterns, host library and bar.

The yardstick is brute force through the pinned pass: RF_p[k] = (S(p_k + a/2) - S(p_k - a/2)) / a from two runs of
lsx_stokes_host_window with the field changed at depth k alone.  Each run has the Stokes bar of stokes_cases.bars
(1e-11 I_host + 3 x the +-1-ulp-exp envelope per entry), so a brute-force response has (bar(S+) + bar(S-)) / a per entry: nothing new
is typed in.  SIGNAL is the signal condition: per case and parameter the largest |RF_brute| is at least SIGNAL x the largest bar."""
import ctypes as C

import numpy as np

import stokes_cases as sc
from lightspinner_amd import zeeman

PARAMS = ('B', 'gammaB', 'chiB')
BITS = {'B': 1, 'gammaB': 2, 'chiB': 4}
# amplitudes of the tests: a tenth of stokes_cases.field's 0.12 T, and the same number of radians
AMPS = {'B': 0.012, 'gammaB': 0.012, 'chiB': 0.012}
SIGNAL = 1000.0

_dp, _ip, _bp = sc._dp, sc._ip, sc._bp


class HostLib(sc.HostLib):
    """liblsx_stokes_host.so with lsx_stokes_host_response"""

    def __init__(self):
        super().__init__()
        f = self.dll.lsx_stokes_host_response
        f.argtypes = [C.c_int32, C.c_int32, _dp, _dp, _dp, _dp, _dp, C.c_int32, _dp, _dp, _dp, _dp, _dp, _bp, _ip, _ip, _dp, _dp, _dp, _dp,
                      _dp, _dp, C.c_double, C.c_int32, C.c_int32, C.c_uint32, _dp, C.c_int32, _ip, _dp, _dp]
        f.restype = C.c_int

    def response_rc(self, col, mu, parameters=PARAMS, amplitudes=AMPS, ks=None, ulp=0, params_bits=None, amp_array=None, nk=None,
                    want_stokes=True):
        """-> (code, rf {name: [4][nla][nk]}, stokes [4][nla] or None) for a stokes_cases.Column at one angle"""
        nc, al, st, sh = zeeman.pack(col.patterns, len(col.patterns))
        nla, Ns = col.wav.shape[0], col.z.shape[0]
        bits = sum(BITS[p] for p in parameters) if params_bits is None else params_bits
        names = [p for p in PARAMS if p in parameters]
        amp = np.array([amplitudes.get(p, 0.0) for p in PARAMS]) if amp_array is None else np.asarray(amp_array, dtype=np.float64)
        kk = None if ks is None else np.ascontiguousarray(ks, dtype=np.int32)
        n_k = (Ns if kk is None else kk.shape[0]) if nk is None else nk
        rf = np.full((max(len(names), 1), 4, nla, max(n_k, 1)), np.nan)
        S = np.full((4, nla), np.nan) if want_stokes else None
        act = np.ascontiguousarray(col.active, dtype=np.uint8)
        a = [sc._d(t) for t in (col.z, col.T, col.wav, col.chi_c, col.eta_c, col.lambda0, col.nd, col.ne, col.aD, col.vB, col.vlos, col.B,
                                col.gammaB, col.chiB)]
        p = sc._p
        rc = self.dll.lsx_stokes_host_response(Ns, nla, p(a[0]), p(a[1]), p(a[2]), p(a[3]), p(a[4]), len(col.patterns), p(a[5]), p(a[6]),
                                               p(a[7]), p(a[8]), p(a[9]), act.ctypes.data_as(_bp), nc.ctypes.data_as(_ip),
                                               al.ctypes.data_as(_ip), p(st), p(sh), p(a[10]), p(a[11]), p(a[12]), p(a[13]), float(mu),
                                               int(col.lower_zero), int(ulp), bits, p(amp), n_k,
                                               None if kk is None else kk.ctypes.data_as(_ip), p(rf), None if S is None else p(S))
        return rc, {n: rf[i] for i, n in enumerate(names)}, S

    def response(self, col, mu, **kw):
        rc, rf, S = self.response_rc(col, mu, **kw)
        assert rc == sc.LSX_OK, rc
        return rf, S


def changed(col, name, k, delta):
    """the Column with parameter `name` moved by delta at depth k alone"""
    a = np.array(getattr(col, name), dtype=np.float64)
    a[k] = a[k] + delta if delta > 0 else a[k] - (-delta)
    return col.replace(**{name: a})


def brute(host, col, mu, parameters=PARAMS, amplitudes=AMPS, ks=None):
    """-> (rf {name: [4][nla][nk]}, bar {name: [4][nla][nk]}): central differences of lsx_stokes_host_window and their bar"""
    Ns = col.z.shape[0]
    ks = range(Ns) if ks is None else ks
    rf, bar = {}, {}
    for name in parameters:
        a = amplitudes[name]
        r, b = [], []
        for k in ks:
            run = {(sg, u): host.window(changed(col, name, k, sg * 0.5 * a), mu, ulp=u) for sg in (1, -1) for u in (0, 1, -1)}
            r.append((run[1, 0] - run[-1, 0]) / a)
            b.append(sum(sc.BASE * np.abs(run[sg, 0][0:1]) + sc.K_ENVELOPE * np.abs(run[sg, 1] - run[sg, -1]) for sg in (1, -1)) / a)
        rf[name], bar[name] = np.stack(r, axis=-1), np.stack(b, axis=-1)
    return rf, bar


def ratio(x, ref, bar):
    """largest |x - ref| / bar over the entries (<= 1: inside)"""
    dev = np.abs(np.asarray(x) - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bar > 0, dev / bar, np.where(dev > 0, np.inf, 0.0))
    return float(np.max(r))


def signal(ref, bar):
    """largest |RF_brute| over the largest bar"""
    return float(np.max(np.abs(ref)) / np.max(bar))


def stack_rf(r, names=None):
    """a StokesResponse's rf -> [ncol][npar][4][nla][nk][nmu]"""
    names = [p for p in PARAMS if p in r.rf] if names is None else names
    return np.stack([r.rf[n] for n in names], axis=1)
