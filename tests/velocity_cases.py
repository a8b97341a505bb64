"""What the tests of the line-of-sight velocity as a quantity of the call share (tests/test_stokes_velocity_host.py,
tests/test_stokes_velocity.py; include/lsx_hip_stokes_velocity.h).  Built on tests/stokes_cases.py, tests/stokes_response_cases.py and
tests/fit_cases.py: their columns, patterns, fields, host libraries, bars and yardstick -- nothing new is typed in.

A stokes_cases.Column carries `vlos`, so `rc.changed(col, 'vlos', k, +-a/2)` and `rc.brute(..., parameters=['vlos'])` are the brute
force of RF_vlos through the pinned pass, with the bar (bar(S+) + bar(S-)) / a, and `rc.SIGNAL` is the signal condition.
The amplitude of the tests is a tenth of the smallest vBroad among the window's lines (`amplitude`).
`HostLib` adds lsx_stokes_host_response_v, `FitHostLib` lsx_fit_host_expand4 and lsx_fit_host_normal4; `HostBackend` is
fit_cases.HostBackend with four quantities, the velocity the fourth row of the expanded field.
`recovery` is fit_cases.recovery with a velocity that is linear in depth, a few tenths of vBroad."""
import ctypes as C

import numpy as np

import fit_cases as fc
import fit_instrument_cases as fic
import stokes_cases as sc
import stokes_response_cases as rc
from lightspinner_amd import fit, zeeman

PARAMS = rc.PARAMS + ('vlos',)
BITS = dict(rc.BITS, vlos=8)
SIGNAL = rc.SIGNAL
_dp, _ip, _bp = sc._dp, sc._ip, sc._bp
same = fc.same

WINDOWS = [(0, 1), (7, 1), (0, 63), (7, 64), (0, 65), (7, 130)]
MUS = np.array([1.0, 0.1, 0.6])
NNODES = [(0, 0, 0, 1), (1, 0, 0, 2), (2, 2, 2, 2), (6, 6, 6, 6)]


def amplitude(vB):
    """the tests' amplitude of vlos [m/s]: a tenth of the smallest vBroad handed over"""
    return 0.1 * float(np.min(vB))


def amps(vB):
    return dict(rc.AMPS, vlos=amplitude(vB))


def velocity(Ns, ncol):
    """velocities of the calls, [ncol][Ns] in m/s: different per column, both signs, up to about half a Doppler width"""
    d = np.linspace(0.0, 1.0, Ns)
    return sc._d(np.stack([1.2e3 * np.cos(3.0 * d + 0.7 * c) - 300.0 * c for c in range(ncol)]))


class HostLib(rc.HostLib):
    """liblsx_stokes_host.so with lsx_stokes_host_response_v"""

    def __init__(self):
        super().__init__()
        f = self.dll.lsx_stokes_host_response_v
        f.argtypes = self.dll.lsx_stokes_host_response.argtypes
        f.restype = C.c_int

    def response_v_rc(self, col, mu, parameters=PARAMS, amplitudes=None, ks=None, ulp=0, params_bits=None, amp_array=None, want_stokes=True,
                      vlos='own'):
        """-> (code, rf {name: [4][nla][nk]}, stokes [4][nla] or None) for a stokes_cases.Column (its vlos is the call's) at one angle"""
        nc, al, st, sh = zeeman.pack(col.patterns, len(col.patterns))
        nla, Ns = col.wav.shape[0], col.z.shape[0]
        amplitudes = amps(col.vB) if amplitudes is None else amplitudes
        bits = sum(BITS[p] for p in parameters) if params_bits is None else params_bits
        names = [p for p in PARAMS if p in parameters]
        amp = np.array([amplitudes.get(p, 0.0) for p in PARAMS]) if amp_array is None else np.asarray(amp_array, dtype=np.float64)
        kk = None if ks is None else np.ascontiguousarray(ks, dtype=np.int32)
        n_k = Ns if kk is None else kk.shape[0]
        rf = np.full((max(len(names), 1), 4, nla, max(n_k, 1)), np.nan)
        S = np.full((4, nla), np.nan) if want_stokes else None
        act = np.ascontiguousarray(col.active, dtype=np.uint8)
        a = [sc._d(t) for t in (col.z, col.T, col.wav, col.chi_c, col.eta_c, col.lambda0, col.nd, col.ne, col.aD, col.vB, col.vlos, col.B,
                                col.gammaB, col.chiB)]
        p = sc._p
        code = self.dll.lsx_stokes_host_response_v(Ns, nla, p(a[0]), p(a[1]), p(a[2]), p(a[3]), p(a[4]), len(col.patterns), p(a[5]), p(a[6]),
                                                   p(a[7]), p(a[8]), p(a[9]), act.ctypes.data_as(_bp), nc.ctypes.data_as(_ip),
                                                   al.ctypes.data_as(_ip), p(st), p(sh), None if vlos is None else p(a[10]), p(a[11]),
                                                   p(a[12]), p(a[13]), float(mu), int(col.lower_zero), int(ulp), bits, None if amp is None else p(amp),
                                                   n_k, None if kk is None else kk.ctypes.data_as(_ip), p(rf), None if S is None else p(S))
        return code, {n: rf[i] for i, n in enumerate(names)}, S

    def response_v(self, col, mu, **kw):
        code, rf, S = self.response_v_rc(col, mu, **kw)
        assert code == sc.LSX_OK, code
        return rf, S


class FitHostLib(fc.FitHostLib):
    """liblsx_fit_host.so with lsx_fit_host_expand4 and lsx_fit_host_normal4"""

    def __init__(self):
        super().__init__()
        d = self.dll
        d.lsx_fit_host_expand4.argtypes = d.lsx_fit_host_expand.argtypes
        d.lsx_fit_host_normal4.argtypes = [C.c_int32, C.c_int32, C.c_int32, _ip, _dp, _dp, _dp, _dp, _dp, C.c_int32, C.c_int32, _ip, _dp,
                                           _dp, _dp, _dp]
        d.lsx_fit_host_expand4.restype = d.lsx_fit_host_normal4.restype = C.c_int

    def expand4(self, Ns, nnode, basis, base, nodes):
        """-> field [ncol][4][Ns]"""
        nn = np.ascontiguousarray(nnode, dtype=np.int32)
        assert nn.shape == (4,)
        x = sc._d(np.atleast_2d(nodes))
        bs = None if base is None else sc._d(np.broadcast_to(base, (x.shape[0], 4, Ns)))
        out = np.empty((x.shape[0], 4, Ns))
        code = self.dll.lsx_fit_host_expand4(Ns, x.shape[0], nn.ctypes.data_as(_ip), fc._p(sc._d(basis)), fc._p(bs), fc._p(x), fc._p(out))
        assert code == sc.LSX_OK, code
        return out

    def normal4(self, nnode, rf, S, obs, weight, basis, chi2_only=False, instrument=None):
        """one column: rf [npar][4][nla][Ns][nmu] (None with chi2_only), S [4][nla][nmu], obs, weight [4][nla or nobs][nmu]
        -> (chi2, grad, hess)"""
        nn = np.ascontiguousarray(nnode, dtype=np.int32)
        P = int(nn.sum())
        S = sc._d(S)
        _, nla, nmu = S.shape
        Ns = np.asarray(basis).shape[-1]
        ob = sc._d(obs)
        chi2, grad, hess = np.empty(1), np.full(P, np.nan), np.full((P, P), np.nan)
        w = None if weight is None else sc._d(np.broadcast_to(weight, ob.shape))
        rf_ = None if chi2_only else sc._d(rf)
        assert rf_ is None or rf_.shape == (int((nn > 0).sum()), 4, nla, Ns, nmu), rf_.shape
        nobs, width, first, iw = 0, 0, None, None
        if instrument is not None:
            nobs, width, first, iw = instrument.nobs, instrument.width, instrument.first.ctypes.data_as(_ip), fc._p(sc._d(instrument.weight))
        code = self.dll.lsx_fit_host_normal4(Ns, nla, nmu, nn.ctypes.data_as(_ip), fc._p(rf_), fc._p(S), fc._p(ob), fc._p(w),
                                             fc._p(sc._d(basis)), nobs, width, first, iw, fc._p(chi2), None if chi2_only else fc._p(grad),
                                             None if chi2_only else fc._p(hess))
        assert code == sc.LSX_OK, code
        return chi2[0], grad, hess


def basis_of(Ns, nnode):
    return fc.basis_of(Ns, nnode)


def nodes_of(fld4, Ns, nnode, base=None):
    """fit_cases.nodes_of for four quantities ([ncol][Ns] each, the velocity last)"""
    return fc.nodes_of(fld4, Ns, nnode, base)


def off_truth(nodes, nnode, vB):
    """the start of the tests: fit_cases.off_truth for the field, the true velocity nodes + 0.3 vBroad"""
    x = np.array(nodes, dtype=np.float64)
    o = np.cumsum([0] + list(nnode))
    x[:, :o[3]] = fc.off_truth(x[:, :o[3]], nnode[:3])
    x[:, o[3]:o[4]] += 0.3 * vB
    return x


def base_of(fld4, nnode, given):
    """base [ncol][4][Ns] as fit_cases.base_of makes it"""
    return fc.base_of(fld4, nnode, given)


def smear(instrument, x):
    """x [...][nla][nmu] -> [...][nobs][nmu] by the dense matrix (tests only)"""
    return np.einsum('ol,...lm->...om', instrument.matrix(), np.asarray(x))


class HostBackend:
    """fit_cases.HostBackend with four quantities: fit_field_normal, fit_field_chi2, fit_field_step as Engine has them for nnode of four
    counts, from HostLib (the response and the Stokes window of a Column whose vlos is the expanded velocity) and FitHostLib"""

    def __init__(self, host, fithost, prob, block, prof, n, J, patterns, la0, nla):
        self.host, self.fh, self.args, self.patterns, self.la0, self.nla = host, fithost, (prob, block, prof, n, J), patterns, la0, nla
        self.Ns, self.ncol = prob.Nspace, block.ncol
        self.calls = {'normal': 0, 'chi2': 0, 'step': 0}

    def _columns(self, field):
        fld = [sc._d(field[:, p]) for p in range(3)]
        return [sc.column(*self.args, fld, self.patterns, c, self.la0, self.nla).replace(vlos=sc._d(field[c, 3])) for c in range(self.ncol)]

    def response(self, field, mus, nnode, amplitudes):
        """-> rf [ncol][npar][4][nla][Ns][nmu], S [ncol][4][nla][nmu]"""
        names = [p for p, n in zip(PARAMS, nnode) if n > 0]
        rf, S = [], []
        for col in self._columns(field):
            per = [self.host.response_v(col, mu, parameters=names, amplitudes=amplitudes) for mu in mus]
            rf.append(np.stack([np.stack([r[0][p] for r in per], axis=-1) for p in names]))
            S.append(np.stack([r[1] for r in per], axis=-1))
        return np.stack(rf), np.stack(S)

    def fit_field_normal(self, mus, basis, nnode, nodes, obs, weight=None, base=None, amplitudes=None, instrument=None):
        self.calls['normal'] += 1
        field = self.fh.expand4(self.Ns, nnode, basis, base, nodes)
        rf, S = self.response(field, np.atleast_1d(mus), nnode, amplitudes)
        w = None if weight is None else np.broadcast_to(weight, obs.shape)
        out = [self.fh.normal4(nnode, rf[c], S[c], obs[c], None if w is None else w[c], basis, instrument=instrument) for c in range(self.ncol)]
        return fit.FieldNormal(np.array([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]), field)

    def fit_field_chi2(self, mus, basis, nnode, nodes, obs, weight=None, base=None, instrument=None):
        self.calls['chi2'] += 1
        field = self.fh.expand4(self.Ns, nnode, basis, base, nodes)
        S = np.stack([np.stack([self.host.window(col, mu) for mu in np.atleast_1d(mus)], axis=-1) for col in self._columns(field)])
        w = None if weight is None else np.broadcast_to(weight, obs.shape)
        return np.array([self.fh.normal4(nnode, None, S[c], obs[c], None if w is None else w[c], basis, chi2_only=True, instrument=instrument)[0]
                         for c in range(self.ncol)]), field

    def fit_field_step(self, hess, grad, lam, nodes, lo=None, hi=None):
        self.calls['step'] += 1
        return self.fh.step(hess, grad, lam, nodes, lo, hi)[:3]


# ---- the loop's test --------------------------------------------------------------------------------------------------------------------
RECOVERY_WINDOW = fc.RECOVERY_WINDOW
# Ns, nodes per quantity, angles, columns, through Instrument.gaussian
RECOVERY_CASES = [(13, 2, [1.0], 1, False), (13, 2, [1.0, 0.6], 1, False), (5, 2, [1.0], 1, False), (13, 2, [1.0], 3, False),
                  (13, 2, [1.0], 1, True)]
# The iteration cap of the velocity cases: the count of the same loop on the host backend (tests/test_stokes_velocity_host.py runs it
# and asserts it) plus 2.  HOST_ITERATIONS: the host loop's measured counts (the slowest column's), in the order of RECOVERY_CASES
HOST_ITERATIONS = {0: 5, 1: 5, 2: 6, 3: 5, 4: 5}
RECOVERY_LOOP = dict(lambda0=1e-2, factor=10.0)


def max_iter(case):
    return HOST_ITERATIONS[case] + 2


def recovery(Ns, ncol, nn):
    """fit_cases.recovery with the velocity: -> (problem parts, patterns, truth [4] x [ncol][Ns], nnode, basis, true nodes, start nodes,
    vBroad): the truth's velocity falls linearly with depth from +0.3 to -0.2 of the smallest vBroad (a little more per column)"""
    parts, pats, fld, _, _, _, _ = fc.recovery(Ns, ncol, nn)
    vB = float(np.min(parts[2][1]))
    d = np.linspace(0.0, 1.0, Ns)
    v = sc._d(np.stack([vB * (0.3 - 0.5 * d) * (1.0 + 0.2 * c) for c in range(ncol)]))
    fld4 = list(fld) + [v]
    nnode = (nn, nn, nn, nn)
    truth = nodes_of(fld4, Ns, nnode)
    return parts, pats, fld4, nnode, basis_of(Ns, nnode), truth, off_truth(truth, nnode, vB), vB


def recovery_instrument(prob, window=RECOVERY_WINDOW):
    """fit_instrument_cases' first instrument of its loop's test on the window: Instrument.gaussian, 30 pixels, fwhm of two grid steps"""
    return fic.recovery_instrument(fic.window_grid(prob, *window), 'a')


def check_recovery(r, truth, nnode, vB, cap):
    """fit_cases.check_recovery with the velocity nodes' error in units of vBroad (a velocity enters the profile as vlos / vBroad,
    dimensionless like the angles)"""
    o = int(np.sum(nnode[:3]))
    scaled = lambda x: np.concatenate([x[:, :o], x[:, o:] / vB], axis=1)
    rr = fit.FieldFit(scaled(r.nodes), r.field, r.chi2, r.history, r.lam, r.iterations, r.status, r.nnode)
    fc.check_recovery(rr, scaled(truth), max_iter=cap)
