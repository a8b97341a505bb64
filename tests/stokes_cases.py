"""What the tests of the polarised final pass share (tests/test_stokes_host.py, tests/test_stokes.py; include/lsx_hip_stokes.h).

`HostLib` is liblsx_stokes_host.so (make stokeshost): the formulas of lsx_stokes_dev.h compiled for the CPU without contraction, with
the test-only hook that moves every exp(-dtau) by +-1 ulp (the envelope of tests/envelope.py, applied here).
`problem(...)` is a made-up problem from tests/toy.py (its columns: heights, temperatures, populations, background) moved onto a fine
wavelength grid round 500 nm, where three lines of one atom blend over two continua; `PATTERNS` are a normal triplet, an anomalous
pattern of the largest size among the reference's lines (27 components) and a small anomalous one.
`host_stokes` is the reference of the GPU tests: background, sigma J and the continua restated in numpy (rh_method.py:601-632), every
line through the host library, on the populations and J handed over.
The bar, per entry and for all four parameters:  |x - x_host| <= 1e-11 I_host + 3 |x_host(+1 ulp) - x_host(-1 ulp)|."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np

import toy
from conftest import ROOT
from lightspinner_amd import constants as Const
from lightspinner_amd import zeeman
from lightspinner_amd.problem import Problem, Transition

CSRC = os.path.join(ROOT, 'lightspinner_amd', 'csrc')
U = 2.0 ** -53
BASE = 1e-11
K_ENVELOPE = 3.0
LARMOR = 1.60217733E-19 / (4.0 * np.pi * 9.1093897E-31)      # e / (4 pi m_e), the library's constants
CLIGHT = 2.99792458E+08
MAX_COMPONENTS = 64
LSX_OK, LSX_EINVAL, LSX_EUNSUPPORTED = 0, 1, 5

_dp, _ip, _bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return a.ctypes.data_as(_dp)


class HostLib:
    """liblsx_stokes_host.so: lsx_stokes_dev.h compiled for the CPU"""

    def __init__(self):
        subprocess.check_call(['make', '-s', '-C', CSRC, 'stokeshost'])
        self.dll = d = C.CDLL(os.path.join(CSRC, 'liblsx_stokes_host.so'))
        d.lsx_stokes_host_w.argtypes = [C.c_int64, _dp, _dp, _dp, _dp, _dp]
        d.lsx_stokes_host_w.restype = None
        d.lsx_stokes_host_geometry.argtypes = [C.c_int64, _dp, _dp, _dp, _dp]
        d.lsx_stokes_host_geometry.restype = None
        d.lsx_stokes_host_check.argtypes = [C.c_int64, _dp, _dp, _dp, C.c_int32, _ip, _ip, _dp, _dp]
        d.lsx_stokes_host_check.restype = C.c_int
        d.lsx_stokes_host_K.argtypes = [C.c_double, C.c_double, C.c_int32, _dp, _dp, _dp, _dp, _dp, _dp, _ip, _ip, _dp, _dp,
                                        C.c_double, C.c_double, C.c_double, _dp]
        d.lsx_stokes_host_K.restype = C.c_int
        d.lsx_stokes_host_ray.argtypes = [C.c_int32, _dp, _dp, C.c_double, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_int32, _dp]
        d.lsx_stokes_host_ray.restype = C.c_int
        d.lsx_stokes_host_window.argtypes = [C.c_int32, C.c_int32, _dp, _dp, _dp, _dp, _dp, C.c_int32, _dp, _dp, _dp, _dp, _dp, _bp,
                                             _ip, _ip, _dp, _dp, _dp, _dp, _dp, _dp, C.c_double, C.c_int32, C.c_int32, C.c_int32, _dp]
        d.lsx_stokes_host_window.restype = C.c_int

    def w(self, a, v):
        """-> (H, F, dev_voigt's H) of w(v + i a), elementwise"""
        a, v = np.broadcast_arrays(_d(a), _d(v))
        a, v = _d(a).reshape(-1), _d(v).reshape(-1)
        H, F, Hv = np.empty_like(a), np.empty_like(a), np.empty_like(a)
        self.dll.lsx_stokes_host_w(a.shape[0], _p(a), _p(v), _p(H), _p(F), _p(Hv))
        return H, F, Hv

    def geometry(self, gammaB, chiB, mu):
        """-> [n][4] = (c, s2, sQ, sU)"""
        g, x, m = (np.ascontiguousarray(t, dtype=np.float64).reshape(-1) for t in np.broadcast_arrays(_d(gammaB), _d(chiB), _d(mu)))
        out = np.empty((g.shape[0], 4))
        self.dll.lsx_stokes_host_geometry(g.shape[0], _p(g), _p(x), _p(m), _p(out))
        return out

    def check(self, B, gammaB, chiB, patterns):
        """the code the entry's rules give for this field and these patterns (one entry per line)"""
        B, g, x = (_d(t).reshape(-1) for t in (B, gammaB, chiB))
        nc, al, st, sh = zeeman.pack(patterns, len(patterns))
        return self.dll.lsx_stokes_host_check(B.shape[0], _p(B), _p(g), _p(x), len(patterns), nc.ctypes.data_as(_ip),
                                              al.ctypes.data_as(_ip), _p(st), _p(sh))

    def K(self, chi_c, eta_c, nd, ne, aD, v, vZ, rn, patterns, gammaB, chiB, mu):
        """-> [11]: eta_I, eta_Q, eta_U, eta_V, rho_Q, rho_U, rho_V, eps_I, eps_Q, eps_U, eps_V at one point"""
        arr = [_d(np.atleast_1d(t)) for t in (nd, ne, aD, v, vZ, rn)]
        nc, al, st, sh = zeeman.pack(patterns, len(patterns))
        out = np.empty(11)
        rc = self.dll.lsx_stokes_host_K(float(chi_c), float(eta_c), len(patterns), *(_p(t) for t in arr), nc.ctypes.data_as(_ip),
                                        al.ctypes.data_as(_ip), _p(st), _p(sh), float(gammaB), float(chiB), float(mu), _p(out))
        assert rc == LSX_OK, rc
        return out

    def ray(self, z, K, mu, thermal=None, ulp=0, endpoint=True):
        """one ray through K [Ns][11] -> [4]; thermal: None (start from 0) or (Be, Bn); endpoint: with the reference's end-point term in
        I, as the kernel has it (False: the plain DELO-linear step at the end point too)"""
        z, K = _d(z), _d(K)
        out = np.empty(4)
        Be, Bn = (0.0, 0.0) if thermal is None else thermal
        rc = self.dll.lsx_stokes_host_ray(z.shape[0], _p(z), _p(K), float(mu), int(thermal is not None), float(Be), float(Bn), int(ulp), int(endpoint), _p(out))
        assert rc == LSX_OK, rc
        return out

    def window(self, col, mu, ulp=0, endpoint=True):
        """a Column (below) at one angle -> [4][nla]; endpoint as in ray()"""
        nc, al, st, sh = zeeman.pack(col.patterns, len(col.patterns))
        nla, Ns = col.wav.shape[0], col.z.shape[0]
        out = np.empty((4, nla))
        act = np.ascontiguousarray(col.active, dtype=np.uint8)
        a = [_d(t) for t in (col.z, col.T, col.wav, col.chi_c, col.eta_c, col.lambda0, col.nd, col.ne, col.aD, col.vB, col.vlos, col.B,
                             col.gammaB, col.chiB)]
        rc = self.dll.lsx_stokes_host_window(Ns, nla, _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), _p(a[4]), len(col.patterns), _p(a[5]), _p(a[6]),
                                             _p(a[7]), _p(a[8]), _p(a[9]), act.ctypes.data_as(_bp), nc.ctypes.data_as(_ip),
                                             al.ctypes.data_as(_ip), _p(st), _p(sh), _p(a[10]), _p(a[11]), _p(a[12]), _p(a[13]), float(mu),
                                             int(col.lower_zero), int(ulp), int(endpoint), _p(out))
        assert rc == LSX_OK, rc
        return out


@dataclasses.dataclass
class Column:
    """what lsx_stokes_host_window takes for one column and one window"""
    z: np.ndarray
    T: np.ndarray
    wav: np.ndarray            # [nla]
    chi_c: np.ndarray          # [nla][Ns]: everything that is not a line
    eta_c: np.ndarray
    lambda0: np.ndarray        # [nlines]
    nd: np.ndarray             # [nlines][Ns]
    ne: np.ndarray
    aD: np.ndarray
    vB: np.ndarray
    active: np.ndarray         # [nlines][nla]
    patterns: list
    vlos: np.ndarray
    B: np.ndarray
    gammaB: np.ndarray
    chiB: np.ndarray
    lower_zero: bool = False

    def replace(self, **kw):
        return dataclasses.replace(self, **kw)


# ---- patterns -----------------------------------------------------------------------------------------------------------------------
class _Lev:
    def __init__(self, J, L, S):
        from fractions import Fraction
        self.J, self.L, self.S, self.lsCoupling = Fraction(J), L, Fraction(S), True


class _Line:
    def __init__(self, lo=None, up=None, g=None):
        self.iLevel, self.jLevel, self.gLandeEff = lo, up, g


TRIPLET = zeeman.zeeman_components(_Line(g=1.1))                                       # 3 components
LARGEST = zeeman.zeeman_components(_Line(_Lev(4, 2, 2), _Lev(5, 2, 3)))               # J = 4 - 5: 27, the largest of the reference's lines
SMALL = zeeman.zeeman_components(_Line(_Lev('1/2', 0, '1/2'), _Lev('3/2', 1, '1/2')))  # 2S1/2 - 2P3/2: 6
assert (len(TRIPLET), len(LARGEST), len(SMALL)) == (3, 27, 6)
PATTERN_SETS = {'none': [None, None, None], 'triplet': [None, TRIPLET, None], 'largest': [None, LARGEST, None],
                'blend': [SMALL, TRIPLET, None], 'all': [SMALL, LARGEST, TRIPLET]}


# ---- the made-up problem ------------------------------------------------------------------------------------------------------------
NSPECT = 147                  # seven tiles of L = 21 wavelengths (3 rays)
DLAMBDA = 0.002               # nm; the Doppler width is about 0.005 nm
LAMBDA0 = (499.972, 500.0, 500.031)


def problem(Ns, ncol, vlos=False, compact=False, seed=7):
    """-> (prob, block, prof, J): one atom of 6 levels, three lines from the ground level that blend round 500 nm and two continua over
    the whole grid (the topology of toy.toy_problem(multiplet=3)); the columns are toy's, the profiles are built by the library from
    prof = (aDamp [ncol][3][Ns], vBroad [ncol][1][Ns], vlos [ncol][Ns] or None); J [ncol][Nspect][Ns] is made up too"""
    specs = [('l', 0, u, 0.0, 1.0) for u in (1, 2, 3)] + [('c', 0, 5, 0.0, 1.0), ('c', 1, 5, 0.0, 1.0)]
    p0, b0 = toy.spec_problem([(6, specs)], seed=seed, Nspace=Ns, Nrays=3, Nspect=NSPECT, ncol=ncol, phi_compact=compact)
    wl = 500.0 + DLAMBDA * (np.arange(NSPECT) - NSPECT // 2) + 1e-4 * np.sin(np.arange(NSPECT))          # not equidistant
    trans, li = [], 0
    for t in p0.trans:
        if t.is_line:
            lam0 = LAMBDA0[li]
            li += 1
            Bij = t.Bij
            Bji = t.Bji / t.Bij * Bij
            trans.append(Transition(t.atom, True, t.i, t.j, 0, NSPECT, Aji=2.0 * toy.HC / (lam0 * 1e-9) ** 3 * Bji, Bji=Bji, Bij=Bij, lambda0=lam0))
        else:
            trans.append(Transition(t.atom, False, t.i, t.j, 0, NSPECT, lambda0=wl[-1], alpha=np.asarray(t.alpha) * (wl / wl[-1]) ** 3))
    prob = Problem(Nspace=Ns, wavelength=wl, muz=p0.muz, wmu=p0.wmu, Nlevel=p0.Nlevel, trans=trans,
                   active=np.ones((len(trans), NSPECT), dtype=np.uint8), sca_per_lambda=False, phi_compact=compact, atom_names=p0.atom_names)
    block = dataclasses.replace(b0, phi=None, wphi=None).validate(prob)
    rng = np.random.default_rng(seed + 100)
    d = np.linspace(0.0, 1.0, Ns)
    aD = np.stack([[10.0 ** (-3.0 + 1.5 * d + 0.3 * l) * (1.0 + 0.1 * c) for l in range(3)] for c in range(ncol)])
    vB = np.stack([[2.5e3 + 1.5e3 * d ** 2 + 100.0 * c] for c in range(ncol)])
    vl = None
    if vlos:
        vl = np.stack([4.0e3 * np.sin(4.0 * d + c) * (1.0 - d) for c in range(ncol)])
    assert not (compact and vlos)
    J = 0.4 * block.bg_eta / block.bg_chi * (1.0 + 0.2 * rng.uniform(-1, 1, block.bg_chi.shape))
    return prob, block, (aD, vB, vl), J


def field(Ns, ncol, kind='inclined', B0=0.12):
    """-> (B, gammaB, chiB), [ncol][Ns] each.  'gaps': depths with B = 0 between depths with a field; 'along' / 'across' / 'away':
    gamma = 0, pi / 2, pi"""
    d = np.linspace(0.0, 1.0, Ns)
    B = B0 * (0.5 + d)[None, :] * (1.0 + 0.3 * np.arange(ncol))[:, None]
    g = (0.4 + 1.9 * d)[None, :] + 0.1 * np.arange(ncol)[:, None]
    x = (0.5 - 2.5 * d)[None, :] - 0.2 * np.arange(ncol)[:, None]
    if kind == 'gaps':
        B = B * (np.arange(Ns) % 3 != 1)[None, :]
    elif kind in ('along', 'across', 'away'):
        g = np.full_like(g, {'along': 0.0, 'across': 0.5 * np.pi, 'away': np.pi}[kind])
    elif kind == 'zero':
        B = np.zeros_like(B)
    else:
        assert kind == 'inclined'
    return _d(B), _d(g), _d(x)


def column(prob, block, prof, n, J, fld, patterns, col, la0=0, nla=None, lower_zero=False):
    """the Column of one column of a problem: background, sigma J and the continua restated (rh_method.py:601-632), the lines handed on.
    n [ncol][NLtot][Ns], J [ncol][Nspect][Ns]"""
    nla = prob.Nspect - la0 if nla is None else nla
    Ns = prob.Nspace
    hc_4pi = 0.25 * Const.HC / np.pi
    hc_k = Const.HC / (Const.KBoltzmann * Const.NM_TO_M)
    T = block.temperature[col]
    wav = prob.wavelength[la0:la0 + nla]
    chi_c, eta_c = np.zeros((nla, Ns)), np.zeros((nla, Ns))
    lines = []
    for kr, t in enumerate(prob.trans):
        o = int(prob.lev_off[t.atom])
        ni, nj = n[col, o + t.i], n[col, o + t.j]
        if t.is_line:
            cB = hc_4pi * t.Bij
            g = t.Bji / t.Bij
            lines.append((t.lambda0, cB * (ni - g * nj), nj * (t.Aji / t.Bji * (g * cB)), prof[0][col, len(lines)], prof[1][col, t.atom],
                          prob.active[kr, la0:la0 + nla]))
            continue
        for q in range(nla):
            la = la0 + q
            if not prob.active[kr, la]:
                continue
            gij = block.nStar[col, o + t.i] / block.nStar[col, o + t.j] * np.exp(-hc_k / wav[q] / T)
            Vij = float(t.alpha[la - t.Nblue])
            Vji = gij * Vij
            chi_c[q] += ni * Vij - nj * Vji
            eta_c[q] += nj * (2.0 * Const.HC / (Const.NM_TO_M * wav[q]) ** 3 * Vji)
    sca = block.bg_sca[col, la0:la0 + nla] if prob.sca_per_lambda else block.bg_sca[col][None, :]
    chi_c += block.bg_chi[col, la0:la0 + nla]
    eta_c += block.bg_eta[col, la0:la0 + nla] + sca * J[col, la0:la0 + nla]
    st = lambda i: np.stack([l[i] for l in lines]) if lines else np.zeros((0, Ns))
    vl = np.zeros(Ns) if prof[2] is None else prof[2][col]
    return Column(z=block.height[col], T=T, wav=wav, chi_c=chi_c, eta_c=eta_c, lambda0=np.array([l[0] for l in lines]), nd=st(1), ne=st(2),
                  aD=st(3), vB=st(4), active=st(5) if lines else np.zeros((0, nla), dtype=np.uint8), patterns=list(patterns), vlos=vl,
                  B=fld[0][col], gammaB=fld[1][col], chiB=fld[2][col], lower_zero=lower_zero)


def host_stokes(host, prob, block, prof, n, J, fld, patterns, mus, la0=0, nla=None, ulp=0, cols=None, lower_zero=False):
    """-> [ncol][4][nla][nmu]: what lsx_hip_stokes_rays computes, by the host library"""
    cols = range(block.ncol) if cols is None else cols
    out = []
    for c in cols:
        cc = column(prob, block, prof, n, J, fld, patterns, c, la0, nla, lower_zero)
        out.append(np.stack([host.window(cc, mu, ulp) for mu in mus], axis=-1))
    return np.stack(out)


def bars(host_runs):
    """host_runs: {0: x, 1: x(+1 ulp), -1: x(-1 ulp)}, each [...][4][nla][nmu] -> the bar per entry, the same for all four parameters"""
    I = np.abs(host_runs[0][..., 0:1, :, :])
    return BASE * I + K_ENVELOPE * np.abs(host_runs[1] - host_runs[-1])


def excess(x, host_runs):
    """largest |x - x_host| / bar over the entries (<= 1: inside), and the largest deviation relative to I"""
    dev = np.abs(np.asarray(x) - host_runs[0])
    bar = bars(host_runs)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bar > 0, dev / bar, np.where(dev > 0, np.inf, 0.0))
    return float(np.max(r)), float(np.max(dev / np.abs(host_runs[0][..., 0:1, :, :])))


def runs(host, *a, **kw):
    return {u: host_stokes(host, *a, ulp=u, **kw) for u in (0, 1, -1)}


# ---- the reference's linear rule, restated (formal_solver.py:107-139) -------------------------------------------------------------------
def _w2(dtau, ulp):
    if dtau < 5e-4:
        return dtau * (1.0 - 0.5 * dtau), dtau * dtau * (0.5 - dtau / 3.0)
    e = np.exp(-min(dtau, 700.0))
    if ulp:
        e = np.nextafter(e, np.inf if ulp > 0 else -np.inf)
    return 1.0 - e, (1.0 - e) - dtau * e


def linear_rule(z, chi, S, mu, I0, ulp=0, endpoint=True):
    """I at depth 0 of the up-going ray by I_k = I_u e^-dtau + w0 S_k + w1 (S_u - S_k) / dtau from I0 at the last depth; numpy, with
    the Taylor branch of the weights below dtau = 5e-4 and exp(-dtau) moved by `ulp`.  endpoint: the reference's end point
    (formal_solver.py:138-139: the previous interval's weights and the source function of the depth behind, this interval's slope);
    False: the plain step there too"""
    I, prev = I0, 1.0
    for k in range(len(z) - 2, -1, -1):
        dtau = 0.5 * (chi[k + 1] + chi[k]) * abs(z[k + 1] - z[k]) / mu
        dS = (S[k + 1] - S[k]) / dtau
        if k == 0 and endpoint:
            w0, w1 = _w2(prev, ulp)
            I = I * (1.0 - w0) + w0 * S[k + 1] + w1 * dS
        else:
            w0, w1 = _w2(dtau, ulp)
            I = I * (1.0 - w0) + w0 * S[k] + w1 * dS
        prev = dtau
    return I


def planck(T, wav):
    hc_Tkla = Const.HC / (Const.KBoltzmann * Const.NM_TO_M * wav) / T
    return (2.0 * Const.HC) / (Const.NM_TO_M * wav) ** 3 / (np.exp(hc_Tkla) - 1.0)


def thermal_start(col, q, mu, chi):
    """formal_solver.py:203-207 for wavelength q of a Column with total opacity chi [Ns]"""
    Be, Bn = planck(col.T[-1], col.wav[q]), planck(col.T[-2], col.wav[q])
    dtau = 0.5 * (chi[-1] + chi[-2]) * abs(col.z[-2] - col.z[-1]) / mu
    return Be - (Bn - Be) / dtau
