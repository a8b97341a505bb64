"""What the tests of the field fit share (tests/test_fit_host.py, tests/test_fit.py; include/lsx_hip_fit.h).  Built on
tests/stokes_cases.py and tests/stokes_response_cases.py: their columns, patterns, fields and host library.

`FitHostLib` is liblsx_fit_host.so (make fithost): lsx_fit_dev.h compiled for the CPU without contraction.
`yardstick` evaluates chi2, grad and hess in numpy longdouble from a response and a Stokes vector handed over, together with the same
sums with every term replaced by its absolute value.  The bar of an entry is (M + 2 Nspace + 8) u times that absolute sum: the
forward bound of a sum of M products of sums of Nspace products (Higham, Accuracy and Stability, 3.1 and 3.5; with or without fused
multiply-adds), u = 2^-53.  SIGNAL: in every case the largest |grad| is at least SIGNAL x its bar.
`HostBackend` has the three methods drivers.fit_field_columns asks of a backend, on the host libraries: the CPU tests run the same loop.
`recovery` is the set-up of the loop's test: the spectrum of a field that is linear in depth, to be recovered from hat nodes."""
import ctypes as C
import os
import subprocess

import numpy as np

import stokes_cases as sc
import stokes_response_cases as rc
from lightspinner_amd import fit

U = sc.U
SIGNAL = 1000.0
LD = np.longdouble
_dp, _ip = sc._dp, sc._ip
same = lambda a, b: np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))

# the shapes of the issue: node counts, windows, angles
NNODES = [(1, 0, 0), (0, 2, 0), (2, 2, 2), (3, 3, 3), (8, 8, 8)]
WINDOWS = [(0, 1), (7, 1), (0, 63), (7, 63), (0, 64), (7, 64), (0, 65), (7, 65), (0, 130), (7, 130)]
MUS = np.array([1.0, 0.1, 0.6])
AMPS = {'B': 1e-3, 'gammaB': 1e-3, 'chiB': 1e-3}


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


class FitHostLib:
    """liblsx_fit_host.so: lsx_fit_dev.h compiled for the CPU"""

    def __init__(self):
        subprocess.check_call(['make', '-s', '-C', sc.CSRC, 'fithost'])
        self.dll = d = C.CDLL(os.path.join(sc.CSRC, 'liblsx_fit_host.so'))
        d.lsx_fit_host_expand.argtypes = [C.c_int32, C.c_int32, _ip, _dp, _dp, _dp, _dp]
        d.lsx_fit_host_normal.argtypes = [C.c_int32, C.c_int32, C.c_int32, _ip, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]
        d.lsx_fit_host_step.argtypes = [C.c_int32, C.c_int32, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _ip, _dp]
        for f in (d.lsx_fit_host_expand, d.lsx_fit_host_normal, d.lsx_fit_host_step):
            f.restype = C.c_int

    def expand(self, Ns, nnode, basis, base, nodes):
        """-> field [ncol][3][Ns]"""
        nn = np.ascontiguousarray(nnode, dtype=np.int32)
        x = sc._d(np.atleast_2d(nodes))
        bs = None if base is None else sc._d(np.broadcast_to(base, (x.shape[0], 3, Ns)))
        out = np.empty((x.shape[0], 3, Ns))
        rc_ = self.dll.lsx_fit_host_expand(Ns, x.shape[0], nn.ctypes.data_as(_ip), _p(sc._d(basis)), _p(bs), _p(x), _p(out))
        assert rc_ == sc.LSX_OK, rc_
        return out

    def normal(self, nnode, rf, S, obs, weight, basis, chi2_only=False):
        """one column: rf [npar][4][nla][Ns][nmu] (None with chi2_only), S, obs, weight [4][nla][nmu] -> (chi2, grad, hess)"""
        nn = np.ascontiguousarray(nnode, dtype=np.int32)
        P = int(nn.sum())
        S = sc._d(S)
        _, nla, nmu = S.shape
        Ns = np.asarray(basis).shape[-1]
        chi2, grad, hess = np.empty(1), np.full(P, np.nan), np.full((P, P), np.nan)
        w = None if weight is None else sc._d(np.broadcast_to(weight, S.shape))
        rf_ = None if chi2_only else sc._d(rf)
        assert rf_ is None or rf_.shape == (int((nn > 0).sum()), 4, nla, Ns, nmu), rf_.shape
        rc_ = self.dll.lsx_fit_host_normal(Ns, nla, nmu, nn.ctypes.data_as(_ip), _p(rf_), _p(S), _p(sc._d(obs)), _p(w), _p(sc._d(basis)),
                                           _p(chi2), None if chi2_only else _p(grad), None if chi2_only else _p(hess))
        assert rc_ == sc.LSX_OK, rc_
        return chi2[0], grad, hess

    def step(self, hess, grad, lam, nodes, lo=None, hi=None):
        """-> (trial, predicted, status, delta)"""
        g = sc._d(np.atleast_2d(grad))
        nc, P = g.shape
        H = sc._d(np.asarray(hess).reshape(nc, P, P))
        x = sc._d(np.broadcast_to(nodes, (nc, P)))
        lm = sc._d(np.broadcast_to(lam, (nc,)))
        lo_ = sc._d(np.broadcast_to(-np.inf if lo is None else lo, (P,)))
        hi_ = sc._d(np.broadcast_to(np.inf if hi is None else hi, (P,)))
        trial, pred, delta, st = np.empty((nc, P)), np.empty(nc), np.empty((nc, P)), np.empty(nc, dtype=np.int32)
        rc_ = self.dll.lsx_fit_host_step(nc, P, _p(H), _p(g), _p(lm), _p(x), _p(lo_), _p(hi_), _p(trial), _p(pred), st.ctypes.data_as(_ip),
                                         _p(delta))
        assert rc_ == sc.LSX_OK, rc_
        return trial, pred, st, delta


# ---- the parameterisation of the tests ---------------------------------------------------------------------------------------------
def basis_of(Ns, nnode):
    """hat functions over the depth index, the nodes spread evenly -> [P][Ns]"""
    rows = [fit.hat_basis(np.arange(Ns), np.linspace(0, Ns - 1, n) if n > 1 else [0.0]) for n in nnode if n > 0]
    return np.concatenate(rows, axis=0)


def nodes_of(fld, Ns, nnode, base=None):
    """the node values that make a field linear in depth ([ncol][Ns] per parameter: stokes_cases.field) exactly, minus `base`:
    the field's values at the nodes' depths -> [ncol][P]"""
    out = []
    for p, n in enumerate(nnode):
        if n == 0:
            continue
        f = fld[p] - (0.0 if base is None else base[:, p])
        d = np.arange(Ns)
        at = np.linspace(0, Ns - 1, n) if n > 1 else np.array([0.5 * (Ns - 1)])
        out.append(np.stack([np.interp(at, d, f[c]) for c in range(f.shape[0])]))
    return np.concatenate(out, axis=1)


def off_truth(nodes, nnode):
    """the start of the issue: B nodes x 1.25, gammaB + 0.15, chiB - 0.2"""
    x = np.array(nodes, dtype=np.float64)
    o = np.cumsum([0] + list(nnode))
    x[:, o[0]:o[1]] *= 1.25
    x[:, o[1]:o[2]] += 0.15
    x[:, o[2]:o[3]] -= 0.2
    return x


def base_of(fld, nnode, given):
    """base [ncol][3][Ns]: the parameters without nodes need their field there; with `given` the fitted ones get 0.3 of theirs too"""
    b = np.stack([np.where(n == 0, 1.0, 0.3 if given else 0.0) * f for n, f in zip(nnode, fld)], axis=1)
    return sc._d(b)


def weights_of(kind, shape, seed=3):
    """None, 'given' (positive, uneven, a sprinkle of zeros) or 'masked' (Q and U zeroed whole)"""
    if kind is None:
        return None
    w = 0.5 + np.random.default_rng(seed).uniform(0.0, 1.0, shape)
    w.reshape(-1)[::7] = 0.0
    if kind == 'masked':
        w[:, 1:3] = 0.0
    return w


# ---- the yardstick -----------------------------------------------------------------------------------------------------------------
def yardstick(nnode, rf, S, obs, weight, basis):
    """rf [ncol][npar][4][nla][Ns][nmu], S, obs, weight [ncol][4][nla][nmu] -> dicts value, bar with 'chi2' [ncol], 'grad' [ncol][P],
    'hess' [ncol][P][P]; value in longdouble, bar = (M + 2 Ns + 8) u x the sum of the terms' absolute values"""
    rf, S, obs = (np.asarray(a, dtype=LD) for a in (rf, S, obs))
    ncol, _, _, nla, Ns, nmu = rf.shape
    M = 4 * nla * nmu
    w = np.ones(S.shape, dtype=LD) if weight is None else np.broadcast_to(np.asarray(weight, dtype=LD), S.shape)
    r = np.where(w > 0, obs - S, LD(0))
    rows, i = [], 0
    for n in nnode:
        rows += [i] * n
        i += n > 0
    b = np.asarray(basis, dtype=LD)
    J = np.stack([np.einsum('cslkm,k->cslm', rf[:, rows[j]], b[j]) for j in range(len(rows))], axis=1).reshape(ncol, len(rows), M)
    Ja = np.stack([np.einsum('cslkm,k->cslm', np.abs(rf[:, rows[j]]), np.abs(b[j])) for j in range(len(rows))], axis=1).reshape(ncol, len(rows), M)
    w, r = w.reshape(ncol, M), r.reshape(ncol, M)
    val = {'chi2': np.sum(w * r * r, axis=1), 'grad': np.einsum('cjd,cd->cj', J, w * r), 'hess': np.einsum('cad,cbd,cd->cab', J, J, w)}
    f = LD((M + 2 * Ns + 8) * U)
    bar = {'chi2': f * np.sum(np.abs(w * r * r), axis=1), 'grad': f * np.einsum('cjd,cd->cj', Ja, np.abs(w * r)),
           'hess': f * np.einsum('cad,cbd,cd->cab', Ja, Ja, w)}
    return val, bar


def inside(x, val, bar):
    """-> the largest |x - value| / bar per quantity (<= 1: inside); 0 / 0 counts as inside"""
    out = {}
    for k in ('chi2', 'grad', 'hess'):
        dev = np.abs(np.asarray(x[k], dtype=LD) - val[k])
        with np.errstate(divide='ignore', invalid='ignore'):
            out[k] = float(np.max(np.where(bar[k] > 0, dev / bar[k], np.where(dev > 0, np.inf, 0.0))))
    return out


def grad_signal(val, bar):
    return float(np.max(np.abs(val['grad'])) / np.max(bar['grad']))


def step_checks(P, hess, grad, lam, nodes, lo, hi, trial, predicted, delta):
    """one column's step against its definitions in longdouble -> (backward error / (P (3 P + 1) u), trial == clip(nodes + delta),
    |predicted - definition| / (its absolute sum x (2 P + 4) u))"""
    H, g, d0 = (np.asarray(a, dtype=LD) for a in (hess, grad, delta))
    A = H + LD(lam) * np.diag(np.diag(H))
    res = np.max(np.abs(g - A @ d0)) / (np.max(np.sum(np.abs(A), axis=1)) * np.max(np.abs(d0)) + np.max(np.abs(g)))
    t = np.clip(np.asarray(nodes) + np.asarray(delta), lo, hi)
    d = np.asarray(trial, dtype=LD) - np.asarray(nodes, dtype=LD)
    pred = 2 * (d @ g) - d @ H @ d
    pabs = 2 * (np.abs(d) @ np.abs(g)) + np.abs(d) @ np.abs(H) @ np.abs(d)
    return float(res / (P * (3 * P + 1) * U)), np.array_equal(t, trial), float(np.abs(LD(predicted) - pred) / (pabs * (2 * P + 4) * U))


# ---- a backend on the host libraries -------------------------------------------------------------------------------------------------
class HostBackend:
    """fit_field_normal, fit_field_chi2, fit_field_step as Engine has them, from stokes_response_cases.HostLib (the response and the
    Stokes window of a Column) and FitHostLib.  The call's keywords the host does not need (col0, ncol: all columns) are refused."""

    def __init__(self, host, fithost, prob, block, prof, n, J, patterns, la0, nla):
        self.host, self.fh, self.args, self.patterns, self.la0, self.nla = host, fithost, (prob, block, prof, n, J), patterns, la0, nla
        self.Ns, self.ncol = prob.Nspace, block.ncol
        self.calls = {'normal': 0, 'chi2': 0, 'step': 0}

    def _columns(self, field):
        fld = [sc._d(field[:, p]) for p in range(3)]
        return [sc.column(*self.args, fld, self.patterns, c, self.la0, self.nla) for c in range(self.ncol)]

    def response(self, field, mus, nnode, amplitudes):
        """-> rf [ncol][npar][4][nla][Ns][nmu], S [ncol][4][nla][nmu]"""
        names = [p for p, n in zip(rc.PARAMS, nnode) if n > 0]
        rf, S = [], []
        for col in self._columns(field):
            per = [self.host.response(col, mu, parameters=names, amplitudes=amplitudes) for mu in mus]
            rf.append(np.stack([np.stack([r[0][p] for r in per], axis=-1) for p in names]))
            S.append(np.stack([r[1] for r in per], axis=-1))
        return np.stack(rf), np.stack(S)

    def fit_field_normal(self, mus, basis, nnode, nodes, obs, weight=None, base=None, amplitudes=None):
        self.calls['normal'] += 1
        field = self.fh.expand(self.Ns, nnode, basis, base, nodes)
        rf, S = self.response(field, np.atleast_1d(mus), nnode, dict(AMPS, **(amplitudes or {})))
        w = None if weight is None else np.broadcast_to(weight, S.shape)
        out = [self.fh.normal(nnode, rf[c], S[c], obs[c], None if w is None else w[c], basis) for c in range(self.ncol)]
        return fit.FieldNormal(np.array([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]), field)

    def fit_field_chi2(self, mus, basis, nnode, nodes, obs, weight=None, base=None):
        self.calls['chi2'] += 1
        field = self.fh.expand(self.Ns, nnode, basis, base, nodes)
        S = np.stack([np.stack([self.host.window(col, mu) for mu in np.atleast_1d(mus)], axis=-1) for col in self._columns(field)])
        w = None if weight is None else np.broadcast_to(weight, S.shape)
        return np.array([self.fh.normal(nnode, None, S[c], obs[c], None if w is None else w[c], basis, chi2_only=True)[0]
                         for c in range(self.ncol)]), field

    def fit_field_step(self, hess, grad, lam, nodes, lo=None, hi=None):
        self.calls['step'] += 1
        return self.fh.step(hess, grad, lam, nodes, lo, hi)[:3]


# ---- the loop's test ------------------------------------------------------------------------------------------------------------------
RECOVERY_WINDOW = (52, 44)                     # [52, 96)
RECOVERY_CASES = [(13, 2, [1.0]), (13, 2, [1.0, 0.6]), (5, 2, [1.0]), (13, 3, [1.0])]         # Ns, nodes per parameter, angles
RECOVERY_LOOP = dict(lambda0=1e-2, factor=10.0, max_iter=12)


def recovery(Ns, ncol, nn):
    """-> (problem parts, patterns, truth field, nnode, basis, true nodes, start nodes)"""
    parts = sc.problem(Ns, ncol, vlos=True)
    fld = sc.field(Ns, ncol, 'inclined')
    nnode = (nn, nn, nn)
    truth = nodes_of(fld, Ns, nnode)
    return parts, sc.PATTERN_SETS['blend'], fld, nnode, basis_of(Ns, nnode), truth, off_truth(truth, nnode)


def recovery_weight(obs):
    """1 / (1e-3 max I)^2 per column"""
    return np.broadcast_to((1.0 / (1e-3 * obs[:, 0].max(axis=(1, 2))) ** 2)[:, None, None, None], obs.shape).copy()


def check_recovery(r, truth, max_iter=12):
    """the conditions of the loop's test on a fit.FieldFit"""
    assert np.all(r.status == fit.CONVERGED) and np.all(r.iterations <= max_iter), (r.status, r.iterations)
    assert np.all(r.chi2 <= 1e-8 * r.history[0]), (r.chi2, r.history[0])
    assert np.max(np.abs(r.nodes - truth)) <= 1e-6, np.max(np.abs(r.nodes - truth))
    assert np.all(np.diff(r.history, axis=0) <= 0), r.history
    assert np.array_equal(r.history[-1], r.chi2)
