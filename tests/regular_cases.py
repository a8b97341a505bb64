"""What the tests of the regularised fit and of the nodes' uncertainties share (tests/test_fit_regular_host.py, tests/test_fit_regular.py;
include/lsx_hip_fit_regular.h).  Built on tests/fit_cases.py and tests/stokes_cases.py.

`RegularHostLib` is liblsx_fit_regular_host.so (make fitregularhost): lsx_fit_regular_dev.h compiled for the CPU without contraction,
with the two methods of Engine (fit_field_penalty, fit_field_uncertainty).  `HostBackend` is fit_cases.HostBackend with those two.
`penalty_yardstick` evaluates chi2 + penalty, grad + L^T rho and hess + L^T L in numpy longdouble, together with the same expressions
with every term replaced by its absolute value -- the value handed in counts as a term, and |target| + sum |L| |x| stands in the place
of |rho|: rho cancels (DESIGN.md 4.25 has the reasoning for the instrument's residual).  The bar is (Q + 2 P + 8) u times that: a sum
of Q products of sums of P products, plus the value handed in (Higham, Accuracy and Stability, 3.1 and 3.5).
`uncertainty_checks` holds one column of fit_field_uncertainty against its definitions:
  ainv    every column j by the backward error of fit_cases.step_checks with grad = e_j, lambda = 0: bar P (3 P + 1) u
  cov     against longdouble from the RETURNED ainv and the hess handed in: (2 P + 4) u x the absolute sum (two nested sums of P
          products and the scale)
  sigma   sigma^2 within 2 u of diag(cov) (one correctly rounded square root)
  band    field_sigma^2 against the quadratic form in longdouble from the RETURNED cov: (2 n + 6) u x the absolute sum, n the
          parameter's node count (two nested sums of n products, the square root)
`noisy` is the case of the issue: six B nodes on noisy profiles, with and without a smoothness penalty."""
import ctypes as C
import os
import subprocess

import numpy as np

import fit_cases as fc
import stokes_cases as sc
from lightspinner_amd import _capi, drivers, fit

U, LD = fc.U, fc.LD
_dp, _ip = sc._dp, sc._ip
same = fc.same
ALPHA = (1e6, 1e2, 1e2)                # the issue's: T^-2, rad^-2, rad^-2


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


class RegularHostLib:
    """liblsx_fit_regular_host.so: lsx_fit_regular_dev.h compiled for the CPU"""

    def __init__(self):
        subprocess.check_call(['make', '-s', '-C', sc.CSRC, 'fitregularhost'])
        self.dll = d = C.CDLL(os.path.join(sc.CSRC, 'liblsx_fit_regular_host.so'))
        pen = C.POINTER(_capi.LsxFitPenalty)
        d.lsx_fit_regular_host_penalty.argtypes = [C.c_int32, C.c_int32, pen, _dp, _dp, _dp, _dp, _dp]
        d.lsx_fit_regular_host_uncertainty.argtypes = [C.c_int32, C.c_int32, _dp, pen, _dp, C.c_int32, _ip, _dp, C.c_int32, _dp, _dp, _dp, _dp, _ip]
        for f in (d.lsx_fit_regular_host_penalty, d.lsx_fit_regular_host_uncertainty):
            f.restype = C.c_int

    @staticmethod
    def _pen(penalty, ncol, with_target=True):
        L = sc._d(penalty.L)
        tg = penalty.targets(ncol) if with_target else None
        return _capi.LsxFitPenalty(penalty.nrow, _p(L), _p(tg)), (L, tg)

    def fit_field_penalty(self, nodes, penalty, chi2, grad=None, hess=None):
        x = sc._d(np.atleast_2d(nodes))
        nc, P = x.shape
        st, keep = self._pen(penalty, nc)
        c = np.array(np.broadcast_to(chi2, (nc,)), dtype=np.float64)
        g = None if grad is None else np.array(np.asarray(grad).reshape(nc, P), dtype=np.float64)
        H = None if hess is None else np.array(np.asarray(hess).reshape(nc, P, P), dtype=np.float64)
        pen = np.empty(nc)
        rc_ = self.dll.lsx_fit_regular_host_penalty(nc, P, C.byref(st), _p(x), _p(c), _p(g), _p(H), _p(pen))
        assert rc_ == sc.LSX_OK, rc_
        return c, g, H, pen

    def fit_field_uncertainty(self, hess, basis, nnode, penalty=None, scale=None):
        H = sc._d(np.asarray(hess))
        H = H[None] if H.ndim == 2 else H
        nc, P = H.shape[:2]
        nn = np.ascontiguousarray(nnode, dtype=np.int32)
        bas = sc._d(np.atleast_2d(basis))
        st, keep = (None, None) if penalty is None else self._pen(penalty, nc, False)
        s = None if scale is None else sc._d(np.broadcast_to(scale, (nc,)))
        ai, cov, sg, fs = np.empty((nc, P, P)), np.empty((nc, P, P)), np.empty((nc, P)), np.empty((nc, nn.shape[0], bas.shape[1]))
        status = np.empty(nc, dtype=np.int32)
        rc_ = self.dll.lsx_fit_regular_host_uncertainty(nc, P, _p(H), None if st is None else C.byref(st), _p(s), nn.shape[0],
                                                        nn.ctypes.data_as(_ip), _p(bas), bas.shape[1], _p(ai), _p(cov), _p(sg), _p(fs),
                                                        status.ctypes.data_as(_ip))
        assert rc_ == sc.LSX_OK, rc_
        return fit.FieldUncertainty(ai, cov, sg, fs, status, nn)


class HostBackend(fc.HostBackend):
    """fit_cases.HostBackend with fit_field_penalty and fit_field_uncertainty from RegularHostLib"""

    def __init__(self, reghost, *a):
        super().__init__(*a)
        self.reg = reghost
        self.calls.update(penalty=0, uncertainty=0)

    def fit_field_penalty(self, *a, **kw):
        self.calls['penalty'] += 1
        return self.reg.fit_field_penalty(*a, **kw)

    def fit_field_uncertainty(self, *a, **kw):
        self.calls['uncertainty'] += 1
        return self.reg.fit_field_uncertainty(*a, **kw)


def regular(backend, reghost):
    """any other host backend (the instrument's, the velocity's) with the two methods attached"""
    backend.calls.update(penalty=0, uncertainty=0)

    def penalty(*a, **kw):
        backend.calls['penalty'] += 1
        return reghost.fit_field_penalty(*a, **kw)

    def uncertainty(*a, **kw):
        backend.calls['uncertainty'] += 1
        return reghost.fit_field_uncertainty(*a, **kw)

    backend.fit_field_penalty, backend.fit_field_uncertainty = penalty, uncertainty
    return backend


# ---- the penalty entry -----------------------------------------------------------------------------------------------------------------
PENALTY_P = [1, 2, 12, 13, 24]
rows_of = lambda P: sorted({1, P, 96})


def penalty_case(P, Q, ncol, with_target, seed=5):
    """-> (fit.Penalty with made-up finite rows of mixed signs, nodes [ncol][P])"""
    rng = np.random.default_rng(seed + 1000 * P + Q)
    L = rng.normal(size=(Q, P)) * 10.0 ** rng.uniform(-2, 2, size=(Q, 1))
    tg = rng.normal(size=(ncol, Q)) if with_target else None
    return fit.Penalty(L, tg), rng.normal(size=(ncol, P))


def spread(ne, ncol, seed=9):
    """one column's (chi2, grad, hess) of the fit -> ncol columns, each scaled by its own factor"""
    f = np.random.default_rng(seed).uniform(0.5, 2.0, ncol)
    return ne.chi2[0] * f, ne.grad[0][None] * f[:, None], ne.hess[0][None] * f[:, None, None]


def penalty_yardstick(penalty, nodes, chi2, grad, hess):
    """-> dicts value, bar with 'chi2', 'penalty' [ncol], 'grad' [ncol][P], 'hess' [ncol][P][P]"""
    L, x = np.asarray(penalty.L, dtype=LD), np.asarray(nodes, dtype=LD)
    nc, (Q, P) = x.shape[0], L.shape
    t = np.zeros((nc, Q), dtype=LD) if penalty.target is None else np.asarray(penalty.targets(nc), dtype=LD)
    rho, rabs = t - x @ L.T, np.abs(t) + np.abs(x) @ np.abs(L).T
    c, g, H = (np.asarray(a, dtype=LD) for a in (chi2, grad, hess))
    val = {'penalty': np.sum(rho * rho, axis=1), 'grad': g + rho @ L, 'hess': H + (L.T @ L)[None]}
    val['chi2'] = c + val['penalty']
    f = LD((Q + 2 * P + 8) * U)
    bar = {'penalty': f * np.sum(rabs * rabs, axis=1), 'grad': f * (np.abs(g) + rabs @ np.abs(L)), 'hess': f * (np.abs(H) + (np.abs(L).T @ np.abs(L))[None])}
    bar['chi2'] = f * (np.abs(c) + np.sum(rabs * rabs, axis=1))
    return val, bar


def inside(x, val, bar):
    """-> the largest |x - value| / bar per quantity (<= 1: inside); 0 / 0 counts as inside"""
    out = {}
    for k in x:
        dev = np.abs(np.asarray(x[k], dtype=LD) - val[k])
        with np.errstate(divide='ignore', invalid='ignore'):
            out[k] = float(np.max(np.where(bar[k] > 0, dev / bar[k], np.where(dev > 0, np.inf, 0.0))))
    return out


def check_penalty(be, penalty, nodes, chi2, grad, hess):
    """every statement of the penalty entry on one call of backend `be` -> the worst deviation / bar per quantity"""
    c, g, H, pen = be.fit_field_penalty(nodes, penalty, chi2, grad, hess)
    val, bar = penalty_yardstick(penalty, nodes, chi2, grad, hess)
    x = inside(dict(chi2=c, grad=g, hess=H, penalty=pen), val, bar)
    assert max(x.values()) <= 1.0, x
    c2, g2, H2, pen2 = be.fit_field_penalty(nodes, penalty, chi2)
    assert g2 is None and H2 is None and same(c2, c) and same(pen2, pen)                  # the chi2 of a trial
    assert same(H, np.swapaxes(H, 1, 2))
    nc = nodes.shape[0]
    for col in sorted({0, nc // 2, nc - 1}):                                               # a column alone
        one = fit.Penalty(penalty.L, None if penalty.target is None else penalty.targets(nc)[col:col + 1])
        c1, g1, H1, p1 = be.fit_field_penalty(nodes[col:col + 1], one, chi2[col:col + 1], grad[col:col + 1], hess[col:col + 1])
        assert same(c1[0], c[col]) and same(g1[0], g[col]) and same(H1[0], H[col]) and same(p1[0], pen[col]), col
    return x


def check_linear_nodes_cost_nothing(be, ne):
    """dyadic nodes linear in the node index, order-2 rows with alpha = 1: the penalty is 0.0, chi2 and grad keep their bits"""
    nnode = (8, 8, 8)
    pen = fit.Penalty.smoothness(nnode, (1.0, 1.0, 1.0), order=2)
    assert pen.nrow == 18
    nodes = np.stack([np.concatenate([a + b * np.arange(8.0) for a, b in ((0.25, 0.125), (1.5, -0.0625), (-2.0, 0.5))]),
                      np.concatenate([a + b * np.arange(8.0) for a, b in ((3.0, 0.0), (-0.75, 0.25), (0.0, -1.0))])])
    chi2, grad, hess = spread(ne, 2)
    c, g, H, p = be.fit_field_penalty(nodes, pen, chi2, grad, hess)
    assert np.all(p == 0.0) and same(c, chi2) and same(g, grad) and not same(H, hess)


# ---- the uncertainty entry -------------------------------------------------------------------------------------------------------------
def systems_call(nnode, Ns=13):
    """the recipe of tests/test_fit_host.py's _systems: -> what a backend's fit_field_normal is asked at the start of the recovery
    (problem parts, patterns, basis, base, start nodes, truth nodes)"""
    parts = sc.problem(Ns, 1, vlos=True)
    fld = sc.field(Ns, 1)
    basis, base = fc.basis_of(Ns, nnode), fc.base_of(fld, nnode, False)
    truth = fc.nodes_of(fld, Ns, nnode, base)
    return parts, sc.PATTERN_SETS['blend'], basis, base, fc.off_truth(truth, nnode), truth


def smoothness_or_none(nnode):
    return fit.Penalty.smoothness(nnode, ALPHA[:len(nnode)] if len(nnode) == 3 else ALPHA + (1e-4,), order=2) if max(nnode) >= 3 else None


def uncertainty_checks(hess, penalty, scale, basis, nnode, unc, c=0):
    """one column of a FieldUncertainty against its definitions -> dict of the worst deviation / bar: 'ainv', 'cov', 'sigma', 'band'"""
    P = hess.shape[-1]
    H = np.tril(hess) + np.tril(hess, -1).T                                                 # the lower triangle is read
    Hl = np.asarray(H, dtype=LD)
    A = Hl if penalty is None else Hl + np.asarray(penalty.L, dtype=LD).T @ np.asarray(penalty.L, dtype=LD)
    X = np.asarray(unc.ainv[c], dtype=LD)
    out = {'ainv': 0.0}
    for j in range(P):
        e = np.zeros(P)
        e[j] = 1.0
        be_, ok, _ = fc.step_checks(P, A, e, 0.0, np.zeros(P), -np.inf, np.inf, unc.ainv[c][:, j], 0.0, unc.ainv[c][:, j])
        assert ok
        out['ainv'] = max(out['ainv'], be_)
    s = LD(1.0 if scale is None else scale)
    if penalty is None:
        assert same(np.tril(unc.cov[c]), np.tril(unc.ainv[c]) * float(s)) if scale is not None else same(np.tril(unc.cov[c]), np.tril(unc.ainv[c]))
        out['cov'] = 0.0
    else:
        ref, ab = s * (X.T @ Hl @ X), s * (np.abs(X).T @ np.abs(Hl) @ np.abs(X))
        out['cov'] = float(np.max(np.abs(np.asarray(unc.cov[c], dtype=LD) - ref) / (ab * LD((2 * P + 4) * U))))
    assert same(unc.cov[c], unc.cov[c].T)
    d = np.asarray(np.diag(unc.cov[c]), dtype=LD)
    out['sigma'] = float(np.max(np.abs(np.asarray(unc.sigma[c], dtype=LD) ** 2 - d) / (d * LD(2 * U))))
    out['band'] = 0.0
    cv, b = np.asarray(unc.cov[c], dtype=LD), np.asarray(basis, dtype=LD)
    o = 0
    for p, n in enumerate(nnode):
        if n == 0:
            assert np.all(unc.field_sigma[c][p] == 0.0)
            continue
        blk, bp = cv[o:o + n, o:o + n], b[o:o + n]
        ref, ab = np.einsum('nk,nm,mk->k', bp, blk, bp), np.einsum('nk,nm,mk->k', np.abs(bp), np.abs(blk), np.abs(bp))
        dev = np.abs(np.asarray(unc.field_sigma[c][p], dtype=LD) ** 2 - ref)
        out['band'] = max(out['band'], float(np.max(dev / (ab * LD((2 * n + 6) * U)))))
        o += n
    return out


def check_uncertainty(be, hess, basis, nnode, ncol=1):
    """every statement of the uncertainty entry for one system of the fit, repeated over ncol columns with a factor each; with the three
    bad systems among them where ncol allows -> the worst deviation / bar per quantity"""
    f = np.random.default_rng(4).uniform(0.5, 2.0, ncol)
    H = hess[None] * f[:, None, None]
    P = H.shape[-1]
    worst = {}
    pen = smoothness_or_none(nnode)
    scale = np.random.default_rng(6).uniform(0.5, 3.0, ncol)
    cols = sorted({0, ncol // 2, ncol - 1})
    for penalty in ([None] if pen is None else [None, pen]):
        plain = be.fit_field_uncertainty(H, basis, nnode, penalty=penalty)
        scaled = be.fit_field_uncertainty(H, basis, nnode, penalty=penalty, scale=scale)
        assert not plain.status.any() and not scaled.status.any()
        assert np.all(np.isfinite(plain.sigma)) and np.all(plain.sigma > 0)
        # the scale multiplies cov and nothing else
        assert same(scaled.ainv, plain.ainv) and same(scaled.cov, plain.cov * scale[:, None, None])
        for c in cols:
            for u, s in ((plain, None), (scaled, scale[c])):
                x = uncertainty_checks(H[c], penalty, s, basis, nnode, u, c)
                assert max(x.values()) <= 1.0, (c, x)
                worst = {k: max(v, worst.get(k, 0.0)) for k, v in x.items()}
            one = be.fit_field_uncertainty(H[c:c + 1], basis, nnode, penalty=penalty)          # a column alone
            assert all(same(getattr(one, k)[0], getattr(plain, k)[c]) for k in ('ainv', 'cov', 'sigma', 'field_sigma')), c
        # a singular, a NaN and an indefinite system among good ones (with a penalty the zero row and column is no longer singular)
        bad = {}
        if ncol >= 3:
            bad = {ncol // 3: 'nan', ncol - 1: 'negative'} if penalty is not None else {0: 'zero', ncol // 3: 'nan', ncol - 1: 'negative'}
        elif penalty is None:
            bad = {0: 'zero'}
        Hb = H.copy()
        for c, kind in bad.items():
            if kind == 'zero':
                Hb[c, -1, :] = Hb[c, :, -1] = 0.0
            elif kind == 'nan':
                Hb[c, 0, 0] = np.nan
            else:
                Hb[c, 0, 0] = -1e12 * abs(Hb[c, 0, 0]) - 1e12
        if ncol == 1 and bad:
            Hb = np.concatenate([Hb, H])                                                     # (a good one beside it)
            ref = be.fit_field_uncertainty(H, basis, nnode, penalty=penalty)
            r = be.fit_field_uncertainty(Hb, basis, nnode, penalty=penalty)
            assert list(r.status) == [1, 0] and all(np.all(np.isnan(getattr(r, k)[0])) for k in ('ainv', 'cov', 'sigma', 'field_sigma'))
            assert all(same(getattr(r, k)[1], getattr(ref, k)[0]) for k in ('ainv', 'cov', 'sigma', 'field_sigma'))
        elif bad:
            r = be.fit_field_uncertainty(Hb, basis, nnode, penalty=penalty)
            good = [c for c in range(ncol) if c not in bad]
            assert list(np.nonzero(r.status)[0]) == sorted(bad), r.status
            for k in ('ainv', 'cov', 'sigma', 'field_sigma'):
                assert np.all(np.isnan(getattr(r, k)[sorted(bad)])) and same(getattr(r, k)[good], getattr(plain, k)[good]), k
    return worst


# ---- the loop --------------------------------------------------------------------------------------------------------------------------
REGULAR_RECOVERY = [(13, 3, 1), (13, 3, 3), (5, 3, 1)]                   # Ns, nodes per parameter, columns: RECOVERY_CASES' (., 3, [1.0])
RECOVERY_ITERATIONS = 5                                                  # what the host loop takes (the issue)


def recovery_penalty(nn):
    return fit.Penalty.smoothness((nn, nn, nn), ALPHA, order=2)


# The pieces compose: through Instrument.gaussian (the instrument tests' set-up (a)) three nodes per parameter and the smoothness penalty;
# with four quantities (velocity_cases' first case) a prior on the vlos nodes, at the truth so that the minimum stays where it is.
# COMPOSE_ITERATIONS: what the host loop takes (tests/test_fit_regular_host.py asserts it); the engine may take two more
COMPOSE_ITERATIONS = {'instrument': 5, 'velocity': 5}


def velocity_prior(nnode, truth, vB):
    """the vlos nodes are expected at `truth` within 0.05 vBroad"""
    return fit.Penalty.prior(nnode, {'vlos': 1.0 / (0.05 * vB) ** 2}, truth)


NOISY = dict(Ns=13, ncol=3, nnode=(6, 2, 2), seed=11, loop=dict(tol=1e-9, max_iter=30))


def noisy_bounds(nnode):
    lo = np.concatenate([np.full(nnode[0], 1e-3), np.zeros(nnode[1]), np.full(nnode[2], -np.pi)])
    hi = np.concatenate([np.ones(nnode[0]), np.full(nnode[1], np.pi), np.full(nnode[2], np.pi)])
    return lo, hi


def noisy_setup():
    """-> (problem parts, patterns, truth field [3 x [ncol][Ns]], nnode, basis, true nodes, start nodes)"""
    Ns, ncol, nnode = NOISY['Ns'], NOISY['ncol'], NOISY['nnode']
    parts = sc.problem(Ns, ncol, vlos=True)
    fld = sc.field(Ns, ncol, 'inclined')
    truth = fc.nodes_of(fld, Ns, nnode)
    return parts, sc.PATTERN_SETS['blend'], fld, nnode, fc.basis_of(Ns, nnode), truth, fc.off_truth(truth, nnode)


def add_noise(clean):
    """Gaussian noise of sigma = 1e-3 max I per column -> (obs, weight = 1 / sigma^2)"""
    sigma = 1e-3 * clean[:, 0].max(axis=(1, 2))
    obs = clean + np.random.default_rng(NOISY['seed']).standard_normal(clean.shape) * sigma[:, None, None, None]
    return obs, np.broadcast_to((1.0 / sigma ** 2)[:, None, None, None], clean.shape).copy()


def noisy_fits(backend, obs, w, mus, basis, start, nnode, **call):
    """-> (the plain fit, the regularised fit), both with uncertainties"""
    lo, hi = noisy_bounds(nnode)
    kw = dict(weight=w, lo=lo, hi=hi, amplitudes=fc.AMPS, uncertainty=True, **NOISY['loop'], **call)
    plain = drivers.fit_field_columns(backend, obs, mus, basis, start, nnode, **kw)
    pen = fit.Penalty.smoothness(nnode, {'B': ALPHA[0]}, order=2)
    return plain, drivers.fit_field_columns(backend, obs, mus, basis, start, nnode, penalty=pen, **kw)


def check_noisy(plain, reg, truth, nnode, label):
    """the conditions of the issue's noisy case; prints iterations, errors and pulls"""
    nB = nnode[0]
    err = lambda r: np.max(np.abs(r.nodes[:, :nB] - truth[:, :nB]), axis=1)
    pull = lambda r: np.abs(r.nodes - truth) / r.uncertainty.sigma
    dof = plain.dof
    print('%s: plain fit %s iterations, chi2_data %s, B error %s T, largest pull %.3g, sigma of the deepest B node %s T'
          % (label, plain.iterations, plain.chi2_data, err(plain), pull(plain).max(), plain.uncertainty.sigma[:, nB - 1]))
    print('%s: regularised %s iterations, chi2_data %s, penalty %s, B error %s T (%s of the plain fit), largest pull %.3g'
          % (label, reg.iterations, reg.chi2_data, reg.penalty, err(reg), err(reg) / err(plain), pull(reg).max()))
    for r in (plain, reg):
        assert np.all(r.status == fit.CONVERGED), r.status
        assert np.all(np.diff(r.history, axis=0) <= 0), r.history
        assert np.array_equal(r.dof, dof) and np.all(np.abs(r.chi2_data - dof) <= 4 * np.sqrt(2.0 * dof)), (r.chi2_data, dof)
        assert not r.uncertainty.status.any() and np.all(pull(r) <= 4.0), pull(r)
        assert same(r.chi2, r.history[-1])
    assert np.all(plain.penalty == 0.0) and same(plain.chi2_data, plain.chi2)
    assert np.all(reg.penalty > 0.0) and np.max(np.abs(reg.chi2_data + reg.penalty - reg.chi2)) <= 4 * U * np.max(reg.chi2)
    assert np.all(err(reg) < err(plain)), (err(reg), err(plain))
