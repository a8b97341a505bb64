"""The regularised fit and the nodes' uncertainties on the CPU (include/lsx_hip_fit_regular.h): fit.Penalty; lsx_fit_regular_dev.h compiled
into liblsx_fit_regular_host.so (make fitregularhost) against numpy longdouble inside rounding bounds (tests/regular_cases.py has them
and their reasons); drivers.fit_field_columns with a penalty and with uncertainties on the host backend -- the noise-free recovery
unchanged, the issue's noisy case; the sanitizer program; names and the compiler's report."""
import os
import re
import subprocess

import numpy as np
import pytest

import fit_cases as fc
import regular_cases as rg
import stokes_cases as sc
import stokes_response_cases as rc
from lightspinner_amd import drivers, fit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD, U = fc.LD, fc.U


@pytest.fixture(scope='module')
def host():
    return rc.HostLib()


@pytest.fixture(scope='module')
def fithost():
    return fc.FitHostLib()


@pytest.fixture(scope='module')
def reghost():
    return rg.RegularHostLib()


@pytest.fixture(scope='module')
def systems(host, fithost):
    """nnode -> (the fit's normal equations at the start of the recovery, basis): one host response per shape for the whole module"""
    out = {}
    for nnode in fc.NNODES:
        (prob, block, prof, J), pats, basis, base, nodes, truth = rg.systems_call(nnode)
        be = fc.HostBackend(host, fithost, prob, block, prof, block.n, J, pats, *fc.RECOVERY_WINDOW)
        _, obs = be.response(fithost.expand(13, nnode, basis, base, truth), fc.MUS[:1], nnode, fc.AMPS)
        out[nnode] = (be.fit_field_normal(fc.MUS[:1], basis, nnode, nodes, obs, weight=fc.recovery_weight(obs), base=base), basis)
    return out


# ---- 1. fit.Penalty ---------------------------------------------------------------------------------------------------------------------
def test_penalty_rows():
    even, uneven = np.arange(5.0), np.array([0.0, 0.3, 1.7, 2.0, 9.5])
    for t in (None, even, uneven):
        pos = None if t is None else {'B': t, 'chiB': t[:4]}
        p1 = fit.Penalty.smoothness((5, 2, 4), {'B': 4.0, 'gammaB': 1.0, 'chiB': 0.25}, order=1, positions=pos)
        assert p1.L.shape == (4 + 1 + 3, 11) and p1.target is None and p1.nrow == 8 and p1.nparam == 11
        assert np.all(p1.L.sum(axis=1) == 0.0) and np.all((p1.L * 0.7).sum(axis=1) == 0.0)                   # constants, exactly: a row is (-w, w)
        assert np.count_nonzero(p1.L) == 16
        p2 = fit.Penalty.smoothness((5, 2, 4), {'B': 4.0, 'gammaB': 1.0, 'chiB': 0.25}, order=2, positions=pos)
        assert p2.L.shape == (3 + 0 + 2, 11) and np.count_nonzero(p2.L) == 15
        tt = even if t is None else t
        x = np.concatenate([0.3 - 1.7 * tt, [5.0, -4.0], 2.5 + 0.4 * tt[:4]])                                 # linear in the positions
        Lx, Labs = np.asarray(p2.L, dtype=LD) @ np.asarray(x, dtype=LD), np.abs(p2.L).astype(LD) @ np.abs(x).astype(LD)
        assert np.all(np.abs(Lx) <= 4 * U * Labs), np.abs(Lx) / (U * Labs)
        assert np.max(np.abs(p2.L @ np.r_[tt ** 2, 0.0, 0.0, np.zeros(4)] - 2.0 * 2.0 * np.r_[1, 1, 1, 0, 0])) < 1e-12     # sqrt(alpha) x''
    # positions as a SEQUENCE in the library's order, the parameters with different node counts: the rows of the dict form
    for tB, tg, tc in ((np.arange(4.0), np.arange(3.0), np.arange(3.0)), ([0.0, 1.0, 2.0, 4.0], [0.0, 1.0, 2.0], [0.0, 1.0, 3.0]),
                       (uneven[:4], (0.0, 0.25, 7.0), np.array([-3.0, 0.5, 0.75]))):
        for order in (1, 2):
            ps = fit.Penalty.smoothness((4, 3, 3), [1.0, 2.0, 3.0], order=order, positions=[tB, tg, tc])
            pd = fit.Penalty.smoothness((4, 3, 3), [1.0, 2.0, 3.0], order=order, positions={'B': tB, 'gammaB': tg, 'chiB': tc})
            assert ps.L.shape == ((3 + 2 + 2, 10) if order == 1 else (2 + 1 + 1, 10)) and np.array_equal(ps.L, pd.L)
            x = np.concatenate([1.0 + 0.5 * np.asarray(tB), 2.0 - 3.0 * np.asarray(tg), -0.25 * np.asarray(tc)])
            if order == 2:
                Lx, Labs = np.asarray(ps.L, dtype=LD) @ np.asarray(x, dtype=LD), np.abs(ps.L).astype(LD) @ np.abs(x).astype(LD)
                assert np.all(np.abs(Lx) <= 4 * U * Labs), np.abs(Lx) / (U * Labs)
            else:
                assert np.all(ps.L.sum(axis=1) == 0.0)
    short = fit.Penalty.smoothness((6, 2, 2), [1e6], positions=[np.array([0.0, 1.0, 3.0, 4.0, 7.0, 8.0])])   # the later entries missing
    assert short.L.shape == (4, 10)
    assert np.array_equal(fit.Penalty.smoothness((6, 2, 2), 1e6).L, fit.Penalty.smoothness((6, 2, 2), np.float64(1e6)).L)   # a scalar: B's
    assert np.array_equal(fit.Penalty.smoothness((3, 0, 0), [1.0]).L, [[1.0, -2.0, 1.0]])
    assert np.array_equal(fit.Penalty.smoothness((3, 0, 0), [4.0], order=1).L, [[-2.0, 2.0, 0.0], [0.0, -2.0, 2.0]])
    assert fit.Penalty.smoothness((3, 1, 1, 3), {'vlos': 1e-4}).L.shape == (1, 8)                             # the fourth quantity
    assert fit.Penalty.smoothness((3, 3, 3), (1.0, 0.0)).nrow == 1                                            # zero or missing: no rows
    pr = fit.Penalty.prior((2, 1, 1), {'B': 4.0, 'chiB': 9.0}, {'B': [0.1, 0.2], 'chiB': [0.5]})
    assert np.array_equal(pr.L, [[2.0, 0, 0, 0], [0, 2.0, 0, 0], [0, 0, 0, 3.0]]) and np.array_equal(pr.target, [0.2, 0.4, 1.5])
    pc = fit.Penalty.prior((2, 1, 1), (4.0,), np.array([[0.1, 0.2, 9, 9], [0.3, 0.4, 9, 9]]))
    assert pc.target.shape == (2, 2) and np.array_equal(pc.targets(2), [[0.2, 0.4], [0.6, 0.8]])
    st = fit.Penalty.stack(fit.Penalty.smoothness((2, 1, 1), [1.0], order=1), pc, pr)
    assert st.L.shape == (6, 4) and st.target.shape == (2, 6) and np.array_equal(st.target[1], [0.0, 0.6, 0.8, 0.2, 0.4, 1.5])
    assert fit.Penalty.stack(fit.Penalty([[1.0, 2.0]]), fit.Penalty([[3.0, 4.0]])).target is None
    assert np.array_equal(pr.targets(3), np.broadcast_to(pr.target, (3, 3)))


def test_penalty_refusals():
    for bad in (lambda: fit.Penalty(np.zeros((0, 3))), lambda: fit.Penalty(np.zeros((97, 3))), lambda: fit.Penalty(np.zeros((2, 25))),
                lambda: fit.Penalty([[np.nan]]), lambda: fit.Penalty([[1.0]], [np.inf]), lambda: fit.Penalty([[1.0]], [1.0, 2.0]),
                lambda: fit.Penalty([[1.0]], np.zeros((2, 2, 1))), lambda: fit.Penalty([[1.0]], [[1.0], [2.0]]).targets(3),
                lambda: fit.Penalty.smoothness((3, 3, 3), [1.0], order=3), lambda: fit.Penalty.smoothness((3, 3, 3), [-1.0]),
                lambda: fit.Penalty.smoothness((3, 3, 3), [np.nan]), lambda: fit.Penalty.smoothness((3, 3, 3), {'T': 1.0}),
                lambda: fit.Penalty.smoothness((3, 3, 3), {'vlos': 1.0}), lambda: fit.Penalty.smoothness((3, 3, 3), [1, 1, 1, 1]),
                lambda: fit.Penalty.smoothness((2, 2, 2), [1.0]), lambda: fit.Penalty.smoothness((3, 3, 3), [0.0]),
                lambda: fit.Penalty.smoothness((3, 0, 0), [1.0], positions=[[0.0, 1.0]]),
                lambda: fit.Penalty.smoothness((3, 0, 0), [1.0], positions=[[0.0, 1.0, 1.0]]),
                lambda: fit.Penalty.smoothness((9, 9, 9), [1.0]), lambda: fit.Penalty.smoothness((3, -1, 0), [1.0]),
                lambda: fit.Penalty.smoothness((3, 3), [1.0]), lambda: fit.Penalty.prior((2, 1, 1), [1.0], [1.0, 2.0]),
                lambda: fit.Penalty.prior((2, 1, 1), {'B': 1.0}, {'chiB': [1.0]}), lambda: fit.Penalty.prior((2, 1, 1), [0.0], np.zeros(4)),
                lambda: fit.Penalty.stack(), lambda: fit.Penalty.stack(fit.Penalty([[1.0]]), fit.Penalty([[1.0, 2.0]])),
                lambda: fit.Penalty.stack(fit.Penalty([[1.0]], np.zeros((2, 1))), fit.Penalty([[1.0]], np.zeros((3, 1))))):
        with pytest.raises(ValueError):
            bad()


# ---- 2. the penalty entry ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', rg.PENALTY_P)
def test_penalty_entry(reghost, systems, P):
    """P = 1, 2, 12, 13, 24; Q = 1, P, 96; target none and given; 1, 3 and 70 columns; on the fit's own sums (P of fit_cases.NNODES)
    and on zeros"""
    ne = {sum(nn): s[0] for nn, s in systems.items()}.get(P)
    worst = {}
    for Q in rg.rows_of(P):
        for ncol, with_target in ((1, False), (3, True), (70, True), (70, False)):
            pen, nodes = rg.penalty_case(P, Q, ncol, with_target)
            ins = [(np.zeros(ncol), np.zeros((ncol, P)), np.zeros((ncol, P, P)))] + ([rg.spread(ne, ncol)] if ne is not None else [])
            if ne is None:              # no system of the fit has this P: made-up symmetric sums of the fit's magnitudes
                r = np.random.default_rng(P)
                K = r.normal(size=(ncol, P, P)) * 1e3
                H = np.tril(K @ np.swapaxes(K, 1, 2))
                ins.append((r.uniform(1e2, 1e4, ncol), r.normal(size=(ncol, P)) * 1e4, H + np.swapaxes(np.tril(H, -1), 1, 2)))
            for chi2, grad, hess in ins:
                x = rg.check_penalty(reghost, pen, nodes, chi2, grad, hess)
                worst = {k: max(v, worst.get(k, 0.0)) for k, v in x.items()}
    print('penalty entry, host, P %d: worst deviation / bar %s' % (P, worst))


def test_linear_nodes_cost_nothing(reghost, systems):
    rg.check_linear_nodes_cost_nothing(reghost, systems[(8, 8, 8)][0])


# ---- 3. the uncertainty entry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nnode', fc.NNODES)
def test_uncertainty_entry(reghost, systems, nnode):
    """the fit's own systems, P = 1, 2, 6, 9, 24: without a penalty and with smoothness(order=2) where it has rows; alone, and five
    columns with a NaN, an indefinite and (without a penalty) a singular system among them"""
    ne, basis = systems[nnode]
    for ncol in (1, 5):
        worst = rg.check_uncertainty(reghost, ne.hess[0], basis, nnode, ncol)
        print('uncertainty entry, host, P %d, %d columns: worst deviation / bar %s' % (sum(nnode), ncol, worst))
    # four quantities, and a basis of another depth count than the fit's
    u = reghost.fit_field_uncertainty(ne.hess, basis[:, :3], tuple(nnode) + (0,))
    assert u.field_sigma.shape == (1, 4, 3) and np.all(u.field_sigma[0, 3] == 0.0) and u.parameter('vlos').shape == (1, 0)
    assert fc.same(u.parameter('B'), u.sigma[:, :nnode[0]])
    corr = u.correlation()
    assert np.max(np.abs(np.diagonal(corr, axis1=1, axis2=2) - 1.0)) <= 4 * U and np.all(np.abs(corr) <= 1.0 + 1e-12)


# ---- 4. the loop -----------------------------------------------------------------------------------------------------------------------------
def test_without_the_new_arguments_the_backend_sees_the_calls_of_today():
    """a scripted backend WITHOUT the two new methods: penalty=None, uncertainty=False ask for nothing new, and the result carries the
    new attributes"""
    class Scripted:
        def __init__(self):
            self.seen = []

        def fit_field_chi2(self, mus, basis, nnode, nodes, obs, weight=None, base=None):
            self.seen.append('chi2')
            x = np.asarray(nodes)[:, 0]
            return np.array([4.0 * 0.5 ** x[0], 2.0 + np.abs(x[1])]), np.zeros((2, 3, 2))

        def fit_field_normal(self, mus, basis, nnode, nodes, obs, weight=None, base=None, amplitudes=None):
            self.seen.append('normal')
            return fit.FieldNormal(None, np.ones((2, 1)), np.ones((2, 1, 1)), None)

        def fit_field_step(self, hess, grad, lam, nodes, lo=None, hi=None):
            self.seen.append('step')
            return np.asarray(nodes) + 1.0, np.ones(2), np.zeros(2, dtype=np.int32)

    be = Scripted()
    obs = np.zeros((2, 4, 5, 1))
    w = np.ones(obs.shape)
    w[1, :, 0] = 0.0
    r = drivers.fit_field_columns(be, obs, [1.0], np.ones((1, 2)), np.zeros((2, 1)), (1, 0, 0), weight=w, lambda0=1.0, lambda_max=1e3, max_iter=3)
    assert be.seen == ['chi2'] + ['normal', 'step', 'chi2'] * 3
    assert r.uncertainty is None and np.all(r.penalty == 0.0) and r.chi2_data is r.chi2 and list(r.dof) == [19, 15]
    assert drivers.fit_field_columns(be, None, [1.0], np.ones((1, 2)), np.zeros((2, 1)), (1, 0, 0), max_iter=1).dof is None
    # the degrees of freedom are counted when asked for: a weight the loop cannot read is the backend's to judge, as it ever was
    odd = drivers.fit_field_columns(be, obs, [1.0], np.ones((1, 2)), np.zeros((2, 1)), (1, 0, 0), weight=np.ones((7, 3)), max_iter=1)
    assert odd.dof is None
    with pytest.raises(ValueError):
        drivers.fit_field_columns(be, obs, [1.0], np.ones((1, 2)), np.zeros((2, 1)), (1, 0, 0), max_iter=1, scale=2.0)       # no uncertainty
    for kw in (dict(penalty=fit.Penalty([[1.0]])), dict(uncertainty=True)):                # the new methods are asked for only then
        with pytest.raises(AttributeError):
            drivers.fit_field_columns(be, obs, [1.0], np.ones((1, 2)), np.zeros((2, 1)), (1, 0, 0), max_iter=1, **kw)


def test_scale_reduced_and_columns_without_an_estimate():
    """a scripted backend with the new methods: scale='reduced' hands over chi2_data / (N - P); a column with N <= P has no estimate"""
    class Scripted:
        def fit_field_chi2(self, mus, basis, nnode, nodes, obs, weight=None, base=None):
            return np.array([30.0, 7.0]), np.zeros((2, 3, 2))

        def fit_field_normal(self, mus, basis, nnode, nodes, obs, weight=None, base=None, amplitudes=None):
            return fit.FieldNormal(np.array([30.0, 7.0]), np.ones((2, 1)), np.ones((2, 1, 1)), None)

        def fit_field_step(self, hess, grad, lam, nodes, lo=None, hi=None):
            return np.asarray(nodes), np.zeros(2), np.zeros(2, dtype=np.int32)

        def fit_field_uncertainty(self, hess, basis, nnode, penalty=None, scale=None):
            self.scale = np.array(scale)
            one = np.ones((2, 1, 1))
            return fit.FieldUncertainty(one.copy(), one * self.scale[:, None, None], np.sqrt(self.scale)[:, None], np.ones((2, 3, 2)),
                                        np.zeros(2, dtype=np.int32), nnode)

    be = Scripted()
    w = np.zeros((2, 4, 4, 1))
    w[0] = 1.0
    w[1, 0, 0] = 2.0                                                                       # column 1: one point of positive weight, N = P
    r = drivers.fit_field_columns(be, np.zeros(w.shape), [1.0], np.ones((1, 2)), np.zeros((2, 1)), (1, 0, 0), weight=w, max_iter=1,
                                  uncertainty=True, scale='reduced')
    assert list(r.dof) == [15, 0] and be.scale[0] == 30.0 / 15 and np.isfinite(be.scale[1])
    u = r.uncertainty
    assert list(u.status) == [0, 1] and u.sigma[0, 0] == np.sqrt(2.0) and all(np.all(np.isnan(a[1])) for a in (u.ainv, u.cov, u.sigma, u.field_sigma))
    with pytest.raises(ValueError):
        drivers.fit_field_columns(be, np.zeros(w.shape), [1.0], np.ones((1, 2)), np.zeros((2, 1)), (1, 0, 0), max_iter=1, uncertainty=True,
                                  scale='chi2')


@pytest.mark.parametrize('Ns,nn,ncol', rg.REGULAR_RECOVERY)
def test_a_smoothness_penalty_leaves_the_noise_free_recovery_alone(host, fithost, reghost, Ns, nn, ncol):
    mus = np.array([1.0])
    (prob, block, prof, J), pats, fld, nnode, basis, truth, start = fc.recovery(Ns, ncol, nn)
    be = rg.HostBackend(reghost, host, fithost, prob, block, prof, block.n, J, pats, *fc.RECOVERY_WINDOW)
    _, obs = be.response(np.stack(fld, axis=1), mus, nnode, fc.AMPS)
    r = drivers.fit_field_columns(be, obs, mus, basis, start, nnode, weight=fc.recovery_weight(obs), amplitudes=fc.AMPS,
                                  penalty=rg.recovery_penalty(nn), **fc.RECOVERY_LOOP)
    print('Ns %d, %d nodes, %d columns, regularised: chi2 %s -> %s in %s iterations, node error %.3g, penalty %s'
          % (Ns, nn, ncol, r.history[0], r.chi2, r.iterations, np.max(np.abs(r.nodes - truth)), r.penalty))
    fc.check_recovery(r, truth)
    assert np.all(r.penalty <= 1e-8 * r.history[0]) and np.all(r.iterations <= rg.RECOVERY_ITERATIONS)
    assert be.calls['penalty'] == be.calls['normal'] + be.calls['chi2'] and be.calls['uncertainty'] == 0 and r.uncertainty is None


def test_the_pieces_compose(reghost):
    """the penalty with an instrument and with four quantities, on the host backends of those tests"""
    import fit_instrument_cases as fic
    import velocity_cases as vc
    mus = np.array([1.0])
    (prob, block, prof, J), pats, fld, nnode, basis, truth, start = fc.recovery(13, 1, 3)
    be = rg.regular(fic.InstHostBackend(rc.HostLib(), fic.FitInstHostLib(), prob, block, prof, block.n, J, pats, *fc.RECOVERY_WINDOW), reghost)
    inst = fic.recovery_instrument(fic.window_grid(prob, *fc.RECOVERY_WINDOW), 'a')
    obs = vc.smear(inst, be.response(np.stack(fld, axis=1), mus, nnode, fc.AMPS)[1])
    r = drivers.fit_field_columns(be, obs, mus, basis, start, nnode, weight=fc.recovery_weight(obs), amplitudes=fc.AMPS, instrument=inst,
                                  penalty=rg.recovery_penalty(3), uncertainty=True, **fc.RECOVERY_LOOP)
    print('through the instrument: %s iterations, node error %.3g, penalty %s, sigma %s' % (r.iterations, np.max(np.abs(r.nodes - truth)),
                                                                                             r.penalty, r.uncertainty.sigma))
    fc.check_recovery(r, truth)
    assert np.all(r.penalty <= 1e-8 * r.history[0]) and np.all(r.iterations == rg.COMPOSE_ITERATIONS['instrument'])
    assert not r.uncertainty.status.any() and np.all(r.uncertainty.sigma > 0)

    Ns, nn, mu4, ncol, _ = vc.RECOVERY_CASES[0]
    (prob, block, prof, J), pats, fld4, nnode, basis, truth, start, vB = vc.recovery(Ns, ncol, nn)
    be = rg.regular(vc.HostBackend(vc.HostLib(), vc.FitHostLib(), prob, block, prof, block.n, J, pats, *vc.RECOVERY_WINDOW), reghost)
    _, obs = be.response(np.stack(fld4, axis=1), np.array(mu4), nnode, vc.amps(prof[1]))
    r = drivers.fit_field_columns(be, obs, np.array(mu4), basis, start, nnode, weight=fc.recovery_weight(obs), amplitudes=vc.amps(prof[1]),
                                  penalty=rg.velocity_prior(nnode, truth, vB), uncertainty=True, max_iter=vc.max_iter(0), **vc.RECOVERY_LOOP)
    print('four quantities: %s iterations, penalty %s, sigma(vlos) / vBroad %s' % (r.iterations, r.penalty, r.uncertainty.parameter('vlos') / vB))
    vc.check_recovery(r, truth, nnode, vB, vc.max_iter(0))
    assert np.all(r.penalty <= 1e-8 * r.history[0]) and np.all(r.iterations == rg.COMPOSE_ITERATIONS['velocity'])
    assert r.uncertainty.field_sigma.shape == (1, 4, Ns) and not r.uncertainty.status.any()


def test_the_noisy_case(host, fithost, reghost):
    """Six B nodes, two each for gammaB and chiB, three columns, noise of 1e-3 max I (seed 11), weights 1 / sigma^2, bounds, tol 1e-9.
    Measured on the CPU (the issue): the plain fit converges in 9, 5, 9 iterations with chi2 142.8, 167.3, 156.8 for 166 degrees of
    freedom, B nodes off by up to 0.059, 0.023, 0.256 T, largest pull 1.40; with 1e6 T^-2 on the second differences of B 5 iterations
    each, B nodes off by 0.0015, 0.0027, 0.0025 T, largest pull against the sandwich 1.73.  What this run gives is printed."""
    (prob, block, prof, J), pats, fld, nnode, basis, truth, start = rg.noisy_setup()
    mus = np.array([1.0])
    be = rg.HostBackend(reghost, host, fithost, prob, block, prof, block.n, J, pats, *fc.RECOVERY_WINDOW)
    _, clean = be.response(np.stack(fld, axis=1), mus, nnode, fc.AMPS)
    obs, w = rg.add_noise(clean)
    n0 = dict(be.calls)
    plain, reg = rg.noisy_fits(be, obs, w, mus, basis, start, nnode)
    rg.check_noisy(plain, reg, truth, nnode, 'host')
    assert be.calls['uncertainty'] == 2 and reg.uncertainty.field_sigma.shape == (3, 3, 13)
    # plain: a chi2 call more than normal calls and one normal call for the uncertainties; regularised: a penalty call behind each but that one
    n_plain = len(plain.history) - 1
    n_reg = len(reg.history) - 1
    assert be.calls['normal'] - n0['normal'] == n_plain + n_reg + 2 and be.calls['penalty'] == 2 * n_reg + 1
    # the band of the expanded field is sigma at the nodes' depths (hat functions: node values ARE field values there)
    assert np.allclose(reg.uncertainty.field_sigma[:, 0, 0], reg.uncertainty.sigma[:, 0], rtol=1e-12)


# ---- 5., 6. --------------------------------------------------------------------------------------------------------------------------------
def test_the_sanitizer_program():
    """make fitregularsan: both entries' host mirrors on P = Q = 1, on P = 24, Q = 96, Nspace = 82 and with a singular column among good
    ones under ASan and UBSan, stand-alone"""
    subprocess.check_call(['make', '-s', '-C', sc.CSRC, 'fitregularsan'])
    out = subprocess.run([os.path.join(sc.CSRC, 'lsx_fit_regular_san')], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and 'lsx_fit_regular_san: ok' in out.stdout and 'runtime error' not in out.stderr, out.stdout + out.stderr


def test_names_and_resources():
    """the header declares exactly the two entries; the library exports exactly those under lsx_hip_regular; neither is required of a
    library; the compiler's report of the unit: three kernels, no scratch, no spilled vector register, no dynamic stack"""
    hdr = open(os.path.join(ROOT, 'include', 'lsx_hip_fit_regular.h')).read()
    declared = sorted(set(re.findall(r'\b(lsx_hip_\w+)\s*\(', re.sub(r'/\*.*?\*/', '', hdr, flags=re.S))))
    want = ['lsx_hip_regular_penalty', 'lsx_hip_regular_uncertainty']
    assert declared == want
    top = open(os.path.join(ROOT, 'include', 'lsx_hip.h')).read()
    assert top.index('#include "lsx_hip_fit.h"') < top.index('#include "lsx_hip_fit_regular.h"')
    assert 'regular' not in open(os.path.join(ROOT, 'include', 'lsx_hip_fit.h')).read()
    from lightspinner_amd import _capi
    assert not [n for n in _capi.REQUIRED_SYMBOLS if 'regular' in n]
    so = os.path.join(sc.CSRC, 'liblsx_hip.so')
    log = os.path.join(sc.CSRC, 'build', 'lsx_fit_regular.ru.log')
    if not (os.path.exists(so) and os.path.exists(log)):
        subprocess.check_call(['make', '-s', '-j', '8', '-C', sc.CSRC])
    syms = subprocess.run(['nm', '-D', '--defined-only', so], capture_output=True, text=True, check=True).stdout
    assert sorted(n for n in re.findall(r' T (\w+)', syms) if n.startswith('lsx_hip_regular')) == want
    blocks = re.split(r'remark: Function Name: ', open(log).read())[1:]
    names = [b.split()[0] for b in blocks]
    assert len(names) == 3 and all(any(k in n for n in names) for k in ('k_regular_penalty', 'k_regular_covariance', 'k_regular_band')), names
    for b in blocks:
        get = lambda key: re.search(re.escape(key) + r': (\S+)', b).group(1)
        assert (get('ScratchSize [bytes/lane]'), get('VGPRs Spill'), get('Dynamic Stack')) == ('0', '0', 'False'), b.split()[0]
