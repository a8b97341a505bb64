"""The regularised fit and the nodes' uncertainties on the GPU (include/lsx_hip_fit_regular.h: lsx_hip_regular_penalty, _uncertainty): the
two entries against numpy longdouble inside the host tests' bars with the same bit-for-bit statements (tests/regular_cases.py), over
several blocks and under a work cap of one column a group; drivers.fit_field_columns on the engine -- the noise-free recovery under a
smoothness penalty, the issue's noisy case, through an instrument and with four quantities; FALC Ca II 854.2 nm with three B nodes;
Context.fit_field; the refusals."""
import ctypes as C

import numpy as np
import pytest

import fit_cases as fc
import regular_cases as rg
import stokes_cases as sc
from conftest import golden
from lightspinner_amd import _capi, drivers, fit
from test_fit import make_engine, spectrum, stack

pytestmark = pytest.mark.gpu
same = fc.same


@pytest.fixture(scope='module')
def fithost():
    return fc.FitHostLib()


@pytest.fixture(scope='module')
def systems(hip_lib, fithost):
    """nnode -> (the engine's normal equations at the start of the recovery, basis), for P = 1, 6, 24"""
    out = {}
    for nnode in ((1, 0, 0), (2, 2, 2), (8, 8, 8)):
        (prob, block, prof, J), pats, basis, base, nodes, truth = rg.systems_call(nnode)
        e = make_engine(hip_lib, prob, block, prof, J)
        la0, nla = fc.RECOVERY_WINDOW
        obs = spectrum(e, fc.MUS[:1], fithost.expand(13, nnode, basis, base, truth), pats, la0=la0, nla=nla)
        out[nnode] = (e.fit_field_normal(fc.MUS[:1], basis, nnode, nodes, obs, weight=fc.recovery_weight(obs), base=base, patterns=pats,
                                         la0=la0, nla=nla, amplitudes=fc.AMPS), basis)
        e.close()
    return out


@pytest.fixture(scope='module')
def engine(hip_lib):
    """any engine: the columns of the two entries need not be the context's"""
    prob, block, prof, J = sc.problem(5, 1, vlos=True)
    e = make_engine(hip_lib, prob, block, prof, J)
    yield e
    e.close()


# ---- 7. the penalty entry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', [1, 13, 24])
def test_penalty_entry(engine, systems, P):
    """P = 1, 13, 24; Q = 1, 96; 1 and 70 columns (70 blocks); on the fit's own sums or made-up ones of their magnitude, and on zeros;
    then the 70 columns once more in groups of one under the smallest work cap: the same bits"""
    ne = {sum(nn): s[0] for nn, s in systems.items()}.get(P)
    worst = {}
    for Q in (1, 96):
        for ncol, with_target in ((1, False), (70, True)):
            pen, nodes = rg.penalty_case(P, Q, ncol, with_target)
            if ne is not None:
                sums = rg.spread(ne, ncol)
            else:
                r = np.random.default_rng(P)
                K = np.tril(r.normal(size=(ncol, P, P)) * 1e3)
                H = K @ np.swapaxes(K, 1, 2)
                sums = (r.uniform(1e2, 1e4, ncol), r.normal(size=(ncol, P)) * 1e4, np.tril(H) + np.swapaxes(np.tril(H, -1), 1, 2))
            for chi2, grad, hess in ((np.zeros(ncol), np.zeros((ncol, P)), np.zeros((ncol, P, P))), sums):
                x = rg.check_penalty(engine, pen, nodes, chi2, grad, hess)
                worst = {k: max(v, worst.get(k, 0.0)) for k, v in x.items()}
    whole = engine.fit_field_penalty(nodes, pen, *sums)
    engine.lib.check(engine.lib.dll.lsx_hip_fit_field_work_cap(engine._h, 1))
    one_by_one = engine.fit_field_penalty(nodes, pen, *sums)
    engine.lib.check(engine.lib.dll.lsx_hip_fit_field_work_cap(engine._h, 0))
    assert all(same(a, b) for a, b in zip(whole, one_by_one))
    print('penalty entry, P %d: worst deviation / bar %s' % (P, worst))


def test_linear_nodes_cost_nothing(engine, systems):
    rg.check_linear_nodes_cost_nothing(engine, systems[(8, 8, 8)][0])


# ---- 8. the uncertainty entry --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nnode,Ns', [((1, 0, 0), 3), ((2, 2, 2), 82), ((8, 8, 8), 3), ((6, 6, 6, 6), 82), ((3, 3, 0, 0), 3)])
def test_uncertainty_entry(engine, systems, nnode, Ns):
    """P = 1, 6, 24 on 70 columns (70 blocks) with a singular, a NaN and an indefinite system among good ones; Nspace 3 and 82; three
    and four quantities (the 24 x 24 system of (8, 8, 8) read as (6, 6, 6, 6), the 6 x 6 one as (3, 3, 0, 0): the arithmetic does not
    ask what a node means, and smoothness has rows from three nodes on); then in groups of one under the smallest work cap"""
    P = sum(nnode)
    ne = {sum(nn): s[0] for nn, s in systems.items()}[P]
    basis = fc.basis_of(Ns, nnode)
    worst = rg.check_uncertainty(engine, ne.hess[0], basis, nnode, 70)
    print('uncertainty entry, P %d, Nspace %d, %d quantities: worst deviation / bar %s' % (P, Ns, len(nnode), worst))
    H = ne.hess[0][None] * np.linspace(0.5, 2.0, 70)[:, None, None]
    pen = rg.smoothness_or_none(nnode)
    whole = engine.fit_field_uncertainty(H, basis, nnode, penalty=pen, scale=2.0)
    engine.lib.check(engine.lib.dll.lsx_hip_fit_field_work_cap(engine._h, 1))
    one_by_one = engine.fit_field_uncertainty(H, basis, nnode, penalty=pen, scale=2.0)
    engine.lib.check(engine.lib.dll.lsx_hip_fit_field_work_cap(engine._h, 0))
    assert all(same(getattr(whole, k), getattr(one_by_one, k)) for k in ('ainv', 'cov', 'sigma', 'field_sigma')) and not whole.status.any()
    lean = engine.fit_field_uncertainty(H, basis, nnode, penalty=pen, scale=2.0, ainv=False, field_sigma=False)
    assert lean.ainv is None and lean.field_sigma is None and same(lean.cov, whole.cov) and same(lean.sigma, whole.sigma)


# ---- 9. the loop on the engine ---------------------------------------------------------------------------------------------------------------
def test_a_smoothness_penalty_leaves_the_noise_free_recovery_alone(hip_lib, fithost):
    """three columns, three nodes per parameter, within the host loop's count + 2; a column fitted alone takes, bit for bit, the path it
    takes among three"""
    Ns, nn, ncol = rg.REGULAR_RECOVERY[1]
    mus = np.array([1.0])
    (prob, block, prof, J), pats, fld, nnode, basis, truth, start = fc.recovery(Ns, ncol, nn)
    e = make_engine(hip_lib, prob, block, prof, J)
    la0, nla = fc.RECOVERY_WINDOW
    obs = spectrum(e, mus, np.stack(fld, axis=1), pats, la0=la0, nla=nla)
    w = fc.recovery_weight(obs)
    kw = dict(amplitudes=fc.AMPS, patterns=pats, la0=la0, nla=nla, penalty=rg.recovery_penalty(nn), uncertainty=True, **fc.RECOVERY_LOOP)
    r = drivers.fit_field_columns(e, obs, mus, basis, start, nnode, weight=w, **kw)
    print('regularised recovery: chi2 %s -> %s in %s iterations, node error %.3g, penalty %s'
          % (r.history[0], r.chi2, r.iterations, np.max(np.abs(r.nodes - truth)), r.penalty))
    fc.check_recovery(r, truth)
    assert np.all(r.penalty <= 1e-8 * r.history[0]) and np.all(r.iterations <= rg.RECOVERY_ITERATIONS + 2)
    assert same(r.field, fithost.expand(Ns, nnode, basis, None, r.nodes)) and not r.uncertainty.status.any()
    one = drivers.fit_field_columns(e, obs[1:2], mus, basis, start[1:2], nnode, weight=w[1:2], col0=1, ncol=1, **kw)
    assert same(one.nodes[0], r.nodes[1]) and same(one.history[:, 0], r.history[:len(one.history), 1])
    assert same(one.penalty[0], r.penalty[1]) and same(one.chi2_data[0], r.chi2_data[1])
    assert all(same(getattr(one.uncertainty, k)[0], getattr(r.uncertainty, k)[1]) for k in ('ainv', 'cov', 'sigma', 'field_sigma'))
    e.close()


def test_the_noisy_case(hip_lib):
    """tests/test_fit_regular_host.py's, with the same seed and the same conditions, on the engine"""
    (prob, block, prof, J), pats, fld, nnode, basis, truth, start = rg.noisy_setup()
    mus = np.array([1.0])
    e = make_engine(hip_lib, prob, block, prof, J)
    la0, nla = fc.RECOVERY_WINDOW
    obs, w = rg.add_noise(spectrum(e, mus, np.stack(fld, axis=1), pats, la0=la0, nla=nla))
    plain, reg = rg.noisy_fits(e, obs, w, mus, basis, start, nnode, patterns=pats, la0=la0, nla=nla)
    rg.check_noisy(plain, reg, truth, nnode, 'engine')
    e.close()


def test_the_pieces_compose(hip_lib):
    """once through Instrument.gaussian with the smoothness penalty, once with four quantities and a prior on the vlos nodes: within the
    host loop's count + 2 (tests/test_fit_regular_host.py)"""
    import fit_instrument_cases as fic
    import velocity_cases as vc
    mus = np.array([1.0])
    (prob, block, prof, J), pats, fld, nnode, basis, truth, start = fc.recovery(13, 1, 3)
    e = make_engine(hip_lib, prob, block, prof, J)
    la0, nla = fc.RECOVERY_WINDOW
    inst = fic.recovery_instrument(fic.window_grid(prob, la0, nla), 'a')
    obs = e.apply_instrument(spectrum(e, mus, np.stack(fld, axis=1), pats, la0=la0, nla=nla), inst)
    r = drivers.fit_field_columns(e, obs, mus, basis, start, nnode, weight=fc.recovery_weight(obs), amplitudes=fc.AMPS, patterns=pats, la0=la0,
                                  nla=nla, instrument=inst, penalty=rg.recovery_penalty(3), uncertainty=True, **fc.RECOVERY_LOOP)
    print('through the instrument: %s iterations, node error %.3g, penalty %s' % (r.iterations, np.max(np.abs(r.nodes - truth)), r.penalty))
    fc.check_recovery(r, truth)
    assert np.all(r.penalty <= 1e-8 * r.history[0]) and np.all(r.iterations <= rg.COMPOSE_ITERATIONS['instrument'] + 2)
    assert not r.uncertainty.status.any() and np.all(r.uncertainty.sigma > 0)
    e.close()

    Ns, nn, mu4, ncol, _ = vc.RECOVERY_CASES[0]
    (prob, block, prof, J), pats, fld4, nnode, basis, truth, start, vB = vc.recovery(Ns, ncol, nn)
    e = make_engine(hip_lib, prob, block, prof, J)
    obs = stack(e.stokes_rays(np.array(mu4), *fld4[:3], patterns=pats, la0=la0, nla=nla, vlos=fld4[3]))
    cap = rg.COMPOSE_ITERATIONS['velocity'] + 2
    r = drivers.fit_field_columns(e, obs, np.array(mu4), basis, start, nnode, weight=fc.recovery_weight(obs), amplitudes=vc.amps(prof[1]),
                                  patterns=pats, la0=la0, nla=nla, penalty=rg.velocity_prior(nnode, truth, vB), uncertainty=True, max_iter=cap,
                                  **vc.RECOVERY_LOOP)
    print('four quantities: %s iterations, penalty %s, sigma(vlos) / vBroad %s' % (r.iterations, r.penalty, r.uncertainty.parameter('vlos') / vB))
    vc.check_recovery(r, truth, nnode, vB, cap)
    assert np.all(r.penalty <= 1e-8 * r.history[0])
    assert r.uncertainty.field_sigma.shape == (1, 4, Ns) and not r.uncertainty.status.any() and np.all(r.uncertainty.sigma > 0)
    e.close()


# ---- 10. FALC Ca II --------------------------------------------------------------------------------------------------------------------------
def test_falc_caii_8542(hip_lib):
    """The converged fixture, the field and the start of tests/test_fit.py's FALC test (0.1 T, 45 deg, 30 deg; from 0.11 T, 50 deg, 25 deg)
    with THREE hat nodes for B over the depth index, noise of 1e-3 max I (seed 11) and 1e6 T^-2 on the second difference of the B nodes.
    Asserted: converged, chi2 never rises, status 0, every sigma finite and positive.  The recovered values, their sigma and the
    pulls are printed ("How the regularised fit is pinned"), not asserted: the noise level at which three B nodes are all
    constrained on FALC is not known."""
    from test_stokes import FALC_MUS, falc, falc_engine
    prob, block, prof, n, J, (la0, nla), line = falc()
    e, fld = falc_engine(hip_lib)
    pats = [None] * prob.Nlines
    pats[line] = sc.TRIPLET
    Ns = prob.Nspace
    basis, nnode = fit.stack_basis(B=fit.hat_basis(np.arange(Ns), np.linspace(0, Ns - 1, 3)), gammaB=np.ones(Ns), chiB=np.ones(Ns))
    clean = stack(e.stokes_rays(FALC_MUS, *fld, patterns=pats, la0=la0, nla=nla))
    sigma = 1e-3 * clean[:, 0].max()
    obs = clean + np.random.default_rng(11).standard_normal(clean.shape) * sigma
    truth = np.array([0.1, 0.1, 0.1, np.deg2rad(45.0), np.deg2rad(30.0)])
    start = np.array([[0.11, 0.11, 0.11, np.deg2rad(50.0), np.deg2rad(25.0)]])
    r = drivers.fit_field_columns(e, obs, FALC_MUS, basis, start, nnode, weight=np.full(obs.shape, 1.0 / sigma ** 2), patterns=pats, la0=la0,
                                  nla=nla, penalty=fit.Penalty.smoothness(nnode, {'B': rg.ALPHA[0]}, order=2), uncertainty=True, tol=1e-9)
    u = r.uncertainty
    print('FALC regularised fit: chi2 %.6e -> %.6e (data %.6e for %d degrees of freedom, penalty %.3e), %d iterations, status %d'
          % (r.history[0, 0], r.chi2[0], r.chi2_data[0], r.dof[0], r.penalty[0], r.iterations[0], r.status[0]))
    print('FALC nodes %s\nFALC sigma %s\nFALC pulls %s' % (r.nodes[0], u.sigma[0], (r.nodes[0] - truth) / u.sigma[0]))
    print('FALC band of B: %.3e .. %.3e T' % (u.field_sigma[0, 0].min(), u.field_sigma[0, 0].max()))
    assert r.status[0] == fit.CONVERGED and np.all(np.diff(r.history[:, 0]) <= 0)
    assert u.status[0] == 0 and np.all(np.isfinite(u.sigma)) and np.all(u.sigma > 0)
    e.close()


# ---- 11. through Context; the refusals ----------------------------------------------------------------------------------------------------------
def test_fit_field_is_the_driver_on_the_engine(hip_lib):
    from helpers import build_fakes
    from lightspinner_amd import zeeman
    from lightspinner_amd.rh_method import Context
    d = dict(np.load(golden('falc_ca.npz')))
    atmos, spect, eq, bg = build_fakes(d)
    ctx = Context(atmos, spect, eq, bg, lib=hip_lib)
    for _ in range(2):
        ctx.formal_sol_gamma_matrices()
    trans = [t for a in ctx.activeAtoms for t in a.trans]
    kr = [k for k, t in enumerate(trans) if t.isLine and abs(t.lambda0 - 854.44) < 0.1][0]
    trans[kr].transModel.gLandeEff = 1.1
    I0, J0, n0 = ctx.I.copy(), ctx.J.copy(), [np.array(a.n) for a in ctx.activeAtoms]
    Ns = ctx.problem.Nspace
    mus = [1.0, 0.6]
    st = ctx.compute_stokes(mus, np.full(Ns, 0.1), 0.7, 0.5, transition=trans[kr])
    obs = np.stack([st.I, st.Q, st.U, st.V])
    w = 1.0 / (1e-3 * obs[0].max()) ** 2
    hats = fit.hat_basis(np.arange(Ns), np.linspace(0, Ns - 1, 3))
    start = np.array([0.105, 0.1, 0.105, 0.75, 0.45])
    basis, nnode = fit.stack_basis(B=hats, gammaB=np.ones(Ns), chiB=np.ones(Ns))
    pen = fit.Penalty.stack(fit.Penalty.smoothness(nnode, {'B': 1e6}), fit.Penalty.prior(nnode, {'chiB': 1e2}, {'chiB': [0.5]}))
    r = ctx.fit_field(mus, obs, transition=trans[kr], basis={'B': hats, 'gammaB': np.ones(Ns), 'chiB': np.ones(Ns)}, start=start, weight=w,
                      max_iter=3, penalty=pen, uncertainty=True, scale='reduced')
    pats = [zeeman.zeeman_components(t.transModel) for t in trans if t.isLine]
    la0, nla = int(trans[kr].Nblue), int(trans[kr].wavelength.shape[0])
    ref = drivers.fit_field_columns(ctx._engine, obs[None], np.array(mus), basis, start[None], nnode, weight=np.full((1,) + obs.shape, w),
                                    patterns=pats, la0=la0, nla=nla, max_iter=3, penalty=pen, uncertainty=True, scale='reduced')
    assert r.nnode == (3, 1, 1) and r.nodes.shape == (5,) and r.history.ndim == 1 and r.history[-1] < r.history[0]
    assert same(r.nodes, ref.nodes[0]) and same(r.history, ref.history[:, 0]) and same(r.field, ref.field[0])
    assert same(r.penalty, ref.penalty[0]) and same(r.chi2_data, ref.chi2_data[0]) and r.dof == ref.dof[0] == 4 * nla * 2 - 5
    u, v = r.uncertainty, ref.uncertainty
    assert u.cov.shape == (5, 5) and u.sigma.shape == (5,) and u.field_sigma.shape == (3, Ns) and u.status == 0
    assert all(same(getattr(u, k), getattr(v, k)[0]) for k in ('ainv', 'cov', 'sigma', 'field_sigma'))
    assert u.parameter('B').shape == (3,) and np.max(np.abs(np.diag(u.correlation()) - 1.0)) <= 4 * fc.U
    plain = ctx.fit_field(mus, obs, transition=trans[kr], basis=basis, nnode=nnode, start=start, weight=w, max_iter=1)
    assert plain.uncertainty is None and plain.penalty == 0.0 and same(plain.chi2_data, plain.chi2)
    assert np.array_equal(ctx.I, I0) and np.array_equal(ctx.J, J0) and all(np.array_equal(a.n, b) for a, b in zip(ctx.activeAtoms, n0))
    ctx.close()


def test_refusals(hip_lib):
    """every refusal of the two entries, through Engine and raw; the context's I, J, n and a following stokes_rays keep their bits"""
    Ns, ncol = 5, 3
    prob, block, prof, J = sc.problem(Ns, ncol, vlos=True)
    fld = sc.field(Ns, ncol)
    patterns = sc.PATTERN_SETS['all']
    e = make_engine(hip_lib, prob, block, prof, J)
    e.formal_sol_gamma()
    before = [e.get(w).copy() for w in (_capi.LSX_I, _capi.LSX_J, _capi.LSX_N)]
    S0 = stack(e.stokes_rays(fc.MUS, *fld, patterns=patterns))
    EINVAL = sc.LSX_EINVAL
    dll, h = e.lib.dll, e._h
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    P, Q = 3, 2
    L, tg, x = np.ones((Q, P)), np.zeros((2, Q)), np.zeros((2, P))
    chi2, grad, hess, out = np.ones(2), np.ones((2, P)), np.stack([np.eye(P)] * 2), np.empty(2)

    def penalty(ncol=2, P=P, Q=Q, L=L, tg=tg, x=x, chi2=chi2, grad=grad, hess=hess, pen=True):
        st = _capi.LsxFitPenalty(Q, dp(L), dp(tg))
        return dll.lsx_hip_regular_penalty(h, ncol, P, C.byref(st) if pen else None, dp(x), dp(chi2), dp(grad), dp(hess), dp(out))

    assert penalty() == sc.LSX_OK and penalty(grad=None, hess=None) == sc.LSX_OK and penalty(tg=None) == sc.LSX_OK
    bad = lambda a: np.where(np.arange(a.size).reshape(a.shape) == a.size - 1, np.nan, a)
    inf = lambda a: np.where(np.arange(a.size).reshape(a.shape) == 0, np.inf, a)
    for kw in (dict(pen=False), dict(L=None), dict(x=None), dict(chi2=None), dict(grad=None), dict(hess=None), dict(ncol=0), dict(ncol=-1),
               dict(P=0), dict(P=25), dict(Q=0), dict(Q=97), dict(L=bad(L)), dict(L=inf(L)), dict(tg=bad(tg)), dict(tg=inf(tg)),
               dict(x=bad(x)), dict(x=inf(x))):
        assert penalty(**kw) == EINVAL, kw
    chi2[0], grad[1, 0], hess[0, 1, 1] = np.nan, np.inf, np.nan                            # data, not arguments: they flow through
    assert penalty() == sc.LSX_OK and np.isnan(chi2[0]) and np.isinf(grad[1, 0]) and np.isnan(hess[0, 1, 1]) and np.isfinite(chi2[1])

    H = np.stack([np.eye(P) * 2.0] * 2)
    nn, basis, scale = np.array([2, 1, 0], dtype=np.int32), np.ones((P, Ns)), np.ones(2)
    ainv, cov, sg, fs, status = np.empty((2, P, P)), np.empty((2, P, P)), np.empty((2, P)), np.empty((2, 3, Ns)), np.empty(2, dtype=np.int32)

    def uncertainty(ncol=2, P=P, H=H, Q=Q, L=L, pen=True, scale=scale, npar=3, nn=nn, basis=basis, Ns=Ns, ainv=ainv, cov=cov, sg=sg, fs=fs,
                    status=status):
        st = _capi.LsxFitPenalty(Q, dp(L), None)
        return dll.lsx_hip_regular_uncertainty(h, ncol, P, dp(H), C.byref(st) if pen else None, dp(scale), npar, ip(nn), dp(basis), Ns,
                                               dp(ainv), dp(cov), dp(sg), dp(fs), ip(status))

    for kw in ({}, dict(pen=False), dict(scale=None), dict(ainv=None), dict(fs=None), dict(npar=4, nn=np.array([2, 1, 0, 0], dtype=np.int32),
                                                                                          fs=np.empty((2, 4, Ns)))):
        assert uncertainty(**kw) == sc.LSX_OK and not status.any(), kw
    for kw in (dict(H=None), dict(cov=None), dict(sg=None), dict(status=None), dict(nn=None), dict(basis=None), dict(ncol=0), dict(P=0),
               dict(P=25), dict(L=None), dict(Q=0), dict(Q=97), dict(L=bad(L)), dict(scale=np.array([1.0, -1e-300])),
               dict(scale=np.array([np.nan, 1.0])), dict(scale=np.array([1.0, np.inf])), dict(npar=2), dict(npar=5),
               dict(nn=np.array([2, 2, -1], dtype=np.int32)), dict(nn=np.array([2, 2, 0], dtype=np.int32)), dict(Ns=0), dict(basis=bad(basis)),
               dict(basis=inf(basis))):
        assert uncertainty(**kw) == EINVAL, kw
    Hn = H.copy()
    Hn[1, 0, 0] = np.nan                                                                   # data: status 1, the other column untouched
    assert uncertainty(H=Hn) == sc.LSX_OK and list(status) == [0, 1] and np.all(np.isnan(cov[1])) and np.all(np.isfinite(cov[0]))
    # through Engine: a penalty made for another parameterisation, scale of the wrong sign
    with pytest.raises(ValueError):
        e.fit_field_penalty(x, fit.Penalty(np.ones((1, P + 1))), chi2)
    with pytest.raises(_capi.LsxError) as ei:
        e.fit_field_uncertainty(H, basis, nn, scale=-1.0)
    assert ei.value.code == EINVAL and 'scale' in str(ei.value)
    with pytest.raises(_capi.LsxError) as ei:
        e.fit_field_uncertainty(H, basis, (1, 1, 0))
    assert ei.value.code == EINVAL and 'nnode' in str(ei.value)
    for w_, b_ in zip((_capi.LSX_I, _capi.LSX_J, _capi.LSX_N), before):
        assert np.array_equal(e.get(w_), b_)
    assert same(stack(e.stokes_rays(fc.MUS, *fld, patterns=patterns)), S0)
    e.close()
