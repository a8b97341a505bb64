"""The field fit on the GPU (include/lsx_hip_fit.h: lsx_hip_fit_field_normal, _chi2, _step): chi2, grad and hess against numpy in
longdouble from the rf and stokes that Engine.stokes_response returns for the expanded field, inside (M + 2 Nspace + 8) u x the
absolute sum per entry (tests/fit_cases.py); the step by its backward error, P (3 P + 1) u; the bits under every cut of the call;
the refusals; drivers.fit_field_columns on the engine recovering a known field; FALC Ca II 854.2 nm."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import fit_cases as fc
import stokes_cases as sc
import stokes_response_cases as rc
from conftest import golden
from lightspinner_amd import _capi, drivers, fit, synth
from lightspinner_amd.problem import Engine
from test_fit_host import CASES

pytestmark = pytest.mark.gpu
same = fc.same


@pytest.fixture(scope='module')
def fithost():
    return fc.FitHostLib()


def make_engine(hip_lib, prob, block, prof, J):
    e = Engine(prob, block.ncol, lib=hip_lib)
    synth.load_columns(e, block, prof)
    e.set(_capi.LSX_J, J)
    return e


def stack(r):
    return np.stack([r.I, r.Q, r.U, r.V], axis=1)          # [ncol][4][nla][nmu]


def spectrum(e, mus, field, pats, **kw):
    return stack(e.stokes_rays(mus, field[:, 0], field[:, 1], field[:, 2], patterns=pats, **kw))


def response(e, mus, field, nnode, pats, amplitudes=fc.AMPS, **kw):
    """-> rf [ncol][npar][4][nla][Ns][nmu], S [ncol][4][nla][nmu] of Engine.stokes_response for the fitted parameters"""
    names = [p for p, n in zip(rc.PARAMS, nnode) if n > 0]
    r = e.stokes_response(mus, field[:, 0], field[:, 1], field[:, 2], patterns=pats, parameters=names, amplitudes=amplitudes, **kw)
    return rc.stack_rf(r, names), stack(r.stokes)


@pytest.mark.parametrize('Ns,ncol,win,ms,nnode,wkind,given,pats', CASES)
def test_normal_equations(hip_lib, fithost, Ns, ncol, win, ms, nnode, wkind, given, pats):
    """the cases of tests/test_fit_host.py: M = 4 to 1560, P = 1 to 24"""
    prob, block, prof, J = sc.problem(Ns, ncol, vlos=True)
    fld = sc.field(Ns, ncol)
    la0, nla = win
    mus, pats = fc.MUS[ms], sc.PATTERN_SETS[pats]
    e = make_engine(hip_lib, prob, block, prof, J)
    basis, base = fc.basis_of(Ns, nnode), fc.base_of(fld, nnode, given)
    truth = fc.nodes_of(fld, Ns, nnode, base)
    obs = spectrum(e, mus, fithost.expand(Ns, nnode, basis, base, truth), pats, la0=la0, nla=nla)
    nodes = fc.off_truth(truth, nnode)
    w = fc.weights_of(wkind, obs.shape)
    kw = dict(weight=w, base=base if given or 0 in nnode else None, patterns=pats, la0=la0, nla=nla)
    if kw['base'] is None:
        assert not np.any(base)
    ne = e.fit_field_normal(mus, basis, nnode, nodes, obs, amplitudes=fc.AMPS, **kw)
    assert same(ne.field, fithost.expand(Ns, nnode, basis, base, nodes))
    rf, S = response(e, mus, ne.field, nnode, pats, la0=la0, nla=nla)
    val, bar = fc.yardstick(nnode, rf, S, obs, w, basis)
    x = fc.inside(dict(chi2=ne.chi2, grad=ne.grad, hess=ne.hess), val, bar)
    sig = fc.grad_signal(val, bar)
    print('Ns %d, M %d, P %d: deviation / bar %s, largest |grad| / bar %.3g' % (Ns, 4 * nla * len(mus), sum(nnode), x, sig))
    assert max(x.values()) <= 1.0 and sig >= fc.SIGNAL
    assert same(ne.hess, np.swapaxes(ne.hess, 1, 2))
    c2, f2 = e.fit_field_chi2(mus, basis, nnode, nodes, obs, **kw)
    assert same(c2, ne.chi2) and same(f2, ne.field)
    if w is not None:                     # a masked point's obs does not enter
        n2 = e.fit_field_normal(mus, basis, nnode, nodes, np.where(w > 0, obs, obs * 3.0 + 1.0), amplitudes=fc.AMPS, **kw)
        assert all(same(getattr(n2, k), getattr(ne, k)) for k in ('chi2', 'grad', 'hess'))
    e.close()


def test_bits(hip_lib, fithost):
    """a column's chi2, grad and hess do not depend on the column range, on one column per pass under a small work cap (the
    response's, the Stokes pass's and the fit's own), or on the other columns' nodes and obs"""
    Ns, ncol, nnode, la0, nla = 13, 3, (3, 3, 3), 7, 65
    prob, block, prof, J = sc.problem(Ns, ncol, vlos=True)
    fld = sc.field(Ns, ncol)
    pats = sc.PATTERN_SETS['blend']
    e = make_engine(hip_lib, prob, block, prof, J)
    basis = fc.basis_of(Ns, nnode)
    truth = fc.nodes_of(fld, Ns, nnode)
    mus = fc.MUS
    obs = spectrum(e, mus, fithost.expand(Ns, nnode, basis, None, truth), pats, la0=la0, nla=nla)
    nodes = fc.off_truth(truth, nnode)
    w = fc.weights_of('given', obs.shape)
    keys = ('chi2', 'grad', 'hess')

    def call(x=nodes, o=obs, wt=w, **kw):
        return e.fit_field_normal(mus, basis, nnode, x, o, weight=wt, patterns=pats, la0=la0, nla=nla, amplitudes=fc.AMPS, **kw)

    whole = call()
    for c in range(3):
        one = call(nodes[c:c + 1], obs[c:c + 1], w[c:c + 1], col0=c, ncol=1)
        assert all(same(getattr(one, k)[0], getattr(whole, k)[c]) for k in keys), c
    two = call(nodes[1:], obs[1:], w[1:], col0=1, ncol=2)
    assert all(same(getattr(two, k), getattr(whole, k)[1:]) for k in keys)
    assert all(same(getattr(call(work_cap_bytes=1), k), getattr(whole, k)) for k in keys)          # the fit's groups: one column each
    call(work_cap_bytes=0)
    e.lib.check(e.lib.dll.lsx_hip_response_stokes_work_cap(e._h, 1))                                # one column a pass of the response
    e.lib.check(e.lib.dll.lsx_hip_stokes_rays_work_cap(e._h, 1))
    assert all(same(getattr(call(), k), getattr(whole, k)) for k in keys)
    c2 = e.fit_field_chi2(mus, basis, nnode, nodes, obs, weight=w, patterns=pats, la0=la0, nla=nla)[0]
    assert same(c2, whole.chi2)
    e.lib.check(e.lib.dll.lsx_hip_response_stokes_work_cap(e._h, 0))
    e.lib.check(e.lib.dll.lsx_hip_stokes_rays_work_cap(e._h, 0))
    x2, o2 = nodes.copy(), obs.copy()
    x2[[0, 2]] = truth[[0, 2]] * 1.1
    o2[[0, 2]] *= 1.3
    other = call(x2, o2)
    assert all(same(getattr(other, k)[1], getattr(whole, k)[1]) for k in keys)
    assert not same(other.chi2[0], whole.chi2[0])
    e.close()


@pytest.mark.parametrize('nnode', fc.NNODES)
def test_step(hip_lib, fithost, nnode):
    """systems of the fit itself, P = 1, 2, 6, 9, 24, 70 columns with different dampings (more than one block at every P): delta is
    the trial from nodes = 0 without bounds; unclamped and with every bound active; singular and NaN systems among good ones"""
    Ns, la0, nla = 13, *fc.RECOVERY_WINDOW
    prob, block, prof, J = sc.problem(Ns, 1, vlos=True)
    fld = sc.field(Ns, 1)
    pats = sc.PATTERN_SETS['blend']
    e = make_engine(hip_lib, prob, block, prof, J)
    basis, base = fc.basis_of(Ns, nnode), fc.base_of(fld, nnode, False)
    truth = fc.nodes_of(fld, Ns, nnode, base)
    obs = spectrum(e, fc.MUS[:1], fithost.expand(Ns, nnode, basis, base, truth), pats, la0=la0, nla=nla)
    nodes = fc.off_truth(truth, nnode)
    ne = e.fit_field_normal(fc.MUS[:1], basis, nnode, nodes, obs, weight=fc.recovery_weight(obs), base=base, patterns=pats, la0=la0,
                            nla=nla, amplitudes=fc.AMPS)
    P, nc = sum(nnode), 70
    lam = 10.0 ** np.linspace(-3.0 if P == 24 else -6.0, 1.0, nc)
    H, g, x = np.repeat(ne.hess, nc, axis=0), np.repeat(ne.grad, nc, axis=0), np.repeat(nodes, nc, axis=0)
    delta, _, st0 = e.fit_field_step(H, g, lam, np.zeros((nc, P)))
    trial, pred, st = e.fit_field_step(H, g, lam, x)
    lo, hi = nodes[0] - 0.25 * np.min(np.abs(delta), axis=0), nodes[0] + 0.5 * np.min(np.abs(delta), axis=0)      # active in every column
    t2, p2, s2 = e.fit_field_step(H, g, lam, x, lo, hi)
    assert not st0.any() and not st.any() and not s2.any() and np.all(pred > 0)
    worst = [0.0, 0.0]
    for c in range(nc):
        be_, ok, pr = fc.step_checks(P, H[c], g[c], lam[c], x[c], -np.inf, np.inf, trial[c], pred[c], delta[c])
        _, ok2, pr2 = fc.step_checks(P, H[c], g[c], lam[c], x[c], lo, hi, t2[c], p2[c], delta[c])
        worst = [max(worst[0], be_), max(worst[1], pr, pr2)]
        assert be_ <= 1.0 and ok and ok2 and pr <= 1.0 and pr2 <= 1.0, (c, be_, ok, ok2, pr, pr2)
    assert np.all((t2 >= lo) & (t2 <= hi)) and not np.array_equal(t2, trial)
    print('P %d: backward error / bar %.3g, predicted / bar %.3g' % (P, *worst))
    Hb = H.copy()
    Hb[3, -1, :] = Hb[3, :, -1] = 0.0
    Hb[40, 0, 0] = np.nan
    Hb[69, 0, 0] = -Hb[69, 0, 0]
    t3, p3, s3 = e.fit_field_step(Hb, g, lam, x)
    bad = [3, 40, 69]
    good = [c for c in range(nc) if c not in bad]
    assert list(np.nonzero(s3)[0]) == bad and np.all(p3[bad] == 0.0) and same(t3[bad], x[bad])
    assert same(t3[good], trial[good]) and same(p3[good], pred[good])
    e.close()


def test_refusals(hip_lib, fithost):
    Ns, ncol, nnode = 5, 3, (2, 2, 2)
    prob, block, prof, J = sc.problem(Ns, ncol, vlos=True)
    fld = sc.field(Ns, ncol)
    patterns = sc.PATTERN_SETS['all']
    e = make_engine(hip_lib, prob, block, prof, J)
    e.formal_sol_gamma()
    before = [e.get(w).copy() for w in (_capi.LSX_I, _capi.LSX_J, _capi.LSX_N)]
    S0 = stack(e.stokes_rays(fc.MUS, *fld, patterns=patterns))
    basis = fc.basis_of(Ns, nnode)
    nodes = fc.nodes_of(fld, Ns, nnode)
    obs = S0 * 1.01
    EINVAL, EUNS = sc.LSX_EINVAL, sc.LSX_EUNSUPPORTED

    def refused(code, mus=fc.MUS, b=basis, nn=nnode, x=nodes, o=obs, word=None, chi2_too=True, **kw):
        kw.setdefault('patterns', patterns)
        calls = [lambda: e.fit_field_normal(mus, b, nn, x, o, **kw)]
        if chi2_too:
            kw2 = {k: v for k, v in kw.items() if k != 'amplitudes'}
            calls.append(lambda: e.fit_field_chi2(mus, b, nn, x, o, **kw2))
        for f in calls:
            with pytest.raises(_capi.LsxError) as ei:
                f()
            assert ei.value.code == code, (ei.value.code, str(ei.value))
            assert word is None or word in str(ei.value), str(ei.value)

    e.fit_field_normal(fc.MUS, basis, nnode, nodes, obs, patterns=patterns)
    # what the response refuses, of the expanded field
    for p in range(3):
        for bad in (np.nan, np.inf):
            bs = np.zeros((ncol, 3, Ns))
            bs[1, p, 2] = bad
            refused(EINVAL, base=bs, word='base')
    x = nodes.copy()
    x[2, 0] = -1.0                                        # B < 0 at depth 0 of column 2
    refused(EINVAL, x=x)
    x[2, 0] = 2e-4                                        # 0 <= B < a_B / 2 there: the response's rule, known after the expansion
    refused(EINVAL, x=x, word='column 2, depth 0', chi2_too=False, amplitudes={'B': 1e-3})
    e.fit_field_chi2(fc.MUS, basis, nnode, x, obs, patterns=patterns)                       # (the Stokes pass takes that field)
    e.fit_field_normal(fc.MUS, basis[2:], (0, 2, 2), x[:, 2:], obs, base=fc.base_of(fld, (0, 2, 2), False), patterns=patterns,
                       amplitudes={'B': np.nan})                                            # not fitted: its amplitude is not read
    for p in rc.PARAMS:
        for bad in (0.0, -1e-3, np.nan, np.inf):
            refused(EINVAL, amplitudes={p: bad}, word=p, chi2_too=False)
    refused(EINVAL, patterns=[([-1, 0, 2], [1, 1, 1], [0, 0, 0]), None, None])
    refused(EINVAL, la0=-1, nla=3, o=obs[:, :, :3])
    refused(EINVAL, la0=prob.Nspect - 2, nla=3, o=obs[:, :, :3])
    refused(EINVAL, col0=2, ncol=2, x=nodes[:2], o=obs[:2])
    for bad in ([0.0], [1.0 + 1e-12], [np.nan], [-0.5]):
        refused(EINVAL, mus=np.array(bad), o=obs[..., :1])
    over = (np.r_[sc.LARGEST.alpha, np.zeros(38, dtype=np.int32)], np.r_[sc.LARGEST.strength, np.zeros(38)], np.r_[sc.LARGEST.shift, np.zeros(38)])
    refused(EUNS, patterns=[over, None, None])
    # its own
    for nn, b in (((0, 0, 0), basis[:0]), ((9, 8, 8), np.ones((25, Ns))), ((3, -1, 0), basis[:2])):
        with pytest.raises(_capi.LsxError) as ei:
            e.fit_field_normal(fc.MUS, b, nn, np.zeros((ncol, 1)), obs, patterns=patterns)
        assert ei.value.code == EINVAL
    for bad in (np.nan, np.inf, -np.inf):
        for name in ('b', 'x', 'o'):
            a = {'b': basis, 'x': nodes, 'o': obs}[name].copy()
            a.reshape(-1)[-2] = bad
            refused(EINVAL, **{name: a})
        wt = np.ones_like(obs)
        wt[1, 2, 3, 0] = bad
        refused(EINVAL, weight=wt, word='weight')
    wt = np.ones_like(obs)
    wt[0, 0, 0, 0] = -1e-300
    refused(EINVAL, weight=wt, word='negative')
    # null outputs, raw
    dll, h = e.lib.dll, e._h
    from lightspinner_amd import zeeman
    nc, al, st, sh = zeeman.pack(patterns, prob.Nlines)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    mu, amp, nn = np.ascontiguousarray(fc.MUS), np.full(3, 1e-3), np.array(nnode, dtype=np.int32)
    ob = np.ascontiguousarray(obs)
    out = [np.empty(ncol), np.empty((ncol, 6)), np.empty((ncol, 6, 6))]

    def raw(chi2=out[0], grad=out[1], hess=out[2], amps=amp):
        return dll.lsx_hip_fit_field_normal(h, 3, dp(mu), 0, ncol, 0, prob.Nspect, ip(nc), ip(al), dp(st), dp(sh), ip(nn), dp(basis), None,
                                            dp(nodes), dp(amps), dp(ob), None, dp(chi2), dp(grad), dp(hess), None)

    assert raw() == sc.LSX_OK
    assert raw(chi2=None) == EINVAL and raw(grad=None) == EINVAL and raw(hess=None) == EINVAL and raw(amps=None) == EINVAL
    assert dll.lsx_hip_fit_field_chi2(h, 3, dp(mu), 0, ncol, 0, prob.Nspect, ip(nc), ip(al), dp(st), dp(sh), ip(nn), dp(basis), None,
                                      dp(nodes), dp(ob), None, None, None) == EINVAL
    # the step's
    H, g = np.eye(6)[None], np.ones((1, 6))
    for kw in (dict(lam=-1.0), dict(lam=np.nan), dict(lam=np.inf), dict(lo=np.ones(6), hi=np.zeros(6)), dict(lo=np.full(6, np.nan))):
        with pytest.raises(_capi.LsxError) as ei:
            e.fit_field_step(H, g, kw.pop('lam', 1.0), np.zeros((1, 6)), **kw)
        assert ei.value.code == EINVAL
    for w_, b_ in zip((_capi.LSX_I, _capi.LSX_J, _capi.LSX_N), before):
        assert np.array_equal(e.get(w_), b_)
    assert same(stack(e.stokes_rays(fc.MUS, *fld, patterns=patterns)), S0)
    e.close()


@pytest.mark.parametrize('Ns,nn,mus', fc.RECOVERY_CASES + [(13, 2, 'three columns')])
def test_the_loop_recovers_a_known_field(hip_lib, fithost, Ns, nn, mus):
    ncol = 3 if mus == 'three columns' else 1
    mus = np.array([1.0] if ncol == 3 else mus)
    (prob, block, prof, J), pats, fld, nnode, basis, truth, start = fc.recovery(Ns, ncol, nn)
    e = make_engine(hip_lib, prob, block, prof, J)
    la0, nla = fc.RECOVERY_WINDOW
    obs = spectrum(e, mus, np.stack(fld, axis=1), pats, la0=la0, nla=nla)
    w = fc.recovery_weight(obs)
    r = drivers.fit_field_columns(e, obs, mus, basis, start, nnode, weight=w, amplitudes=fc.AMPS, patterns=pats, la0=la0, nla=nla,
                                  **fc.RECOVERY_LOOP)
    print('Ns %d, %d nodes, %d angles, %d columns: chi2 %s -> %s in %s iterations, node error %.3g, lambda %s'
          % (Ns, nn, len(mus), ncol, r.history[0], r.chi2, r.iterations, np.max(np.abs(r.nodes - truth)), r.lam))
    fc.check_recovery(r, truth)
    assert same(r.field, fithost.expand(Ns, nnode, basis, None, r.nodes))
    for c in range(ncol):
        n_c = int(r.iterations[c])
        assert np.all(r.history[n_c:, c] == r.history[n_c, c])
    if ncol == 3:           # a column fitted alone takes the same path, bit for bit
        one = drivers.fit_field_columns(e, obs[1:2], mus, basis, start[1:2], nnode, weight=w[1:2], amplitudes=fc.AMPS, patterns=pats,
                                        la0=la0, nla=nla, col0=1, ncol=1, **fc.RECOVERY_LOOP)
        assert same(one.nodes[0], r.nodes[1]) and same(one.history[:, 0], r.history[:len(one.history), 1])
    e.close()


# ---- FALC Ca II ------------------------------------------------------------------------------------------------------------------------
def test_falc_caii_8542(hip_lib):
    """the converged fixture and the field of the response's test (0.1 T, 45 deg, 30 deg; mu = 1 and 0.6): the normal equations at the
    start against numpy from Engine.stokes_response; one constant node per parameter from 0.11 T, 50 deg, 25 deg.
    The iteration count and the recovered values are printed, not asserted."""
    from test_stokes import FALC_MUS, falc, falc_engine
    prob, block, prof, n, J, (la0, nla), line = falc()
    e, fld = falc_engine(hip_lib)
    pats = [None] * prob.Nlines
    pats[line] = sc.TRIPLET
    Ns, nnode = prob.Nspace, (1, 1, 1)
    basis = np.ones((3, Ns))
    obs = stack(e.stokes_rays(FALC_MUS, *fld, patterns=pats, la0=la0, nla=nla))
    w = fc.recovery_weight(obs)
    start = np.array([[0.11, np.deg2rad(50.0), np.deg2rad(25.0)]])
    kw = dict(weight=w, patterns=pats, la0=la0, nla=nla)
    ne = e.fit_field_normal(FALC_MUS, basis, nnode, start, obs, **kw)
    rf, S = response(e, FALC_MUS, ne.field, nnode, pats, amplitudes=None, la0=la0, nla=nla)
    val, bar = fc.yardstick(nnode, rf, S, obs, w, basis)
    x = fc.inside(dict(chi2=ne.chi2, grad=ne.grad, hess=ne.hess), val, bar)
    print('FALC Ca II 854.2 nm, %d wavelengths, %d depths: deviation / bar %s, |grad| / bar %.3g' % (nla, Ns, x, fc.grad_signal(val, bar)))
    assert max(x.values()) <= 1.0 and fc.grad_signal(val, bar) >= fc.SIGNAL
    assert same(e.fit_field_chi2(FALC_MUS, basis, nnode, start, obs, **kw)[0], ne.chi2)
    r = drivers.fit_field_columns(e, obs, FALC_MUS, basis, start, nnode, **kw)
    print('FALC fit: chi2 %.6e -> %.6e, %d iterations, status %d, B %.9f T, gammaB %.7f deg, chiB %.7f deg, lambda %.1e'
          % (r.history[0, 0], r.chi2[0], r.iterations[0], r.status[0], r.nodes[0, 0], *np.rad2deg(r.nodes[0, 1:]), r.lam[0]))
    assert np.all(np.diff(r.history[:, 0]) <= 0) and r.chi2[0] <= 1e-6 * r.history[0, 0]
    e.close()


# ---- through Context -----------------------------------------------------------------------------------------------------------------
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
    hats = fit.hat_basis(np.arange(Ns), [0.0, Ns - 1.0])
    start = np.array([0.105, 0.105, 0.75, 0.45])
    r = ctx.fit_field(mus, obs, transition=trans[kr], basis={'B': hats, 'gammaB': np.ones(Ns), 'chiB': np.ones(Ns)}, start=start, weight=w,
                      max_iter=4)
    pats = [zeeman.zeeman_components(t.transModel) for t in trans if t.isLine]
    la0, nla = int(trans[kr].Nblue), int(trans[kr].wavelength.shape[0])
    basis, nnode = fit.stack_basis(B=hats, gammaB=np.ones(Ns), chiB=np.ones(Ns))
    ref = drivers.fit_field_columns(ctx._engine, obs[None], np.array(mus), basis, start[None], nnode, weight=np.full((1,) + obs.shape, w),
                                    patterns=pats, la0=la0, nla=nla, max_iter=4)
    assert r.nnode == (2, 1, 1) and r.nodes.shape == (4,) and r.field.shape == (3, Ns) and r.history.ndim == 1
    assert same(r.nodes, ref.nodes[0]) and same(r.history, ref.history[:, 0]) and same(r.field, ref.field[0])
    assert r.iterations == ref.iterations[0] and r.status == ref.status[0] and r.history[-1] < r.history[0]
    one = ctx.fit_field(0.6, obs[..., 1], transition=kr, basis=basis, nnode=nnode, start=start, max_iter=1)
    assert one.nodes.shape == (4,) and one.history.shape == (2,)
    assert np.array_equal(ctx.I, I0) and np.array_equal(ctx.J, J0) and all(np.array_equal(a.n, b) for a, b in zip(ctx.activeAtoms, n0))
    ctx.close()
