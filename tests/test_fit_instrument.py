"""The instrument of the field fit on the GPU (include/lsx_hip_fit_instrument.h: lsx_hip_instrument_fit_normal, _fit_chi2, _apply;
k_fit_smear): chi2, grad and hess against numpy in longdouble from the rf and stokes that Engine.stokes_response returns for the
expanded field, both smeared by Instrument.matrix() in longdouble, inside (M' + 2 Nspace + 2 width + 8) u x the absolute sum per entry
and apply_instrument inside (width + 1) u x its absolute sum (tests/fit_instrument_cases.py); the bits under every cut of the call; the
refusals; drivers.fit_field_columns on the engine recovering a known field through a smearing, undersampling instrument; FALC Ca II
854.2 nm."""
import ctypes as C

import numpy as np
import pytest

import fit_cases as fc
import fit_instrument_cases as ic
import stokes_cases as sc
from conftest import golden
from lightspinner_amd import _capi, drivers, fit
from test_fit import make_engine, response, spectrum, stack

pytestmark = pytest.mark.gpu
same = fc.same
KEYS = ('chi2', 'grad', 'hess')


def last_error(e):
    return e.lib.dll.lsx_last_error().decode(errors='replace')


@pytest.fixture(scope='module')
def fithost():
    return ic.FitInstHostLib()


@pytest.mark.parametrize('Ns,ncol,win,ms,nnode,wkind,given,pats,kind', ic.GPU_CASES)
def test_normal_equations(hip_lib, fithost, Ns, ncol, win, ms, nnode, wkind, given, pats, kind):
    prob, block, prof, J = sc.problem(Ns, ncol, vlos=True)
    fld = sc.field(Ns, ncol)
    la0, nla = win
    mus, pats = fc.MUS[ms], sc.PATTERN_SETS[pats]
    e = make_engine(hip_lib, prob, block, prof, J)
    inst = ic.instrument_of(kind, ic.window_grid(prob, la0, nla))
    basis, base = fc.basis_of(Ns, nnode), fc.base_of(fld, nnode, given)
    truth = fc.nodes_of(fld, Ns, nnode, base)
    S_true = spectrum(e, mus, fithost.expand(Ns, nnode, basis, base, truth), pats, la0=la0, nla=nla)
    obs = e.apply_instrument(S_true, inst)
    assert obs.shape == (ncol, 4, inst.nobs, len(mus))
    sm = ic.smear_excess(obs, S_true, inst)
    nodes = fc.off_truth(truth, nnode)
    w = fc.weights_of(wkind, obs.shape)
    kw = dict(weight=w, base=base if given or 0 in nnode else None, patterns=pats, la0=la0, nla=nla, instrument=inst)
    ne = e.fit_field_normal(mus, basis, nnode, nodes, obs, amplitudes=fc.AMPS, **kw)
    assert same(ne.field, fithost.expand(Ns, nnode, basis, base, nodes))
    rf, S = response(e, mus, ne.field, nnode, pats, la0=la0, nla=nla)
    val, bar = ic.yardstick(nnode, rf, S, obs, w, basis, inst)
    x = fc.inside(dict(chi2=ne.chi2, grad=ne.grad, hess=ne.hess), val, bar)
    sig = fc.grad_signal(val, bar)
    print('Ns %d, nla %d, %s: nobs %d, width %d, M\' %d, P %d: deviation / bar %s, smear alone %.3g, largest |grad| / bar %.3g'
          % (Ns, nla, kind, inst.nobs, inst.width, 4 * inst.nobs * len(mus), sum(nnode), x, sm, sig))
    assert max(x.values()) <= 1.0 and sm <= 1.0 and sig >= fc.SIGNAL
    assert same(ne.hess, np.swapaxes(ne.hess, 1, 2))
    c2, f2 = e.fit_field_chi2(mus, basis, nnode, nodes, obs, **kw)
    assert same(c2, ne.chi2) and same(f2, ne.field)
    if w is not None:                     # a masked pixel's obs does not enter
        n2 = e.fit_field_normal(mus, basis, nnode, nodes, np.where(w > 0, obs, obs * 3.0 + 1.0), amplitudes=fc.AMPS, **kw)
        assert all(same(getattr(n2, k), getattr(ne, k)) for k in KEYS)
    if kind == 'identity':                # today's entry, as numbers
        n0 = e.fit_field_normal(mus, basis, nnode, nodes, obs, amplitudes=fc.AMPS, **dict(kw, instrument=None))
        assert all(np.array_equal(getattr(n0, k), getattr(ne, k)) for k in KEYS)
    e.close()


def _raw(e, prob, mus, pats, la0, nla, nnode, basis, nodes, obs, w, inst_ptr, chi2_only=False):
    """the new entries, raw: -> (rc, chi2, grad, hess)"""
    from lightspinner_amd import zeeman
    dll, h = e.lib.dll, e._h
    nc, al, st, sh = zeeman.pack(pats, prob.Nlines)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    mu, amp, nn = np.ascontiguousarray(mus, dtype=np.float64), np.full(3, 1e-3), np.array(nnode, dtype=np.int32)
    ob, x, bs = np.ascontiguousarray(obs), np.ascontiguousarray(nodes), np.ascontiguousarray(basis)
    wt = None if w is None else np.ascontiguousarray(w)
    ncol, P = x.shape
    out = [np.empty(ncol), np.empty((ncol, P)), np.empty((ncol, P, P))]
    if chi2_only:
        rc_ = dll.lsx_hip_instrument_fit_chi2(h, len(mu), dp(mu), 0, ncol, la0, nla, ip(nc), ip(al), dp(st), dp(sh), ip(nn), dp(bs), None,
                                              dp(x), dp(ob), dp(wt), dp(out[0]), None, inst_ptr)
    else:
        rc_ = dll.lsx_hip_instrument_fit_normal(h, len(mu), dp(mu), 0, ncol, la0, nla, ip(nc), ip(al), dp(st), dp(sh), ip(nn), dp(bs), None,
                                                dp(x), dp(amp), dp(ob), dp(wt), dp(out[0]), dp(out[1]), dp(out[2]), None, inst_ptr)
    return (rc_,) + tuple(out)


def test_bits(hip_lib, fithost):
    """a column's chi2, grad and hess through an instrument do not depend on the column range, on one column per group or pass under
    a small work cap (the fit's own, the response's, the Stokes pass's), or on the other columns' nodes and obs; the chi2 entry gives
    the normal entry's chi2; without an instrument the new entries are the existing ones; S' inside the fit is apply_instrument's"""
    Ns, ncol, nnode, la0, nla = 13, 3, (3, 3, 3), 7, 65
    prob, block, prof, J = sc.problem(Ns, ncol, vlos=True)
    fld = sc.field(Ns, ncol)
    pats = sc.PATTERN_SETS['blend']
    e = make_engine(hip_lib, prob, block, prof, J)
    inst = ic.instrument_of('gaussian', ic.window_grid(prob, la0, nla))
    basis = fc.basis_of(Ns, nnode)
    truth = fc.nodes_of(fld, Ns, nnode)
    mus = fc.MUS
    obs = e.apply_instrument(spectrum(e, mus, fithost.expand(Ns, nnode, basis, None, truth), pats, la0=la0, nla=nla), inst)
    nodes = fc.off_truth(truth, nnode)
    w = fc.weights_of('given', obs.shape)

    def call(x=nodes, o=obs, wt=w, **kw):
        return e.fit_field_normal(mus, basis, nnode, x, o, weight=wt, patterns=pats, la0=la0, nla=nla, amplitudes=fc.AMPS, instrument=inst, **kw)

    whole = call()
    assert same(whole.hess, np.swapaxes(whole.hess, 1, 2))
    for c in range(3):
        one = call(nodes[c:c + 1], obs[c:c + 1], w[c:c + 1], col0=c, ncol=1)
        assert all(same(getattr(one, k)[0], getattr(whole, k)[c]) for k in KEYS), c
    two = call(nodes[1:], obs[1:], w[1:], col0=1, ncol=2)
    assert all(same(getattr(two, k), getattr(whole, k)[1:]) for k in KEYS)
    assert all(same(getattr(call(work_cap_bytes=1), k), getattr(whole, k)) for k in KEYS)          # the fit's groups: one column each
    assert same(e.apply_instrument(np.ones((5, nla, 2)), inst), e.apply_instrument(np.ones((1, nla, 2)), inst).repeat(5, axis=0))      # (one row a group)
    call(work_cap_bytes=0)
    e.lib.check(e.lib.dll.lsx_hip_response_stokes_work_cap(e._h, 1))                                # one column a pass of the response
    e.lib.check(e.lib.dll.lsx_hip_stokes_rays_work_cap(e._h, 1))
    assert all(same(getattr(call(), k), getattr(whole, k)) for k in KEYS)
    c2 = e.fit_field_chi2(mus, basis, nnode, nodes, obs, weight=w, patterns=pats, la0=la0, nla=nla, instrument=inst)[0]
    assert same(c2, whole.chi2)
    e.lib.check(e.lib.dll.lsx_hip_response_stokes_work_cap(e._h, 0))
    e.lib.check(e.lib.dll.lsx_hip_stokes_rays_work_cap(e._h, 0))
    x2, o2 = nodes.copy(), obs.copy()
    x2[[0, 2]] = truth[[0, 2]] * 1.1
    o2[[0, 2]] *= 1.3
    other = call(x2, o2)
    assert all(same(getattr(other, k)[1], getattr(whole, k)[1]) for k in KEYS)
    assert not same(other.chi2[0], whole.chi2[0])
    o3 = np.where(w > 0, obs, obs * 3.0 + 1.0)                                                      # the obs of zero-weight pixels
    assert not same(o3, obs) and all(same(getattr(call(o=o3), k), getattr(whole, k)) for k in KEYS)
    # S' inside the fit is apply_instrument(stokes_rays(field_out)): chi2 == 0.0 exactly with that array as obs
    o4 = e.apply_instrument(spectrum(e, mus, whole.field, pats, la0=la0, nla=nla), inst)
    zero = call(o=o4)
    assert np.all(zero.chi2 == 0.0) and not np.any(zero.grad)
    assert np.all(e.fit_field_chi2(mus, basis, nnode, nodes, o4, weight=w, patterns=pats, la0=la0, nla=nla, instrument=inst)[0] == 0.0)
    # instrument = None through the new entries: the existing entries, bit for bit
    grid_obs = spectrum(e, mus, fithost.expand(Ns, nnode, basis, None, truth), pats, la0=la0, nla=nla)
    wg = fc.weights_of('given', grid_obs.shape)
    old = e.fit_field_normal(mus, basis, nnode, nodes, grid_obs, weight=wg, patterns=pats, la0=la0, nla=nla, amplitudes=fc.AMPS)
    rc_, chi2, grad, hess = _raw(e, prob, mus, pats, la0, nla, nnode, basis, nodes, grid_obs, wg, None)
    assert rc_ == sc.LSX_OK and same(chi2, old.chi2) and same(grad, old.grad) and same(hess, old.hess)
    rc_, chi2, _, _ = _raw(e, prob, mus, pats, la0, nla, nnode, basis, nodes, grid_obs, wg, None, chi2_only=True)
    assert rc_ == sc.LSX_OK and same(chi2, old.chi2)
    e.close()


def test_refusals(hip_lib, fithost):
    Ns, ncol, nnode = 5, 3, (2, 2, 2)
    prob, block, prof, J = sc.problem(Ns, ncol, vlos=True)
    fld = sc.field(Ns, ncol)
    patterns = sc.PATTERN_SETS['all']
    nla = prob.Nspect
    e = make_engine(hip_lib, prob, block, prof, J)
    e.formal_sol_gamma()
    before = [e.get(w).copy() for w in (_capi.LSX_I, _capi.LSX_J, _capi.LSX_N)]
    S0 = stack(e.stokes_rays(fc.MUS, *fld, patterns=patterns))
    basis = fc.basis_of(Ns, nnode)
    nodes = fc.nodes_of(fld, Ns, nnode)
    good = ic.instrument_of('gaussian', ic.window_grid(prob, 0, nla))
    obs = e.apply_instrument(S0, good) * 1.01
    EINVAL, EUNS = sc.LSX_EINVAL, sc.LSX_EUNSUPPORTED
    e.fit_field_normal(fc.MUS, basis, nnode, nodes, obs, patterns=patterns, instrument=good)

    def struct(nobs, width, first, weight):
        f = None if first is None else np.ascontiguousarray(first, dtype=np.int32)
        w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64)
        st = _capi.LsxFitInstrument(nobs, width, None if f is None else f.ctypes.data_as(C.POINTER(C.c_int32)),
                                    None if w is None else w.ctypes.data_as(C.POINTER(C.c_double)))
        return st, (f, w)

    def refused(code, st, word=None, o=obs, wt=None, mus=fc.MUS):
        """all three entries refuse the instrument with `code` (apply has no obs to refuse)"""
        ptr = C.byref(st[0])
        for chi2_only in (False, True):
            rc_ = _raw(e, prob, mus, patterns, 0, nla, nnode, basis, nodes, o, wt, ptr, chi2_only)[0]
            assert rc_ == code, (rc_, last_error(e))
            assert word is None or word in last_error(e), last_error(e)
        return ptr

    def apply_refused(code, st, word=None):
        x, out = np.ones((4, nla, 3)), np.empty((4, max(st[0].nobs, 1), 3))
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        rc_ = e.lib.dll.lsx_hip_instrument_apply(e._h, C.byref(st[0]), nla, 3, 4, dp(x), dp(out))
        assert rc_ == code, (rc_, last_error(e))
        assert word is None or word in last_error(e), last_error(e)

    nobs, width = good.nobs, good.width
    f_hi, f_lo = good.first.copy(), good.first.copy()
    f_hi[3], f_lo[5] = nla - width + 1, -1
    w_nan, w_inf = good.weight.copy(), good.weight.copy()
    w_nan[2, 1], w_inf[0, 0] = np.nan, -np.inf
    for st, word in ((struct(0, width, good.first, good.weight), 'nobs'), (struct(-3, width, good.first, good.weight), 'nobs'),
                     (struct(nobs, 0, good.first, good.weight), 'width'), (struct(nobs, nla + 1, good.first, good.weight), 'width'),
                     (struct(nobs, width, f_hi, good.weight), 'pixel 3'), (struct(nobs, width, f_lo, good.weight), 'pixel 5'),
                     (struct(nobs, width, good.first, w_nan), 'not finite'), (struct(nobs, width, good.first, w_inf), 'not finite'),
                     (struct(nobs, width, None, good.weight), 'null'), (struct(nobs, width, good.first, None), 'null')):
        refused(EINVAL, st, word)
        apply_refused(EINVAL, st, word)
    # 4 nobs nmu over the limit that 4 nla nmu has: refused before first and weight are read (their arrays are not that long)
    big = struct((2 ** 31 - 1) // 2 // 12 + 1, width, good.first, good.weight)
    refused(EUNS, big)
    # everything the existing entries refuse, obs and weight at their new size
    st = struct(nobs, width, good.first, good.weight)
    for bad in (np.nan, np.inf):
        o = obs.copy()
        o[2, 3, -1, 2] = bad
        refused(EINVAL, st, 'obs', o=o)
        wt = np.ones_like(obs)
        wt[1, 2, -1, 0] = bad
        refused(EINVAL, st, 'weight', wt=wt)
    wt = np.ones_like(obs)
    wt[0, 0, 0, 0] = -1e-300
    refused(EINVAL, st, 'negative', wt=wt)
    refused(EINVAL, st, mus=np.array([0.0, 0.5, 1.0]))
    with pytest.raises(_capi.LsxError) as ei:
        e.fit_field_normal(fc.MUS, basis, nnode, nodes, obs, patterns=patterns, instrument=good, la0=-1, nla=nla)
    assert ei.value.code == EINVAL
    with pytest.raises(_capi.LsxError) as ei:
        e.fit_field_normal(fc.MUS, basis, nnode, nodes[:2], obs[:2], patterns=patterns, instrument=good, col0=2, ncol=2)
    assert ei.value.code == EINVAL
    x = nodes.copy()
    x[2, 0] = 2e-4                                        # 0 <= B < a_B / 2: the response's rule, of the expanded field
    with pytest.raises(_capi.LsxError) as ei:
        e.fit_field_normal(fc.MUS, basis, nnode, x, obs, patterns=patterns, instrument=good, amplitudes={'B': 1e-3})
    assert ei.value.code == EINVAL and 'column 2, depth 0' in str(ei.value)
    # apply's own; the wrapper's
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    x4, out = np.ones((4, nla, 3)), np.empty((4, nobs, 3))
    ptr = C.byref(st[0])
    assert e.lib.dll.lsx_hip_instrument_apply(e._h, ptr, nla, 3, 4, dp(x4), dp(out)) == sc.LSX_OK
    for args in ((None, nla, 3, 4, dp(x4), dp(out)), (ptr, nla, 3, 4, None, dp(out)), (ptr, nla, 3, 4, dp(x4), None), (ptr, 0, 3, 4, dp(x4), dp(out)),
                 (ptr, nla, 0, 4, dp(x4), dp(out)), (ptr, nla, 3, 0, dp(x4), dp(out)), (ptr, width - 1, 3, 4, dp(x4), dp(out))):
        assert e.lib.dll.lsx_hip_instrument_apply(e._h, *args) == EINVAL
    with pytest.raises(ValueError):
        e.apply_instrument(np.ones((4, nla - 1, 3)), good)          # made for another window
    with pytest.raises(ValueError):
        e.fit_field_normal(fc.MUS, basis, nnode, nodes, obs, patterns=patterns, instrument=good, la0=1, nla=nla - 1)
    for w_, b_ in zip((_capi.LSX_I, _capi.LSX_J, _capi.LSX_N), before):
        assert np.array_equal(e.get(w_), b_)
    assert same(stack(e.stokes_rays(fc.MUS, *fld, patterns=patterns)), S0)
    e.close()


@pytest.mark.parametrize('kind', ['a', 'b'])
@pytest.mark.parametrize('Ns,nn,mus', [(13, 2, [1.0, 0.6]), (13, 2, 'three columns')])
def test_the_loop_recovers_a_known_field_through_an_instrument(hip_lib, fithost, Ns, nn, mus, kind):
    ncol = 3 if mus == 'three columns' else 1
    mus = np.array([1.0] if ncol == 3 else mus)
    (prob, block, prof, J), pats, fld, nnode, basis, truth, start = fc.recovery(Ns, ncol, nn)
    e = make_engine(hip_lib, prob, block, prof, J)
    la0, nla = fc.RECOVERY_WINDOW
    inst = ic.recovery_instrument(ic.window_grid(prob, la0, nla), kind)
    obs = e.apply_instrument(spectrum(e, mus, np.stack(fld, axis=1), pats, la0=la0, nla=nla), inst)
    w = fc.recovery_weight(obs)
    kw = dict(amplitudes=fc.AMPS, patterns=pats, la0=la0, nla=nla, instrument=inst, **fc.RECOVERY_LOOP)
    r = drivers.fit_field_columns(e, obs, mus, basis, start, nnode, weight=w, **kw)
    print('(%s) Ns %d, %d nodes, %d angles, %d columns: chi2 %s -> %s in %s iterations, node error %.3g, lambda %s'
          % (kind, Ns, nn, len(mus), ncol, r.history[0], r.chi2, r.iterations, np.max(np.abs(r.nodes - truth)), r.lam))
    fc.check_recovery(r, truth)
    assert same(r.field, fithost.expand(Ns, nnode, basis, None, r.nodes))
    if ncol == 3:           # a column fitted alone takes the path it takes among three, bit for bit
        one = drivers.fit_field_columns(e, obs[1:2], mus, basis, start[1:2], nnode, weight=w[1:2], col0=1, ncol=1, **kw)
        assert same(one.nodes[0], r.nodes[1]) and same(one.history[:, 0], r.history[:len(one.history), 1])
    e.close()


# ---- FALC Ca II ------------------------------------------------------------------------------------------------------------------------
FALC_FWHM = 4.0          # x the window's smallest spacing (the issue's value; DESIGN.md "How the instrument is pinned")


def test_falc_caii_8542(hip_lib):
    """the fixture, field, start and angles of test_fit.py::test_falc_caii_8542 behind nla // 2 uniform pixels and a Gaussian of fwhm
    4 x the window's smallest spacing; obs from apply_instrument.  Asserted as there: chi2 never rises and ends <= 1e-6 x the first."""
    from test_stokes import FALC_MUS, falc, falc_engine
    prob, block, prof, n, J, (la0, nla), line = falc()
    e, fld = falc_engine(hip_lib)
    pats = [None] * prob.Nlines
    pats[line] = sc.TRIPLET
    Ns, nnode = prob.Nspace, (1, 1, 1)
    basis = np.ones((3, Ns))
    grid = ic.window_grid(prob, la0, nla)
    inst = fit.Instrument.gaussian(grid, ic.uniform_pixels(grid, nla // 2), FALC_FWHM * float(np.min(np.diff(grid))))
    S_true = stack(e.stokes_rays(FALC_MUS, *fld, patterns=pats, la0=la0, nla=nla))
    obs = e.apply_instrument(S_true, inst)
    assert ic.smear_excess(obs, S_true, inst) <= 1.0
    w = fc.recovery_weight(obs)
    start = np.array([[0.11, np.deg2rad(50.0), np.deg2rad(25.0)]])
    kw = dict(weight=w, patterns=pats, la0=la0, nla=nla, instrument=inst)
    ne = e.fit_field_normal(FALC_MUS, basis, nnode, start, obs, **kw)
    rf, S = response(e, FALC_MUS, ne.field, nnode, pats, amplitudes=None, la0=la0, nla=nla)
    val, bar = ic.yardstick(nnode, rf, S, obs, w, basis, inst)
    x = fc.inside(dict(chi2=ne.chi2, grad=ne.grad, hess=ne.hess), val, bar)
    print('FALC Ca II 854.2 nm, %d wavelengths -> %d pixels of width %d, %d depths: deviation / bar %s, |grad| / bar %.3g'
          % (nla, inst.nobs, inst.width, Ns, x, fc.grad_signal(val, bar)))
    assert max(x.values()) <= 1.0 and fc.grad_signal(val, bar) >= fc.SIGNAL
    assert same(e.fit_field_chi2(FALC_MUS, basis, nnode, start, obs, **kw)[0], ne.chi2)
    r = drivers.fit_field_columns(e, obs, FALC_MUS, basis, start, nnode, **kw)
    print('FALC fit through the instrument: chi2 %.6e -> %.6e, %d iterations, status %d, B %.9f T, gammaB %.7f deg, chiB %.7f deg, lambda %.1e'
          % (r.history[0, 0], r.chi2[0], r.iterations[0], r.status[0], r.nodes[0, 0], *np.rad2deg(r.nodes[0, 1:]), r.lam[0]))
    assert np.all(np.diff(r.history[:, 0]) <= 0) and r.chi2[0] <= 1e-6 * r.history[0, 0]
    e.close()


def test_context_takes_the_instrument(hip_lib):
    """Context.fit_field(..., instrument=) is the driver on the engine; Context.compute_stokes(..., instrument=) is apply_instrument
    of compute_stokes"""
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
    la0, nla = int(trans[kr].Nblue), int(trans[kr].wavelength.shape[0])
    grid = np.asarray(ctx.problem.wavelength, dtype=np.float64)[la0:la0 + nla]
    inst = fit.Instrument.gaussian(grid, ic.uniform_pixels(grid, nla // 2), FALC_FWHM * float(np.min(np.diff(grid))))
    st = ctx.compute_stokes(mus, np.full(Ns, 0.1), 0.7, 0.5, transition=trans[kr])
    seen = ctx.compute_stokes(mus, np.full(Ns, 0.1), 0.7, 0.5, transition=trans[kr], instrument=inst)
    obs = np.stack([seen.I, seen.Q, seen.U, seen.V])
    assert obs.shape == (4, inst.nobs, 2)
    assert same(obs, ctx._engine.apply_instrument(np.stack([st.I, st.Q, st.U, st.V]), inst))
    one = ctx.compute_stokes(0.6, np.full(Ns, 0.1), 0.7, 0.5, transition=kr, instrument=inst)
    assert one.V.shape == (inst.nobs,) and same(one.V, seen.V[:, 1])
    w = 1.0 / (1e-3 * obs[0].max()) ** 2
    hats = fit.hat_basis(np.arange(Ns), [0.0, Ns - 1.0])
    start = np.array([0.105, 0.105, 0.75, 0.45])
    r = ctx.fit_field(mus, obs, transition=trans[kr], basis={'B': hats, 'gammaB': np.ones(Ns), 'chiB': np.ones(Ns)}, start=start, weight=w,
                      max_iter=4, instrument=inst)
    pats = [zeeman.zeeman_components(t.transModel) for t in trans if t.isLine]
    basis, nnode = fit.stack_basis(B=hats, gammaB=np.ones(Ns), chiB=np.ones(Ns))
    ref = drivers.fit_field_columns(ctx._engine, obs[None], np.array(mus), basis, start[None], nnode, weight=np.full((1,) + obs.shape, w),
                                    patterns=pats, la0=la0, nla=nla, max_iter=4, instrument=inst)
    assert same(r.nodes, ref.nodes[0]) and same(r.history, ref.history[:, 0]) and same(r.field, ref.field[0])
    assert r.iterations == ref.iterations[0] and r.status == ref.status[0] and r.history[-1] < r.history[0]
    assert np.array_equal(ctx.I, I0) and np.array_equal(ctx.J, J0) and all(np.array_equal(a.n, b) for a, b in zip(ctx.activeAtoms, n0))
    ctx.close()
