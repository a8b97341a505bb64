"""The line-of-sight velocity as a quantity of the call on the GPU (include/lsx_hip_stokes_velocity.h): lsx_hip_velocity_stokes_rays
against the host window of the same velocity inside stokes_cases.bars; lsx_hip_velocity_response_stokes against both brute forces
(the host's, and the GPU's own Engine.stokes_rays(vlos=...) differences) inside (bar(S+) + bar(S-)) / a with the response at least
1000 x the bar; lsx_hip_velocity_fit_normal / _chi2 against fit_cases.yardstick; the bits under every cut of a call and against the
entries without a velocity; drivers.fit_field_columns recovering a field and a velocity within the host loop's count + 2; FALC Ca II
854.2 nm with a 1.5 km/s shift; Context.fit_field.  The yardsticks are those of tests/velocity_cases.py: nothing new is typed in."""
import dataclasses

import numpy as np
import pytest

import fit_cases as fc
import fit_instrument_cases as fic
import stokes_cases as sc
import stokes_response_cases as rc
import velocity_cases as vc
from conftest import golden
from lightspinner_amd import _capi, drivers, fit, synth
from lightspinner_amd.problem import Engine

pytestmark = pytest.mark.gpu
same = vc.same
MUS = vc.MUS


@pytest.fixture(scope='module')
def host():
    return vc.HostLib()


@pytest.fixture(scope='module')
def fithost():
    return vc.FitHostLib()


def make_engine(hip_lib, prob, block, prof, J):
    e = Engine(prob, block.ncol, lib=hip_lib)
    synth.load_columns(e, block, prof)
    e.set(_capi.LSX_J, J)
    return e


def stack(r):
    return np.stack([r.I, r.Q, r.U, r.V], axis=1)          # [ncol][4][nla][nmu]


def with_velocity(prof, vel):
    """the profile inputs as the host sees a call with the velocity `vel`: the kept broadening arrays and that velocity"""
    return (prof[0], prof[1], vel)


# Ns, columns, the context's own profiles (with a velocity / compact), patterns: 3 and 4 depths put every depth into the start-value and
# the end-point sets of the response at once, 5 parts them; 'none': no line has a pattern and the velocity still moves I
SHAPES = [(3, 1, False, False, 'triplet'), (4, 3, True, False, 'all'), (5, 3, False, True, 'blend'), (5, 1, False, False, 'none')]


@pytest.mark.parametrize('Ns,ncol,vlos,compact,pats', SHAPES)
def test_stokes_with_a_given_velocity(hip_lib, host, Ns, ncol, vlos, compact, pats):
    """every window at one and three angles, one and three columns with different velocities; the compact column leaves the branch
    that reads the context's profile store: the host run never reads one"""
    prob, block, prof, J = sc.problem(Ns, ncol, vlos=vlos, compact=compact)
    fld, vel, patterns = sc.field(Ns, ncol), vc.velocity(Ns, ncol), sc.PATTERN_SETS[pats]
    e = make_engine(hip_lib, prob, block, prof, J)
    ref = sc.runs(host, prob, block, with_velocity(prof, vel), block.n, J, fld, patterns, MUS)
    own = stack(e.stokes_rays(MUS, *fld, patterns=patterns))
    assert sc.excess(own, ref)[0] > 1.0                      # the velocity is seen: the context's own spectrum is outside the bar
    worst = 0.0
    for la0, nla in vc.WINDOWS:
        for ms in ([0], [0, 1, 2]):
            x = stack(e.stokes_rays(MUS[ms], *fld, patterns=patterns, la0=la0, nla=nla, vlos=vel))
            ex, rel = sc.excess(x, {u: r[:, :, la0:la0 + nla][..., ms] for u, r in ref.items()})
            worst = max(worst, ex)
            assert ex <= 1.0, (la0, nla, ms, ex, rel)
    whole = stack(e.stokes_rays(MUS, *fld, patterns=patterns, la0=7, nla=64, vlos=vel))
    for c in range(ncol):
        one = stack(e.stokes_rays(MUS, *(f[c:c + 1] for f in fld), patterns=patterns, la0=7, nla=64, vlos=vel[c:c + 1], col0=c, ncol=1))
        assert same(one[0], whole[c]), c
    print('Ns %d ncol %d %s: worst deviation / bar %.3g' % (Ns, ncol, pats, worst))
    e.close()


def test_the_columns_own_velocity_gives_the_bits_of_the_pass_without_one(hip_lib):
    prob, block, prof, J = sc.problem(5, 3, vlos=True)
    fld, patterns = sc.field(5, 3), sc.PATTERN_SETS['all']
    e = make_engine(hip_lib, prob, block, prof, J)
    for la0, nla in ((0, 65), (7, 130)):
        a = stack(e.stokes_rays(MUS, *fld, patterns=patterns, la0=la0, nla=nla))
        b = stack(e.stokes_rays(MUS, *fld, patterns=patterns, la0=la0, nla=nla, vlos=prof[2]))
        assert same(a, b)
    e.close()


# ---- the response ----------------------------------------------------------------------------------------------------------------------
def host_brute(host, prob, block, prof, n, J, fld, patterns, mus, la0, nla, parameters, amps, ks=None, lower_zero=False, cols=None):
    """-> (rf, bar), each {name: [ncol][4][nla][nk][nmu]}: rc.brute per column and angle (prof carries the call's velocity)"""
    cols = range(block.ncol) if cols is None else cols
    rf, bar = {p: [] for p in parameters}, {p: [] for p in parameters}
    for c in cols:
        cc = sc.column(prob, block, prof, n, J, fld, patterns, c, la0, nla, lower_zero)
        per = [rc.brute(host, cc, mu, parameters=parameters, amplitudes=amps, ks=ks) for mu in mus]
        for p in parameters:
            rf[p].append(np.stack([r[0][p] for r in per], axis=-1))
            bar[p].append(np.stack([r[1][p] for r in per], axis=-1))
    return {p: np.stack(v) for p, v in rf.items()}, {p: np.stack(v) for p, v in bar.items()}


def gpu_brute(e, mus, fld, vel, patterns, la0, nla, parameters, amps, ks, **kw):
    """-> {name: [ncol][4][nla][nk][nmu]}: central differences of Engine.stokes_rays(vlos=...), the depth changed in every column"""
    out = {}
    for p in parameters:
        i, a, r = vc.PARAMS.index(p), amps[p], []
        for k in ks:
            S = []
            for sg in (1, -1):
                f = [np.array(t) for t in fld] + [np.array(vel)]
                f[i][:, k] = f[i][:, k] + 0.5 * a if sg > 0 else f[i][:, k] - 0.5 * a
                S.append(stack(e.stokes_rays(mus, f[0], f[1], f[2], patterns=patterns, la0=la0, nla=nla, vlos=f[3], **kw)))
            r.append((S[0] - S[1]) / a)
        out[p] = np.stack(r, axis=-2)
    return out


@pytest.mark.parametrize('Ns,ncol,vlos,compact,pats', SHAPES)
def test_response_against_both_brute_forces(hip_lib, host, Ns, ncol, vlos, compact, pats):
    """all four parameters at once and 'vlos' alone, all depths and a subset, every window, one and three angles; .stokes has the bits
    of stokes_rays(vlos=...).  The host's brute force is made once on the whole grid"""
    prob, block, prof, J = sc.problem(Ns, ncol, vlos=vlos, compact=compact)
    fld, vel, patterns = sc.field(Ns, ncol), vc.velocity(Ns, ncol), sc.PATTERN_SETS[pats]
    amps = vc.amps(prof[1])
    e = make_engine(hip_lib, prob, block, prof, J)
    names = ['vlos'] if pats == 'none' else list(vc.PARAMS)
    ref, bar = host_brute(host, prob, block, with_velocity(prof, vel), block.n, J, fld, patterns, MUS, 0, prob.Nspect, names, amps)
    for p in names:
        assert rc.signal(ref[p], bar[p]) >= vc.SIGNAL, (p, rc.signal(ref[p], bar[p]))
    worst = {p: 0.0 for p in names}
    sub_ks = [0, Ns - 2]
    for la0, nla in vc.WINDOWS:
        for ms in ([0], [0, 1, 2]):
            r = e.stokes_response(MUS[ms], *fld, patterns=patterns, parameters=names, amplitudes=amps, la0=la0, nla=nla, vlos=vel)
            assert same(stack(r.stokes), stack(e.stokes_rays(MUS[ms], *fld, patterns=patterns, la0=la0, nla=nla, vlos=vel)))
            alone = e.stokes_response(MUS[ms], *fld, patterns=patterns, parameters='vlos', amplitudes=amps, la0=la0, nla=nla, vlos=vel, ks=sub_ks)
            assert list(alone.rf) == ['vlos'] and same(alone.rf['vlos'], r.rf['vlos'][..., sub_ks, :])
            gb = gpu_brute(e, MUS[ms], fld, vel, patterns, la0, nla, names, amps, range(Ns)) if (la0, nla) in ((0, 65), (0, 1)) else None
            sub = lambda a: a[:, :, la0:la0 + nla][..., ms]
            for p in names:
                x = rc.ratio(r.rf[p], sub(ref[p]), sub(bar[p]))
                worst[p] = max(worst[p], x)
                assert x <= 1.0, (p, la0, nla, ms, x)
                if gb is not None:
                    x = rc.ratio(r.rf[p], gb[p], sub(bar[p]))
                    assert x <= 1.0, ('gpu brute force', p, la0, nla, ms, x)
    print('Ns %d ncol %d %s: worst deviation / bar' % (Ns, ncol, pats), worst)
    e.close()


def test_response_forty_depths(hip_lib, host):
    """40 depths on the window [7, 72), where the transfer matrix carries most responses: RF_vlos of the middle one of three columns"""
    Ns, ncol, la0, nla = 40, 3, 7, 65
    prob, block, prof, J = sc.problem(Ns, ncol, vlos=True)
    fld, vel, patterns = sc.field(Ns, ncol), vc.velocity(Ns, ncol), sc.PATTERN_SETS['blend']
    amps = vc.amps(prof[1])
    e = make_engine(hip_lib, prob, block, prof, J)
    mus = MUS[:2]
    ref, bar = host_brute(host, prob, block, with_velocity(prof, vel), block.n, J, fld, patterns, mus, la0, nla, ['vlos'], amps, cols=[1])
    r = e.stokes_response(mus, *fld, patterns=patterns, parameters=vc.PARAMS, amplitudes=amps, la0=la0, nla=nla, vlos=vel)
    gb = gpu_brute(e, mus, fld, vel, patterns, la0, nla, ['vlos'], amps, range(Ns))
    assert rc.signal(ref['vlos'], bar['vlos']) >= vc.SIGNAL
    xh, xg = rc.ratio(r.rf['vlos'][1:2], ref['vlos'], bar['vlos']), rc.ratio(r.rf['vlos'][1:2], gb['vlos'][1:2], bar['vlos'])
    print('40 depths, vlos: deviation / bar %.3g (host brute force) %.3g (GPU brute force)' % (xh, xg))
    assert xh <= 1.0 and xg <= 1.0
    e.close()


def test_response_under_a_zero_lower_boundary(hip_lib, host):
    prob, block, prof, J = sc.problem(5, 1, vlos=True)
    fld, vel, patterns = sc.field(5, 1), vc.velocity(5, 1), sc.PATTERN_SETS['blend']
    amps = vc.amps(prof[1])
    e = make_engine(hip_lib, prob, block, prof, J)
    e.set_boundary('zero', 'zero')
    pv = with_velocity(prof, vel)
    ref, bar = host_brute(host, prob, block, pv, block.n, J, fld, patterns, MUS, 0, prob.Nspect, vc.PARAMS, amps, lower_zero=True)
    thermal, _ = host_brute(host, prob, block, pv, block.n, J, fld, patterns, MUS, 0, prob.Nspect, ['vlos'], amps)
    r = e.stokes_response(MUS, *fld, patterns=patterns, parameters=vc.PARAMS, amplitudes=amps, vlos=vel)
    gb = gpu_brute(e, MUS, fld, vel, patterns, 0, prob.Nspect, vc.PARAMS, amps, range(5))
    for p in vc.PARAMS:
        assert rc.signal(ref[p], bar[p]) >= vc.SIGNAL
        assert rc.ratio(r.rf[p], ref[p], bar[p]) <= 1.0 and rc.ratio(r.rf[p], gb[p], bar[p]) <= 1.0, p
    assert rc.ratio(thermal['vlos'], ref['vlos'], bar['vlos']) > 1.0          # the boundary is seen
    e.close()


def test_response_bits(hip_lib):
    """rf does not depend on the column range, on one column per pass under a small work cap, on the window's cut, on the other angles
    or on the set of requested parameters; on a column built with a velocity that is handed over, the rows of B, gammaB, chiB are the
    entry's without a velocity"""
    Ns, ncol, la0, nla = 13, 3, 7, 130
    prob, block, prof, J = sc.problem(Ns, ncol, vlos=True)
    fld, vel, patterns = sc.field(Ns, ncol), vc.velocity(Ns, ncol), sc.PATTERN_SETS['blend']
    amps = vc.amps(prof[1])
    e = make_engine(hip_lib, prob, block, prof, J)
    call = lambda mus=MUS, f=fld, v=vel, names=vc.PARAMS, **kw: e.stokes_response(mus, *f, patterns=patterns, parameters=names, amplitudes=amps,
                                                                                  vlos=v, **dict(dict(la0=la0, nla=nla), **kw))
    whole = call()
    W = rc.stack_rf(whole, vc.PARAMS)
    for c in range(ncol):
        one = call(f=[t[c:c + 1] for t in fld], v=vel[c:c + 1], col0=c, ncol=1)
        assert same(rc.stack_rf(one, vc.PARAMS)[0], W[c]), c
    assert same(rc.stack_rf(call(work_cap_bytes=1), vc.PARAMS), W)
    call(work_cap_bytes=0)
    cut = call(la0=la0 + 30, nla=70)
    assert same(rc.stack_rf(cut, vc.PARAMS), W[:, :, :, 30:100])
    assert same(rc.stack_rf(call(mus=MUS[1:2]), vc.PARAMS), W[..., 1:2])
    for names in (['vlos'], ['B', 'vlos'], ['gammaB', 'chiB']):
        r = call(names=names)
        assert list(r.rf) == names and all(same(r.rf[p], whole.rf[p]) for p in names), names
    own = call(v=prof[2])
    old = e.stokes_response(MUS, *fld, patterns=patterns, amplitudes=rc.AMPS, la0=la0, nla=nla)
    assert all(same(own.rf[p], old.rf[p]) for p in rc.PARAMS) and same(stack(own.stokes), stack(old.stokes))
    e.close()


def test_refusals(hip_lib):
    Ns, ncol = 5, 3
    prob, block, prof, J = sc.problem(Ns, ncol, vlos=True)
    fld, vel, patterns = sc.field(Ns, ncol), vc.velocity(Ns, ncol), sc.PATTERN_SETS['all']
    e = make_engine(hip_lib, prob, block, prof, J)
    S0 = stack(e.stokes_rays(MUS, *fld, patterns=patterns))

    def refused(f, word=None):
        with pytest.raises(_capi.LsxError) as ei:
            f()
        assert ei.value.code == sc.LSX_EINVAL, (ei.value.code, str(ei.value))
        assert word is None or word in str(ei.value), str(ei.value)

    nnode = (1, 1, 1, 1)
    basis, obs = np.ones((4, Ns)), S0 * 1.01
    nodes = np.tile([0.1, 0.5, 0.3, 100.0], (ncol, 1))
    e.fit_field_normal(MUS, basis, nnode, nodes, obs, patterns=patterns)
    for bad in (np.nan, np.inf, -np.inf):
        v = vel.copy()
        v[1, 2] = bad
        refused(lambda: e.stokes_rays(MUS, *fld, patterns=patterns, vlos=v), 'vlos')
        refused(lambda: e.stokes_response(MUS, *fld, patterns=patterns, vlos=v), 'vlos')
        x = nodes.copy()
        x[1, 3] = bad
        refused(lambda: e.fit_field_normal(MUS, basis, nnode, x, obs, patterns=patterns))
        refused(lambda: e.fit_field_chi2(MUS, basis, nnode, x, obs, patterns=patterns))
        bs = np.zeros((ncol, 4, Ns))
        bs[2, 3, 1] = bad
        refused(lambda: e.fit_field_normal(MUS, basis, nnode, nodes, obs, base=bs, patterns=patterns), 'base')
    for bad in (0.0, -1.0, np.nan, np.inf):
        refused(lambda: e.stokes_response(MUS, *fld, patterns=patterns, parameters=vc.PARAMS, amplitudes={'vlos': bad}, vlos=vel), 'vlos')
        refused(lambda: e.fit_field_normal(MUS, basis, nnode, nodes, obs, patterns=patterns, amplitudes={'vlos': bad}), 'vlos')
        e.stokes_response(MUS, *fld, patterns=patterns, parameters=rc.PARAMS, amplitudes={'vlos': bad}, vlos=vel)      # not requested: not read
    with pytest.raises(ValueError):
        e.fit_field_normal(MUS, np.ones((5, Ns)), (1, 1, 1, 1, 1), np.zeros((ncol, 5)), obs, patterns=patterns)
    r = e.stokes_response(MUS, *fld, patterns=patterns, parameters=['vlos'])          # requested without a velocity: zeros
    assert same(r.rf['vlos'], e.stokes_response(MUS, *fld, patterns=patterns, parameters=['vlos'], vlos=0.0).rf['vlos'])
    assert r.amplitudes == {'vlos': 100.0}
    assert same(stack(e.stokes_rays(MUS, *fld, patterns=patterns)), S0)
    e.close()


# ---- the normal equations ----------------------------------------------------------------------------------------------------------------
def response4(e, mus, field, nnode, pats, amps, **kw):
    """-> rf [ncol][npar][4][nla][Ns][nmu], S [ncol][4][nla][nmu] of Engine.stokes_response for the fitted quantities"""
    names = [p for p, n in zip(vc.PARAMS, nnode) if n > 0]
    r = e.stokes_response(mus, field[:, 0], field[:, 1], field[:, 2], patterns=pats, parameters=names, amplitudes=amps, vlos=field[:, 3], **kw)
    return rc.stack_rf(r, names), stack(r.stokes)


@pytest.mark.parametrize('nnode', [(0, 0, 0, 1), (2, 2, 2, 2), (6, 6, 6, 6)])
@pytest.mark.parametrize('wkind', [None, 'given'])
@pytest.mark.parametrize('through', [False, True])
def test_normal_equations(hip_lib, fithost, nnode, wkind, through):
    Ns, ncol, la0, nla = 13, 3, 7, 65
    mus = MUS[:2]
    prob, block, prof, J = sc.problem(Ns, ncol, vlos=True)
    fld4 = list(sc.field(Ns, ncol)) + [vc.velocity(Ns, ncol)]
    pats = sc.PATTERN_SETS['blend']
    vB, amps = float(np.min(prof[1])), vc.amps(prof[1])
    e = make_engine(hip_lib, prob, block, prof, J)
    basis, base = vc.basis_of(Ns, nnode), vc.base_of(fld4, nnode, False)
    truth = vc.nodes_of(fld4, Ns, nnode, base)
    ft = fithost.expand4(Ns, nnode, basis, base, truth)
    inst = vc.recovery_instrument(prob, (la0, nla)) if through else None
    obs = stack(e.stokes_rays(mus, ft[:, 0], ft[:, 1], ft[:, 2], patterns=pats, la0=la0, nla=nla, vlos=ft[:, 3]))
    if through:
        obs = e.apply_instrument(obs, inst)
    nodes = vc.off_truth(truth, nnode, vB)
    w = fc.weights_of(wkind, obs.shape)
    kw = dict(weight=w, base=base, patterns=pats, la0=la0, nla=nla, instrument=inst)
    ne = e.fit_field_normal(mus, basis, nnode, nodes, obs, amplitudes=amps, **kw)
    assert same(ne.field, fithost.expand4(Ns, nnode, basis, base, nodes))
    rf, S = response4(e, mus, ne.field, nnode, pats, amps, la0=la0, nla=nla)
    val, bar = fic.yardstick(nnode, rf, S, obs, w, basis, inst) if through else fc.yardstick(nnode, rf, S, obs, w, basis)
    x = fc.inside(dict(chi2=ne.chi2, grad=ne.grad, hess=ne.hess), val, bar)
    sig = fc.grad_signal(val, bar)
    print('nnode %s, weights %s, instrument %s: deviation / bar %s, largest |grad| / bar %.3g' % (nnode, wkind, through, x, sig))
    assert max(x.values()) <= 1.0 and sig >= fc.SIGNAL
    assert same(ne.hess, np.swapaxes(ne.hess, 1, 2))
    c2, f2 = e.fit_field_chi2(mus, basis, nnode, nodes, obs, **kw)
    assert same(c2, ne.chi2) and same(f2, ne.field)
    e.close()


def test_without_velocity_nodes_the_sums_are_the_old_entrys(hip_lib, fithost):
    """nnode[3] = 0 and base_3 the velocity the columns were built with: chi2, grad and hess of lsx_hip_fit_field_normal, bit for bit"""
    Ns, ncol, la0, nla, nnode = 13, 3, 7, 65, (2, 2, 2)
    prob, block, prof, J = sc.problem(Ns, ncol, vlos=True)
    fld, pats = sc.field(Ns, ncol), sc.PATTERN_SETS['blend']
    e = make_engine(hip_lib, prob, block, prof, J)
    basis = fc.basis_of(Ns, nnode)
    truth = fc.nodes_of(fld, Ns, nnode)
    obs = stack(e.stokes_rays(MUS, *fld, patterns=pats, la0=la0, nla=nla))
    nodes = fc.off_truth(truth, nnode)
    w = fc.weights_of('given', obs.shape)
    kw = dict(weight=w, patterns=pats, la0=la0, nla=nla, amplitudes=fc.AMPS)
    old = e.fit_field_normal(MUS, basis, nnode, nodes, obs, **kw)
    base = np.zeros((ncol, 4, Ns))
    base[:, 3] = prof[2]
    new = e.fit_field_normal(MUS, basis, nnode + (0,), nodes, obs, base=base, **kw)
    assert all(same(getattr(new, k), getattr(old, k)) for k in ('chi2', 'grad', 'hess'))
    assert same(new.field[:, :3], old.field) and same(new.field[:, 3], prof[2])
    e.close()


# ---- the loop ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', range(len(vc.RECOVERY_CASES)))
def test_the_loop_recovers_field_and_velocity(hip_lib, fithost, case):
    Ns, nn, mus, ncol, through = vc.RECOVERY_CASES[case]
    mus = np.array(mus)
    (prob, block, prof, J), pats, fld4, nnode, basis, truth, start, vB = vc.recovery(Ns, ncol, nn)
    e = make_engine(hip_lib, prob, block, prof, J)
    la0, nla = vc.RECOVERY_WINDOW
    inst = vc.recovery_instrument(prob) if through else None
    obs = stack(e.stokes_rays(mus, *fld4[:3], patterns=pats, la0=la0, nla=nla, vlos=fld4[3]))
    if through:
        obs = e.apply_instrument(obs, inst)
    w = fc.recovery_weight(obs)
    cap = vc.max_iter(case)
    kw = dict(amplitudes=vc.amps(prof[1]), patterns=pats, la0=la0, nla=nla, max_iter=cap, **vc.RECOVERY_LOOP)
    if through:
        kw['instrument'] = inst
    r = drivers.fit_field_columns(e, obs, mus, basis, start, nnode, weight=w, **kw)
    o = 3 * nn
    print('case %d: chi2 %s -> %s in %s iterations (cap %d), field error %.3g, velocity error / vBroad %.3g'
          % (case, r.history[0], r.chi2, r.iterations, cap, np.max(np.abs(r.nodes[:, :o] - truth[:, :o])),
             np.max(np.abs(r.nodes[:, o:] - truth[:, o:])) / vB))
    vc.check_recovery(r, truth, nnode, vB, cap)
    assert r.field.shape == (ncol, 4, Ns) and same(r.field, fithost.expand4(Ns, nnode, basis, None, r.nodes))
    if ncol == 3:           # a column fitted alone takes the same path, bit for bit
        one = drivers.fit_field_columns(e, obs[1:2], mus, basis, start[1:2], nnode, weight=w[1:2], col0=1, ncol=1, **kw)
        assert same(one.nodes[0], r.nodes[1]) and same(one.history[:, 0], r.history[:len(one.history), 1])
    e.close()


# ---- FALC Ca II ------------------------------------------------------------------------------------------------------------------------------
def test_falc_caii_8542_with_a_doppler_shift(hip_lib):
    """the converged fixture, 0.1 T at 45 deg, 30 deg and a uniform 1.5 km/s; mu = 1 and 0.6: the normal equations at the start against
    numpy from Engine.stokes_response, then one constant node per quantity from 0.11 T, 50 deg, 25 deg, 1 km/s.
    The recovered values are printed, not asserted."""
    from test_stokes import FALC_MUS, falc, falc_engine
    prob, block, prof, n, J, (la0, nla), line = falc()
    e, fld = falc_engine(hip_lib)
    pats = [None] * prob.Nlines
    pats[line] = sc.TRIPLET
    Ns, nnode = prob.Nspace, (1, 1, 1, 1)
    basis = np.ones((4, Ns))
    obs = stack(e.stokes_rays(FALC_MUS, *fld, patterns=pats, la0=la0, nla=nla, vlos=1.5e3))
    w = fc.recovery_weight(obs)
    start = np.array([[0.11, np.deg2rad(50.0), np.deg2rad(25.0), 1.0e3]])
    kw = dict(weight=w, patterns=pats, la0=la0, nla=nla)
    ne = e.fit_field_normal(FALC_MUS, basis, nnode, start, obs, **kw)
    rf, S = response4(e, FALC_MUS, ne.field, nnode, pats, None, la0=la0, nla=nla)
    val, bar = fc.yardstick(nnode, rf, S, obs, w, basis)
    x = fc.inside(dict(chi2=ne.chi2, grad=ne.grad, hess=ne.hess), val, bar)
    print('FALC Ca II 854.2 nm, %d wavelengths, %d depths: deviation / bar %s, |grad| / bar %.3g' % (nla, Ns, x, fc.grad_signal(val, bar)))
    assert max(x.values()) <= 1.0 and fc.grad_signal(val, bar) >= fc.SIGNAL
    assert same(e.fit_field_chi2(FALC_MUS, basis, nnode, start, obs, **kw)[0], ne.chi2)
    r = drivers.fit_field_columns(e, obs, FALC_MUS, basis, start, nnode, **kw)
    print('FALC fit: chi2 %.6e -> %.6e, %d iterations, status %d, B %.9f T, gammaB %.7f deg, chiB %.7f deg, vlos %.6f m/s, lambda %.1e'
          % (r.history[0, 0], r.chi2[0], r.iterations[0], r.status[0], r.nodes[0, 0], *np.rad2deg(r.nodes[0, 1:3]), r.nodes[0, 3], r.lam[0]))
    assert np.all(np.diff(r.history[:, 0]) <= 0) and r.chi2[0] <= 1e-6 * r.history[0, 0]
    e.close()


# ---- through Context -----------------------------------------------------------------------------------------------------------------------
def test_context_takes_the_velocity(hip_lib):
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
    pats = [zeeman.zeeman_components(t.transModel) for t in trans if t.isLine]
    la0, nla = int(trans[kr].Nblue), int(trans[kr].wavelength.shape[0])
    B = np.full(Ns, 0.1)
    st = ctx.compute_stokes(mus, B, 0.7, 0.5, transition=trans[kr], vlos=1.5e3)
    ref = ctx._engine.stokes_rays(np.array(mus), B, 0.7, 0.5, patterns=pats, la0=la0, nla=nla, vlos=np.full(Ns, 1.5e3))
    assert same(st.V, ref.V[0]) and same(st.I, ref.I[0])
    assert not same(st.I, ctx.compute_stokes(mus, B, 0.7, 0.5, transition=trans[kr]).I)
    inst = fit.Instrument.identity(nla)
    assert same(ctx.compute_stokes(mus, B, 0.7, 0.5, transition=trans[kr], vlos=1.5e3, instrument=inst).I, st.I)
    rr = ctx.compute_stokes_response(1.0, B, 0.7, 0.5, transition=kr, parameters=('B', 'vlos'), ks=[10, 40], vlos=np.full(Ns, 1.5e3))
    assert set(rr.rf) == {'B', 'vlos'} and rr.rf['vlos'].shape == (4, nla, 2) and rr.amplitudes['vlos'] == 100.0
    r0 = ctx.compute_stokes_response(1.0, B, 0.7, 0.5, transition=kr, parameters='vlos', ks=[10, 40])       # the atmosphere's own vlos
    e0 = ctx._engine.stokes_response(np.array([1.0]), B, 0.7, 0.5, patterns=pats, la0=la0, nla=nla, parameters='vlos', ks=[10, 40],
                                     vlos=np.asarray(atmos.vlos, dtype=np.float64))
    assert same(r0.rf['vlos'], e0.rf['vlos'][0, ..., 0])
    obs = np.stack([st.I, st.Q, st.U, st.V])
    w = 1.0 / (1e-3 * obs[0].max()) ** 2
    hats = fit.hat_basis(np.arange(Ns), [0.0, Ns - 1.0])
    start = np.array([0.105, 0.105, 0.75, 0.45, 1.0e3])
    r = ctx.fit_field(mus, obs, transition=trans[kr], basis={'B': hats, 'gammaB': np.ones(Ns), 'chiB': np.ones(Ns), 'vlos': np.ones(Ns)},
                      start=start, weight=w, max_iter=4)
    basis, nnode = fit.stack_basis(B=hats, gammaB=np.ones(Ns), chiB=np.ones(Ns), vlos=np.ones(Ns))
    base = np.zeros((1, 4, Ns))
    base[0, 3] = np.asarray(atmos.vlos, dtype=np.float64)
    want = drivers.fit_field_columns(ctx._engine, obs[None], np.array(mus), basis, start[None], nnode, weight=np.full((1,) + obs.shape, w),
                                     base=base, patterns=pats, la0=la0, nla=nla, max_iter=4)
    assert r.nnode == (2, 1, 1, 1) and r.nodes.shape == (5,) and r.field.shape == (4, Ns) and r.history.ndim == 1
    assert same(r.nodes, want.nodes[0]) and same(r.history, want.history[:, 0]) and same(r.field, want.field[0])
    assert r.history[-1] < r.history[0] and np.array_equal(r.parameter('vlos'), r.nodes[4:])
    assert np.array_equal(ctx.I, I0) and np.array_equal(ctx.J, J0) and all(np.array_equal(a.n, b) for a, b in zip(ctx.activeAtoms, n0))
    ctx.close()
