"""Response functions of the Stokes spectrum to the field vector on the GPU (include/lsx_hip_stokes_response.h,
lsx_hip_response_stokes) against brute force through the pinned pass, twice: central differences of the host library's
lsx_stokes_host_window, and of the GPU's own Engine.stokes_rays, with the field changed at one depth.  Bar per entry
(tests/stokes_response_cases.py): (bar(S+) + bar(S-)) / a, bar(S) the Stokes bar 1e-11 I_host + 3 x the +-1-ulp-exp envelope of the
host run of that field; in every case the largest brute-force response is at least 1000 x the largest bar.
Measured on an MI355X (worst deviation / bar): 0.042 on the shapes of 3, 4 and 5 depths, 0.019 (host) and 1.6e-4 (GPU brute force) at 40
depths, 1.7e-4 on FALC Ca II 854.2 nm with the response at 3.0e6 to 6.6e7 x the bar."""
import dataclasses

import numpy as np
import pytest

import stokes_cases as sc
import stokes_response_cases as rc
from conftest import golden
from lightspinner_amd import _capi, fixtures, synth
from lightspinner_amd.problem import Engine

pytestmark = pytest.mark.gpu

MUS = np.array([1.0, 0.1, 0.6])
WINDOWS = [(0, 1), (7, 1), (0, 63), (7, 63), (0, 64), (7, 64), (0, 65), (7, 65), (0, 130), (7, 130)]
same = lambda a, b: np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.fixture(scope='module')
def host():
    return rc.HostLib()


def make_engine(hip_lib, prob, block, prof, J):
    e = Engine(prob, block.ncol, lib=hip_lib)
    synth.load_columns(e, block, prof)
    e.set(_capi.LSX_J, J)
    return e


def stack(r):
    return np.stack([r.I, r.Q, r.U, r.V], axis=1)          # [ncol][4][nla][nmu]


def host_brute(host, prob, block, prof, n, J, fld, patterns, mus, la0, nla, parameters, ks, lower_zero=False, cols=None):
    """-> (rf, bar), each {name: [ncol][4][nla][nk][nmu]}; ks: {name: depths}"""
    cols = range(block.ncol) if cols is None else cols
    rf, bar = {p: [] for p in parameters}, {p: [] for p in parameters}
    for c in cols:
        cc = sc.column(prob, block, prof, n, J, fld, patterns, c, la0, nla, lower_zero)
        per = [rc.brute(host, cc, mu, parameters=[p], ks=ks[p]) for mu in mus for p in parameters]
        for i, p in enumerate(parameters):
            rf[p].append(np.stack([per[m * len(parameters) + i][0][p] for m in range(len(mus))], axis=-1))
            bar[p].append(np.stack([per[m * len(parameters) + i][1][p] for m in range(len(mus))], axis=-1))
    return {p: np.stack(v) for p, v in rf.items()}, {p: np.stack(v) for p, v in bar.items()}


def gpu_brute(e, mus, fld, patterns, la0, nla, parameters, ks, amplitudes=rc.AMPS, **kw):
    """-> {name: [ncol][4][nla][nk][nmu]}: central differences of Engine.stokes_rays, the depth changed in every column of the call"""
    out = {}
    for p in parameters:
        i, a, r = rc.PARAMS.index(p), amplitudes[p], []
        for k in ks[p]:
            S = []
            for sg in (1, -1):
                f = [np.array(t) for t in fld]
                f[i][:, k] = f[i][:, k] + 0.5 * a if sg > 0 else f[i][:, k] - 0.5 * a
                S.append(stack(e.stokes_rays(mus, *f, patterns=patterns, la0=la0, nla=nla, **kw)))
            r.append((S[0] - S[1]) / a)
        out[p] = np.stack(r, axis=-2)
    return out


def all_depths(Ns, fld=None):
    """every depth for every parameter; with a field: B only where it is not 0"""
    ks = {p: list(range(Ns)) for p in rc.PARAMS}
    if fld is not None:
        ks['B'] = [k for k in range(Ns) if np.all(fld[0][:, k] > 0)]
    return ks


def response(e, mus, fld, patterns, ks, parameters=rc.PARAMS, **kw):
    """one call per distinct set of depths -> ({name: rf}, the StokesRays of the last call)"""
    rf, r = {}, None
    for p in parameters:
        if p in rf:
            continue
        group = [w for w in parameters if ks[w] == ks[p]]
        r = e.stokes_response(mus, *fld, patterns=patterns, parameters=group, amplitudes=rc.AMPS, ks=ks[p], **kw)
        rf.update(r.rf)
    return rf, r.stokes


SHAPES = [(3, 1, False, False, 'triplet', 'inclined'), (4, 3, True, False, 'all', 'inclined'), (5, 3, True, False, 'all', 'gaps'),
          (5, 1, False, True, 'largest', 'inclined')]


@pytest.mark.parametrize('Ns,ncol,vlos,compact,pats,kind', SHAPES)
def test_against_both_brute_forces_on_every_window(hip_lib, host, Ns, ncol, vlos, compact, pats, kind):
    """3, 4 and 5 depths (every depth is in the start-value or the end-point set, or both; at 5 the sets part), windows of 1, 63, 64,
    65, 130 wavelengths at la0 = 0 and 7, one and three angles down to mu = 0.1, one and three columns with different fields, vlos or
    compact profiles, patterns of 3 and 27 components; 'gaps': depths with B = 0 between depths with a field, left out with ks for B
    and kept for the two angles.  The host's brute force is made once on the whole grid"""
    prob, block, prof, J = sc.problem(Ns, ncol, vlos=vlos, compact=compact)
    fld = sc.field(Ns, ncol, kind)
    patterns = sc.PATTERN_SETS[pats]
    e = make_engine(hip_lib, prob, block, prof, J)
    ks = all_depths(Ns, fld)
    assert kind != 'gaps' or 0 < len(ks['B']) < Ns
    ref, bar = host_brute(host, prob, block, prof, block.n, J, fld, patterns, MUS, 0, prob.Nspect, rc.PARAMS, ks)
    for p in rc.PARAMS:
        assert rc.signal(ref[p], bar[p]) >= rc.SIGNAL, (p, rc.signal(ref[p], bar[p]))
    worst = {p: 0.0 for p in rc.PARAMS}
    for la0, nla in WINDOWS:
        for ms in ([0], [0, 1, 2]):
            rf, S = response(e, MUS[ms], fld, patterns, ks, la0=la0, nla=nla)
            assert same(stack(S), stack(e.stokes_rays(MUS[ms], *fld, patterns=patterns, la0=la0, nla=nla)))
            gb = gpu_brute(e, MUS[ms], fld, patterns, la0, nla, rc.PARAMS, ks) if (la0, nla) in ((7, 65), (0, 1)) else None
            for p in rc.PARAMS:
                sub = lambda a: a[:, :, la0:la0 + nla][..., ms]
                x = rc.ratio(rf[p], sub(ref[p]), sub(bar[p]))
                worst[p] = max(worst[p], x)
                assert x <= 1.0, (p, la0, nla, ms, x)
                if gb is not None:
                    x = rc.ratio(rf[p], gb[p], sub(bar[p]))
                    assert x <= 1.0, ('gpu brute force', p, la0, nla, ms, x)
    print('Ns %d ncol %d %s %s: worst deviation / bar' % (Ns, ncol, pats, kind), worst)
    e.close()


def test_forty_depths(hip_lib, host):
    """40 depths, where the transfer matrix carries most responses: the middle one of three columns with different fields and vlos
    (the host's brute force of one column at 40 depths is what this test's time goes into), a blend of a 6-component and a
    3-component pattern with an unpolarised line, mu = 1 and 0.1; the window [7, 72) (two wavefronts, the second with one lane);
    the other windows, columns and angles hang on this one by the bits (test_bits)"""
    Ns, ncol, la0, nla = 40, 3, 7, 65
    prob, block, prof, J = sc.problem(Ns, ncol, vlos=True)
    fld = sc.field(Ns, ncol)
    patterns = sc.PATTERN_SETS['blend']
    e = make_engine(hip_lib, prob, block, prof, J)
    ks = all_depths(Ns)
    mus = MUS[:2]
    ref, bar = host_brute(host, prob, block, prof, block.n, J, fld, patterns, mus, la0, nla, rc.PARAMS, ks, cols=[1])
    rf, S = response(e, mus, fld, patterns, ks, la0=la0, nla=nla)
    gb = gpu_brute(e, mus, fld, patterns, la0, nla, rc.PARAMS, ks)
    for p in rc.PARAMS:
        assert rc.signal(ref[p], bar[p]) >= rc.SIGNAL
        xh, xg = rc.ratio(rf[p][1:2], ref[p], bar[p]), rc.ratio(rf[p][1:2], gb[p][1:2], bar[p])
        print('40 depths, %s: deviation / bar %.3g (host brute force) %.3g (GPU brute force)' % (p, xh, xg))
        assert xh <= 1.0 and xg <= 1.0
    e.close()


def test_a_zero_lower_boundary(hip_lib, host):
    prob, block, prof, J = sc.problem(5, 1, vlos=True)
    fld = sc.field(5, 1)
    patterns = sc.PATTERN_SETS['blend']
    e = make_engine(hip_lib, prob, block, prof, J)
    e.set_boundary('zero', 'zero')
    ks = all_depths(5)
    ref, bar = host_brute(host, prob, block, prof, block.n, J, fld, patterns, MUS, 0, prob.Nspect, rc.PARAMS, ks, lower_zero=True)
    thermal, _ = host_brute(host, prob, block, prof, block.n, J, fld, patterns, MUS, 0, prob.Nspect, ['B'], ks)
    rf, S = response(e, MUS, fld, patterns, ks)
    gb = gpu_brute(e, MUS, fld, patterns, 0, prob.Nspect, rc.PARAMS, ks)
    for p in rc.PARAMS:
        assert rc.signal(ref[p], bar[p]) >= rc.SIGNAL
        assert rc.ratio(rf[p], ref[p], bar[p]) <= 1.0 and rc.ratio(rf[p], gb[p], bar[p]) <= 1.0
    assert rc.ratio(thermal['B'], ref['B'], bar['B']) > 1.0          # the boundary is seen
    e.close()


# ---- FALC Ca II ------------------------------------------------------------------------------------------------------------------------
def test_falc_caii_8542(hip_lib, host):
    """one column from the committed fixture's converged n and J, the window of the 854.2 nm line, 0.1 T at gamma = 45 deg,
    chi = 30 deg, mu = 1 and 0.6, every depth, against the GPU's brute force inside the bar of the host runs"""
    from test_stokes import FALC_MUS, falc, falc_engine
    prob, block, prof, n, J, (la0, nla), line = falc()
    e, fld = falc_engine(hip_lib)
    pats = [None] * prob.Nlines
    pats[line] = sc.TRIPLET
    Ns = prob.Nspace
    ks = all_depths(Ns)
    amps = {'B': 0.01, 'gammaB': 0.01, 'chiB': 0.01}
    r = e.stokes_response(FALC_MUS, *fld, patterns=pats, la0=la0, nla=nla, amplitudes=amps)
    gb = gpu_brute(e, FALC_MUS, fld, pats, la0, nla, rc.PARAMS, ks, amplitudes=amps)
    blk = dataclasses.replace(block, phi=None, wphi=None)
    for p in rc.PARAMS:
        bar = []
        for m, mu in enumerate(FALC_MUS):
            cc = sc.column(prob, blk, prof, n, J, fld, pats, 0, la0, nla)
            bar.append(rc.brute(host, cc, mu, parameters=[p], amplitudes=amps)[1][p])
        bar = np.stack(bar, axis=-1)[None]
        sig, x = rc.signal(gb[p], bar), rc.ratio(r.rf[p], gb[p], bar)
        print('FALC Ca II 854.2 nm, %d wavelengths, %d depths, %s: deviation / bar %.3g, signal / bar %.3g' % (nla, Ns, p, x, sig))
        assert sig >= rc.SIGNAL and x <= 1.0
    assert same(stack(r.stokes), stack(e.stokes_rays(FALC_MUS, *fld, patterns=pats, la0=la0, nla=nla)))
    e.close()


# ---- bit invariance ------------------------------------------------------------------------------------------------------------------
def test_bits(hip_lib):
    """stokes is Engine.stokes_rays; rf does not depend on the column range, on one column per pass under a small work cap, on the
    window's cut, on the other angles, depths or parameters of the call"""
    Ns, ncol = 40, 3
    prob, block, prof, J = sc.problem(Ns, ncol, vlos=True)
    fld = sc.field(Ns, ncol)
    pats = sc.PATTERN_SETS['blend']
    e = make_engine(hip_lib, prob, block, prof, J)
    call = lambda mus=MUS, f=fld, **kw: e.stokes_response(mus, *f, patterns=pats, amplitudes=rc.AMPS, **kw)
    whole = call()
    W = rc.stack_rf(whole)
    assert same(stack(whole.stokes), stack(e.stokes_rays(MUS, *fld, patterns=pats)))
    for c in range(3):
        assert same(rc.stack_rf(call(f=[t[c:c + 1] for t in fld], col0=c, ncol=1))[0], W[c]), c
    assert same(rc.stack_rf(call(f=[t[1:3] for t in fld], col0=1, ncol=2)), W[1:3])
    nlaP = 64 * ((prob.Nspect + 63) // 64)
    one = 8 * (3 * 7 * Ns * 11 * nlaP + 3 * Ns * 5 * nlaP + 3 * 4 * prob.Nspect * Ns * 3 + 3 * Ns) + 64
    assert same(rc.stack_rf(call(work_cap_bytes=one)), W)                 # one column a pass
    assert same(rc.stack_rf(call(work_cap_bytes=1)), W)                   # below one column's need: one column a pass too
    call(work_cap_bytes=0)
    a, b = call(la0=0, nla=71), call(la0=71)
    assert same(np.concatenate([rc.stack_rf(a), rc.stack_rf(b)], axis=3), W)
    for ms in ([1], [2, 0]):
        assert same(rc.stack_rf(call(mus=MUS[ms])), W[..., ms])
    sub = [0, 1, 2, 3, 17, 37, 38, 39]
    assert same(rc.stack_rf(call(ks=sub)), W[..., sub, :])
    assert same(rc.stack_rf(call(ks=[5])), W[..., [5], :])
    for i, p in enumerate(rc.PARAMS):
        assert same(rc.stack_rf(call(parameters=[p])), W[:, i:i + 1])
    assert same(rc.stack_rf(call(parameters=['chiB', 'B'])), W[:, [0, 2]])
    e.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(hip_lib):
    prob, block, prof, J = sc.problem(5, 3, vlos=True)
    fld = sc.field(5, 3)
    gaps = sc.field(5, 3, 'gaps')
    patterns = sc.PATTERN_SETS['all']
    e = make_engine(hip_lib, prob, block, prof, J)
    e.formal_sol_gamma()
    before = [e.get(w).copy() for w in (_capi.LSX_I, _capi.LSX_J, _capi.LSX_N)]
    S0 = stack(e.stokes_rays(MUS, *fld, patterns=patterns))

    def refused(code, mus=MUS, f=fld, pats=patterns, word=None, **kw):
        with pytest.raises(_capi.LsxError) as ei:
            e.stokes_response(mus, *f, patterns=pats, **kw)
        assert ei.value.code == code, (ei.value.code, str(ei.value))
        assert word is None or word in str(ei.value), str(ei.value)

    EINVAL, EUNS = sc.LSX_EINVAL, sc.LSX_EUNSUPPORTED
    # what stokes_rays refuses, with its codes
    for k in range(3):
        for bad in (np.nan, np.inf):
            f = [a.copy() for a in fld]
            f[k][1, 2] = bad
            refused(EINVAL, f=f)
    f = [a.copy() for a in fld]
    f[0][2, 0] = -1e-9
    refused(EINVAL, f=f)
    refused(EINVAL, pats=[([-1, 0, 2], [1, 1, 1], [0, 0, 0]), None, None])
    refused(EINVAL, pats=[([-1, 0, 1], [1, 1, 1 + 1e-11], [0, 0, 0]), None, None])
    refused(EINVAL, la0=-1, nla=3)
    refused(EINVAL, la0=prob.Nspect - 2, nla=3)
    refused(EINVAL, nla=0)
    refused(EINVAL, col0=2, ncol=2, f=[a[:2] for a in fld])
    refused(EINVAL, ncol=0, f=[a[:0] for a in fld])
    for bad in ([0.0], [1.0 + 1e-12], [np.nan], [-0.5]):
        refused(EINVAL, mus=np.array(bad))
    over = (np.r_[sc.LARGEST.alpha, np.zeros(38, dtype=np.int32)], np.r_[sc.LARGEST.strength, np.zeros(38)], np.r_[sc.LARGEST.shift, np.zeros(38)])
    refused(EUNS, pats=[over, None, None])
    # its own
    refused(EINVAL, parameters=[])
    for p in rc.PARAMS:
        for bad in (0.0, -1e-3, np.nan, np.inf):
            refused(EINVAL, parameters=[p], amplitudes={p: bad}, word=p)
    e.stokes_response(MUS[:1], *fld, patterns=patterns, parameters=['gammaB'], amplitudes={'B': np.nan}, nla=3)     # not requested: not read
    for bad in ([], [-1], [5], [1, 1], [2, 1], [0, 1, 2, 3, 4, 5]):
        refused(EINVAL, ks=bad)
    refused(EINVAL, f=gaps, word='column 0, depth 1')                        # B = 0 at depth 1 of every column
    refused(EINVAL, f=gaps, ks=[0, 2, 4], amplitudes={'B': 1.0}, word='depth 0')
    e.stokes_response(MUS[:1], *gaps, patterns=patterns, ks=[0, 2, 3], nla=3)
    e.stokes_response(MUS[:1], *gaps, patterns=patterns, parameters=['gammaB', 'chiB'], nla=3)
    dll, h = e.lib.dll, e._h
    import ctypes as C
    from lightspinner_amd import zeeman
    nc, al, st, sh = zeeman.pack(patterns, prob.Nlines)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    mu, amp = np.array([1.0]), np.full(3, 1e-3)
    rf, S = np.empty((3, 3, 4, prob.Nspect, 5, 1)), np.empty((3, 4, prob.Nspect, 1))

    def raw(bits=7, rfb=rf.nbytes, sb=S.nbytes, amps=dp(amp)):
        return dll.lsx_hip_response_stokes(h, 1, dp(mu), 0, 3, 0, prob.Nspect, dp(fld[0]), dp(fld[1]), dp(fld[2]), ip(nc), ip(al), dp(st),
                                           dp(sh), bits, amps, 5, None, dp(rf), rfb, dp(S), sb)

    assert raw() == sc.LSX_OK
    assert raw(bits=0) == EINVAL and raw(bits=8) == EINVAL and raw(bits=15) == EINVAL
    assert raw(rfb=rf.nbytes - 8) == EINVAL and raw(sb=S.nbytes + 8) == EINVAL and raw(amps=None) == EINVAL
    assert raw(bits=3, rfb=rf.nbytes) == EINVAL and raw(bits=3, rfb=rf.nbytes // 3 * 2) == sc.LSX_OK
    for w, b in zip((_capi.LSX_I, _capi.LSX_J, _capi.LSX_N), before):
        assert np.array_equal(e.get(w), b)
    assert same(stack(e.stokes_rays(MUS, *fld, patterns=patterns)), S0)
    # a GIVEN lower boundary; profiles handed over as arrays
    e.set_boundary('given', 'zero', I_lower=np.ones((3, prob.Nspect, prob.Nrays)))
    refused(EUNS)
    e.close()
    p2, b2 = sc.toy.toy_problem(Nspace=5, ncol=1)
    e2 = Engine(p2, 1, lib=hip_lib)
    e2.set_columns(0, b2)
    with pytest.raises(_capi.LsxError) as ei:
        e2.stokes_response([1.0], *sc.field(5, 1), patterns=None)
    assert ei.value.code == EUNS and 'handed over as arrays' in str(ei.value)
    e2.close()


# ---- through Context -----------------------------------------------------------------------------------------------------------------
def test_compute_stokes_response_is_the_engine_call(hip_lib):
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
    B, g, x = np.full(Ns, 0.1), np.full(Ns, 0.7), 0.5
    ks = [0, 10, 40, Ns - 1]
    r = ctx.compute_stokes_response([1.0, 0.6], B, g, x, transition=trans[kr], ks=ks, parameters=['B', 'chiB'])
    pats = [zeeman.zeeman_components(t.transModel) for t in trans if t.isLine]
    la0, nla = int(trans[kr].Nblue), int(trans[kr].wavelength.shape[0])
    ref = ctx._engine.stokes_response([1.0, 0.6], B, g, x, patterns=pats, la0=la0, nla=nla, ks=ks, parameters=['B', 'chiB'])
    assert sorted(r.rf) == ['B', 'chiB'] and r.amplitudes == {'B': 1e-3, 'chiB': 1e-3} and list(r.ks) == ks and r.la0 == la0
    for p in r.rf:
        assert r.rf[p].shape == (4, nla, 4, 2) and np.array_equal(r.rf[p], ref.rf[p][0])
    st = ctx.compute_stokes([1.0, 0.6], B, g, x, transition=trans[kr])
    for w in 'IQUV':
        assert np.array_equal(getattr(r.stokes, w), getattr(st, w))
    assert np.max(np.abs(r.rf['B'][3])) > 0
    one = ctx.compute_stokes_response(0.6, B, g, x, transition=kr, ks=ks, parameters='B')
    assert one.rf['B'].shape == (4, nla, 4) and np.array_equal(one.rf['B'], r.rf['B'][..., 1]) and one.stokes.I.shape == (nla,)
    assert np.array_equal(ctx.I, I0) and np.array_equal(ctx.J, J0) and all(np.array_equal(a.n, b) for a, b in zip(ctx.activeAtoms, n0))
    ctx.close()
