"""Response functions of the Stokes spectrum to the field vector without a GPU (include/lsx_hip_stokes_response.h):
lsx_stokes_host_response (liblsx_stokes_host.so: the two stages of lsx_stokes_response.hip through the functions of lsx_stokes_dev.h)
against brute force through the pinned lsx_stokes_host_window, the field changed at one depth.  Bar per entry
(tests/stokes_response_cases.py): (bar(S+) + bar(S-)) / a with the Stokes bar of stokes_cases.bars from host runs of the two changed
fields; in every case and for every parameter the largest brute-force response is at least 1000 x the largest bar."""
import os
import re
import subprocess

import numpy as np
import pytest

import stokes_cases as sc
import stokes_response_cases as rc
from conftest import ROOT, golden
from lightspinner_amd import _capi

CSRC = sc.CSRC
ENTRIES = {'lsx_hip_response_stokes', 'lsx_hip_response_stokes_work_cap'}
MUS = (1.0, 0.6, 0.1)
LA0, NLA = 52, 44                 # the three lines of stokes_cases.problem with their wings
same = lambda a, b: np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.fixture(scope='module')
def host():
    return rc.HostLib()


def _col(Ns, pats='blend', vlos=True, lower_zero=False, kind='inclined', la0=LA0, nla=NLA):
    prob, block, prof, J = sc.problem(Ns, 1, vlos=vlos)
    return sc.column(prob, block, prof, block.n, J, sc.field(Ns, 1, kind), sc.PATTERN_SETS[pats], 0, la0, nla, lower_zero)


_made = {}


def made(host, Ns, pats, vlos, lower_zero, mu):
    """column, the library's (rf, stokes) and brute force's (rf, bar) at all depths for all three parameters, made once"""
    key = (Ns, pats, vlos, lower_zero, mu)
    if key not in _made:
        col = _col(Ns, pats, vlos, lower_zero)
        _made[key] = (col, host.response(col, mu), rc.brute(host, col, mu))
    return _made[key]


# ---- 1. brute force on every depth ---------------------------------------------------------------------------------------------------
# 3 and 4 depths put every depth into the start-value and the end-point sets at once, 5 and 6 part the sets, 13 and 40 have depths in
# neither (the transfer matrix); patterns of 3 ('triplet'), 6 + 3 ('blend'), 27 ('largest') and 6 + 27 + 3 ('all') components
CASES = [(3, 'triplet', False, False), (3, 'all', True, True), (4, 'blend', True, False), (4, 'largest', False, True),
         (5, 'all', True, False), (5, 'triplet', False, True), (6, 'largest', False, False), (6, 'blend', True, True),
         (13, 'all', True, False), (13, 'triplet', False, True), (40, 'blend', True, False), (40, 'triplet', False, True)]


@pytest.mark.parametrize('Ns,pats,vlos,lower_zero', CASES)
def test_brute_force_on_every_depth(host, Ns, pats, vlos, lower_zero):
    """Measured (largest deviation / bar over the twelve cases, three angles, all depths): printed per case; the worst is in
    DESIGN.md 2"""
    for mu in MUS:
        col, (rf, S), (ref, bar) = made(host, Ns, pats, vlos, lower_zero, mu)
        assert same(S, host.window(col, mu))                    # the stokes output has the window call's bits
        for p in rc.PARAMS:
            sig, x = rc.signal(ref[p], bar[p]), rc.ratio(rf[p], ref[p], bar[p])
            print('Ns %d %s vlos %s zero %s mu %.1f %s: deviation / bar %.3g, largest response / largest bar %.3g' % (Ns, pats, vlos, lower_zero, mu, p, x, sig))
            assert sig >= rc.SIGNAL, (mu, p, sig)
            assert x <= 1.0, (mu, p, x)


# ---- 2. the special depths apart -----------------------------------------------------------------------------------------------------
def _nodes(host, col, q, mu, field=None):
    """[Ns][11] eta, rho, eps of wavelength q at every depth (lsx_stokes_host_K), the field from `field` or the column"""
    B, g, x = (col.B, col.gammaB, col.chiB) if field is None else field
    Ns = col.z.shape[0]
    K = np.empty((Ns, 11))
    for k in range(Ns):
        act = col.active[:, q].astype(bool)
        v = (col.wav[q] - col.lambda0) * sc.CLIGHT / (col.vB[:, k] * col.lambda0) + 1.0 * (mu * col.vlos[k] / col.vB[:, k])
        vZ = sc.LARMOR * (1e-9 * col.lambda0) * B[k] / col.vB[:, k]
        K[k] = host.K(col.chi_c[q, k], col.eta_c[q, k], col.nd[:, k] * act, col.ne[:, k] * act, col.aD[:, k], v, vZ,
                      1.0 / (np.sqrt(np.pi) * col.vB[:, k]), col.patterns, g[k], x[k], mu)
    return K


def _delo_walk(z, K, mu, Be, Bn, start_from=None, end_dt_from=None):
    """The DELO-linear walk of lsx_stokes_dev.h restated in numpy for one ray through K [Ns][11] (thermalised lower end).
    start_from / end_dt_from: other K arrays whose eta_I the start value resp. the end point's previous interval are formed from
    -- a response 'built from the two neighbouring steps alone' leaves those two at the unchanged column's"""
    Ns = len(z)
    Ks = K if start_from is None else start_from
    Ke = K if end_dt_from is None else end_dt_from
    node = lambda a: (a[0], a[1:4] / a[0], a[4:7] / a[0], a[7:11] / a[0])
    eIu, eu, ru, Su = node(K[-1])
    S = np.zeros(4)
    S[0] = Be - (Bn - Be) / ((Ks[-1, 0] + Ks[-2, 0]) * 0.5 * abs(z[-1] - z[-2]) / mu)
    Kp = lambda e, r: np.array([[0, e[0], e[1], e[2]], [e[0], 0, r[2], -r[1]], [e[1], -r[2], 0, r[0]], [e[2], r[1], -r[0], 0]])
    for k in range(Ns - 2, -1, -1):
        eI, e, r, Sn = node(K[k])
        dtau = 0.5 * (eIu + eI) * abs(z[k + 1] - z[k]) / mu
        w0, w1 = sc._w2(dtau, 0)
        E, G = 1.0 - w0, w1 / dtau
        Fa = w0 - G
        new = np.linalg.solve(np.eye(4) + Fa * Kp(e, r), E * S - G * (Kp(eu, ru) @ S) + Fa * Sn + G * Su)
        if k == 0:
            w0p, w1p = sc._w2(0.5 * (Ke[2, 0] + Ke[1, 0]) * abs(z[2] - z[1]) / mu, 0)
            new[0] += S[0] * (w0 - w0p) + (w0p * Su[0] - w0 * Sn[0]) + (w1p - w1) * (Su[0] - Sn[0]) / dtau
        S, eIu, eu, ru, Su = new, eI, e, r, Sn
    return S


def test_the_special_depths_apart(host):
    """40 depths, thermalised, mu = 1: the depths Ns - 1, Ns - 2, 2, 1, 0 by name.  A response built from the two neighbouring steps
    alone (the walk restated in numpy above, the start value and the end point's previous interval left at the unchanged column's)
    is outside the bar at depth 2 (the end point reads dtau(2, 1)) and at depth Ns - 2 (the start value reads its eta_I); the
    library is inside at all five, and so is the numpy walk with nothing left out: the restatement is right and the test sees the
    trap.  The wavelengths are the window's most transparent ones: the lowest depths show at the surface there"""
    Ns, mu, name = 40, 1.0, 'B'
    col, (rf, S), (ref, bar) = made(host, Ns, 'blend', True, False, mu)
    a = rc.AMPS[name]
    Be, Bn = sc.planck(col.T[-1], col.wav), sc.planck(col.T[-2], col.wav)
    depths = [Ns - 1, Ns - 2, 2, 1, 0]
    for j in depths:
        assert rc.ratio(rf[name][..., j], ref[name][..., j], bar[name][..., j]) <= 1.0, j
    naive_out, full_in = {j: 0.0 for j in depths + [20]}, {j: 0.0 for j in depths + [20]}
    for q in (0, NLA - 1, NLA // 2):
        base = _nodes(host, col, q, mu)
        for j in depths + [20]:
            Kpm = []
            for sg in (1, -1):
                B = np.array(col.B)
                B[j] = B[j] + 0.5 * a if sg > 0 else B[j] - 0.5 * a
                K = base.copy()
                K[j] = _nodes(host, col.replace(z=col.z[j:j + 1], B=B[j:j + 1], gammaB=col.gammaB[j:j + 1], chiB=col.chiB[j:j + 1],
                                                vlos=col.vlos[j:j + 1], chi_c=col.chi_c[:, j:j + 1], eta_c=col.eta_c[:, j:j + 1],
                                                nd=col.nd[:, j:j + 1], ne=col.ne[:, j:j + 1], aD=col.aD[:, j:j + 1], vB=col.vB[:, j:j + 1]),
                              q, mu)[0]
                Kpm.append(K)
            full = (_delo_walk(col.z, Kpm[0], mu, Be[q], Bn[q]) - _delo_walk(col.z, Kpm[1], mu, Be[q], Bn[q])) / a
            naive = (_delo_walk(col.z, Kpm[0], mu, Be[q], Bn[q], base, base) - _delo_walk(col.z, Kpm[1], mu, Be[q], Bn[q], base, base)) / a
            b = bar[name][:, q, j]
            full_in[j] = max(full_in[j], float(np.max(np.abs(full - ref[name][:, q, j]) / b)))
            naive_out[j] = max(naive_out[j], float(np.max(np.abs(naive - ref[name][:, q, j]) / b)))
    print('two steps alone, deviation / bar by depth:', naive_out, '; the whole walk in numpy:', full_in)
    assert all(v <= 1.0 for v in full_in.values()), full_in
    assert naive_out[20] <= 1.0 and naive_out[2] > 1.0 and naive_out[Ns - 2] > 1.0, naive_out


# ---- 3. properties ---------------------------------------------------------------------------------------------------------------------
def test_no_pattern_and_no_field_give_zeros(host):
    """With no pattern every response is 0.0 exactly.  With B = 0 everywhere and only the two angles requested the responses of
    Q, U, V are 0.0 exactly (the split profiles' differences are: lsx_stokes_dev.h, line_profiles) and that of I is zero inside the
    bar, not exactly: a polarised line's eta_I goes through the geometry, phi (s^2 + 1 + c^2) / 2, and s^2 + c^2 is 1 only to
    rounding (lsx_stokes_dev.h, line_add_plain's remark), in the pinned pass and so in its brute force as well"""
    for mu in MUS:
        rf, S = host.response(_col(13, 'none'), mu)
        assert all(np.all(v == 0.0) for v in rf.values()) and np.all(S[1:] == 0.0) and np.all(S[0] != 0.0)
        col = _col(13, 'all', kind='zero')
        names = ('gammaB', 'chiB')
        rf, S = host.response(col, mu, parameters=names)
        ref, bar = rc.brute(host, col, mu, parameters=names)
        assert sorted(rf) == ['chiB', 'gammaB']
        for p in names:
            assert np.all(rf[p][1:] == 0.0) and np.all(ref[p][1:] == 0.0)
            assert np.all(np.abs(rf[p][0]) <= bar[p][0]) and rc.ratio(rf[p], ref[p], bar[p]) <= 1.0


def test_the_azimuth_at_disc_centre(host):
    """mu = 1: moving the azimuth at ALL depths by d turns (Q, U) by 2 d and leaves I and V alone.  So, summed over all depths, the
    response to chiB is (0, -2 U, 2 Q, 0) up to the difference quotient's own second-order term, which is stated from runs at a
    and a / 2: t = 4 / 3 (sum(a) - sum(a / 2)).  Bar of the sum: the depths' bars added; the library is within a bar of brute
    force and brute force within a bar of the truth: twice that, for the a-run and for t; and the bar of (U, Q) themselves.
    (At ONE depth the response of I and V to chiB is not zero, with a uniform azimuth either: rho_V turns the plane of polarisation
    between the depths, so the column with one depth turned by +a/2 is no mirror image of the one with -a/2.  The figures are
    printed: the sum over the depths is what vanishes.)"""
    col, (rf, S), (ref, bar) = made(host, 13, 'all', True, False, 1.0)
    a = rc.AMPS['chiB']
    half = {'chiB': 0.5 * a}
    rf2, _ = host.response(col, 1.0, parameters=('chiB',), amplitudes=half)
    _, bar2 = rc.brute(host, col, 1.0, parameters=('chiB',), amplitudes=half)
    sum_a, sum_h = rf['chiB'].sum(axis=-1), rf2['chiB'].sum(axis=-1)
    t = 4.0 / 3.0 * (sum_a - sum_h)
    runs = {u: host.window(col, 1.0, ulp=u)[None, :, :, None] for u in (0, 1, -1)}
    sbar = sc.bars(runs)[0, :, :, 0]
    allowed = 2.0 * (bar['chiB'].sum(axis=-1) + 4.0 / 3.0 * (bar['chiB'].sum(axis=-1) + bar2['chiB'].sum(axis=-1))) + 2.0 * sbar
    want = np.stack([np.zeros_like(S[0]), -2.0 * S[2], 2.0 * S[1], np.zeros_like(S[0])])
    dev = np.abs(sum_a - t - want)
    one = np.max(np.abs(rf['chiB'][[0, 3]]), axis=-1)
    print('azimuth: sum over depths against (0, -2U, 2Q, 0): largest deviation / allowed %.3g; second-order term / allowed %.3g; '
          '(Q, U) / allowed %.3g; largest response of I, V at one depth / allowed %.3g, / I %.3g'
          % (np.max(dev / allowed), np.max(np.abs(t) / allowed), np.max(np.abs(want[1:3]) / allowed[1:3]), np.max(one / allowed[[0, 3]]),
             np.max(one / np.abs(S[0]))))
    assert np.all(dev <= allowed)
    assert np.max(np.abs(want[1:3]) / allowed[1:3]) >= rc.SIGNAL and np.max(one / allowed[[0, 3]]) >= rc.SIGNAL


def test_subsets_of_depths_and_parameters_give_the_full_calls_bits(host):
    for Ns, mu in ((5, 0.6), (40, 0.1)):
        col, (rf, S), _ = made(host, Ns, 'all' if Ns == 5 else 'blend', True, False, mu)
        for ks in ([0], [Ns - 1], [1, 2], [Ns - 2], [0, 2, Ns - 1], [Ns // 2], list(range(1, Ns, 2))):
            sub, S2 = host.response(col, mu, ks=ks)
            assert same(S2, S)
            for p in rc.PARAMS:
                assert same(sub[p], rf[p][..., ks]), (Ns, ks, p)
        for names in (('B',), ('gammaB',), ('chiB',), ('B', 'chiB'), ('chiB', 'gammaB')):
            sub, _ = host.response(col, mu, parameters=names, ks=[0, Ns - 2])
            assert sorted(sub) == sorted(names)
            for p in names:
                assert same(sub[p], rf[p][..., [0, Ns - 2]]), (Ns, names, p)


# ---- 4. the rules ------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_with_its_code(host):
    col = _col(5, 'all')
    code = lambda c=col, **kw: host.response_rc(c, 0.6, **kw)[0]
    OK, EINVAL, EUNS = sc.LSX_OK, sc.LSX_EINVAL, sc.LSX_EUNSUPPORTED
    assert code() == OK and code(want_stokes=False) == OK
    assert code(params_bits=0) == EINVAL and code(params_bits=8) == EINVAL and code(params_bits=9) == EINVAL
    for i, p in enumerate(rc.PARAMS):
        for bad in (0.0, -1e-3, np.nan, np.inf, -np.inf):
            amp = [0.01, 0.01, 0.01]
            amp[i] = bad
            assert code(parameters=(p,), amp_array=amp) == EINVAL, (p, bad)
            assert code(parameters=[w for w in rc.PARAMS if w != p], amp_array=amp) == OK, (p, bad)       # not requested: not read
    for bad in ([-1], [5], [1, 1], [2, 1], [0, 1, 2, 3, 4, 4]):
        assert code(ks=bad) == EINVAL, bad
    assert code(ks=[0], nk=0) == EINVAL
    gaps = _col(5, 'all', kind='gaps')                                            # B = 0 at depths 1 and 4
    assert code(gaps) == EINVAL and code(gaps, ks=[0, 2, 3]) == OK and code(gaps, parameters=('gammaB', 'chiB')) == OK
    assert code(gaps, ks=[0, 1], parameters=('B',)) == EINVAL
    edge = col.replace(B=np.full(5, 0.5 * rc.AMPS['B']))
    assert code(edge) == OK and code(col.replace(B=np.full(5, np.nextafter(0.5 * rc.AMPS['B'], 0.0)))) == EINVAL
    # what the Stokes pass refuses, with its codes
    for w in ('B', 'gammaB', 'chiB'):
        bad = np.array(getattr(col, w))
        bad[2] = np.nan
        assert code(col.replace(**{w: bad})) == EINVAL
    assert code(col.replace(B=-col.B), parameters=('chiB',)) == EINVAL
    assert code(col.replace(patterns=[([-1, 0, 2], [1, 1, 1], [0, 0, 0]), None, None])) == EINVAL
    over = (np.r_[sc.LARGEST.alpha, np.zeros(38, dtype=np.int32)], np.r_[sc.LARGEST.strength, np.zeros(38)], np.r_[sc.LARGEST.shift, np.zeros(38)])
    assert code(col.replace(patterns=[over, None, None])) == EUNS
    assert host.response_rc(col, 0.0)[0] == EINVAL and host.response_rc(col, 1.0 + 1e-12)[0] == EINVAL


# ---- 5. the entry's hygiene ----------------------------------------------------------------------------------------------------------
def test_the_entries_are_exported_declared_in_a_header_of_their_own_and_bound():
    lib = os.path.join(CSRC, 'liblsx_hip.so')
    assert os.path.exists(lib), 'build the HIP library first (make -C lightspinner_amd/csrc)'
    syms = subprocess.run(['nm', '-D', '--defined-only', lib], capture_output=True, text=True, check=True).stdout
    text = open(os.path.join(ROOT, 'include', 'lsx_hip_stokes_response.h')).read()
    assert set(re.findall(r'\b(lsx_hip_[a-z0-9_]+)\s*\(', text)) == ENTRIES
    assert set(re.findall(r'\bT (lsx_hip_response_stokes[a-z0-9_]*)\b', syms)) == ENTRIES
    assert '#include "lsx_hip_stokes_response.h"' in open(os.path.join(ROOT, 'include', 'lsx_hip.h')).read()
    assert not any(s.startswith('lsx_hip_stokes') for s in _capi.REQUIRED_SYMBOLS)        # the common ABI is what it was
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    assert 'lsx_hip_stokes_response.h' in re.search(r'^BUILD_SRCS := (.*)$', mk, re.M).group(1)
    host = subprocess.run(['nm', '-D', '--defined-only', os.path.join(CSRC, 'liblsx_stokes_host.so')], capture_output=True, text=True, check=True).stdout
    assert re.search(r'\bT lsx_stokes_host_response\b', host) and re.search(r'\bT lsx_stokes_host_window\b', host)
    hip = _capi.load_hip_library()
    assert hip.has_stokes_response and hip.dll.lsx_hip_response_stokes.restype is not None
    from lightspinner_amd.problem import StokesResponse
    assert StokesResponse.DEFAULT_AMPLITUDES == {'B': 1e-3, 'gammaB': 1e-3, 'chiB': 1e-3}


@pytest.mark.parametrize('compiler,std', [('gcc', 'c99'), ('g++', 'c++11')])
def test_the_header_compiles_alone(compiler, std):
    lang = 'c' if compiler == 'gcc' else 'c++'
    r = subprocess.run([compiler, '-std=' + std, '-Wall', '-Wextra', '-pedantic', '-Werror', '-fsyntax-only', '-x', lang,
                        os.path.join(ROOT, 'include', 'lsx_hip_stokes_response.h')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_oracle_has_no_such_entry_and_the_engine_says_so(oracle_lib):
    from lightspinner_amd import fixtures
    from lightspinner_amd.problem import Engine
    prob, block, raw = fixtures.load_problem_npz(golden('falc_ca.npz'))
    e = Engine(prob, 1, lib=oracle_lib)
    e.set_columns(0, block)
    assert not oracle_lib.has_stokes_response
    with pytest.raises(NotImplementedError, match='lsx_hip_response_stokes'):
        e.stokes_response([1.0], 0.1, 0.5, 0.5)
    e.close()


def test_the_kernels_use_no_scratch_and_spill_no_vector_register():
    """build/lsx_stokes_response.ru.log, the compiler's resource report of the unit: both kernels without scratch, without a spilled
    vector register and without a dynamic stack; and the report belongs to the object beside it"""
    path, obj = (os.path.join(CSRC, 'build', 'lsx_stokes_response' + x) for x in ('.ru.log', '.o'))
    if not (os.path.exists(path) and os.path.exists(obj)):
        subprocess.check_call(['make', '-s', '-j', '8', '-C', CSRC])
    assert os.path.getmtime(path) >= os.path.getmtime(os.path.join(CSRC, 'lsx_stokes_response.hip')) - 1.0
    assert abs(os.path.getmtime(path) - os.path.getmtime(obj)) < 120.0, 'the report is not from the compile that made the object'
    blocks = re.split(r'remark: [^\n]*Function Name: ', open(path).read())[1:]
    names = [b.split()[0] for b in blocks]
    assert len(names) == 2 and any('k_response_nodes' in x for x in names) and any('k_response_walk' in x for x in names), names
    for b, name in zip(blocks, names):
        val = lambda key: int(re.search(re.escape(key) + r':? (\d+)', b).group(1))
        assert val('ScratchSize [bytes/lane]') == 0, name
        assert val('VGPRs Spill') == 0, name
        assert re.search(r'Dynamic Stack: False', b), name


def test_the_host_response_under_asan_ubsan():
    """columns of 3, 4 and 40 depths, subsets of the depths, every set of parameters and every refusal: in a stand-alone program"""
    subprocess.check_call(['make', '-s', '-C', CSRC, 'stokesrespsan'])
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:halt_on_error=1', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')
    out = subprocess.run([os.path.join(CSRC, 'lsx_stokes_response_san')], capture_output=True, text=True, timeout=600, env=env)
    tail = out.stdout[-1500:] + '\n' + out.stderr[-3000:]
    assert out.returncode == 0, tail
    assert 'STOKES RESPONSE SANITIZED RUN COMPLETE' in out.stdout, tail
