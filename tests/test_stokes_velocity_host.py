"""The line-of-sight velocity as a quantity of the call, without a GPU (include/lsx_hip_stokes_velocity.h): the host twins
lsx_stokes_host_response_v (liblsx_stokes_host.so) and lsx_fit_host_expand4 / lsx_fit_host_normal4 (liblsx_fit_host.so) through the
device headers' arithmetic.  RF_vlos against brute force through the pinned lsx_stokes_host_window with the velocity changed at one
depth, inside (bar(S+) + bar(S-)) / a and with the response at least 1000 x the bar (tests/stokes_response_cases.py); the sums
against fit_cases.yardstick; drivers.fit_field_columns on the host backend recovering a field and a velocity; the refusals; the
stand-alone sanitizer program."""
import os
import re
import subprocess

import numpy as np
import pytest

import fit_cases as fc
import fit_instrument_cases as fic
import stokes_cases as sc
import stokes_response_cases as rc
import velocity_cases as vc
from conftest import ROOT
from lightspinner_amd import drivers, fit

CSRC = sc.CSRC
ENTRIES = {'lsx_hip_velocity_stokes_rays', 'lsx_hip_velocity_response_stokes', 'lsx_hip_velocity_fit_normal', 'lsx_hip_velocity_fit_chi2'}
MUS = (1.0, 0.6, 0.1)
LA0, NLA = 52, 44                 # the three lines of stokes_cases.problem with their wings
same = vc.same


@pytest.fixture(scope='module')
def host():
    return vc.HostLib()


@pytest.fixture(scope='module')
def fithost():
    return vc.FitHostLib()


def _col(Ns, pats='blend', vlos=True, lower_zero=False, given=True):
    """a stokes_cases column; given: the velocity of the call is velocity_cases.velocity, else the column's own"""
    prob, block, prof, J = sc.problem(Ns, 1, vlos=vlos)
    col = sc.column(prob, block, prof, block.n, J, sc.field(Ns, 1), sc.PATTERN_SETS[pats], 0, LA0, NLA, lower_zero)
    return col.replace(vlos=vc.velocity(Ns, 1)[0]) if given else col


# 3 and 4 depths put every depth into the start-value and the end-point sets at once, 5 parts the sets
CASES = [(3, 'triplet', False, False), (3, 'all', True, True), (4, 'blend', True, False), (4, 'largest', False, True),
         (5, 'all', True, False), (5, 'none', False, True)]


@pytest.mark.parametrize('Ns,pats,vlos,lower_zero', CASES)
def test_brute_force_on_every_depth(host, Ns, pats, vlos, lower_zero):
    """all four parameters at once and 'vlos' alone, on all depths and on subsets; 'none': no line has a pattern and the velocity still
    moves I"""
    col = _col(Ns, pats, vlos, lower_zero)
    amps = vc.amps(col.vB)
    for mu in MUS:
        ref, bar = rc.brute(host, col, mu, parameters=['vlos'], amplitudes=amps)
        names = ['vlos'] if pats == 'none' else list(vc.PARAMS)
        rf, S = host.response_v(col, mu, parameters=names)
        assert same(S, host.window(col, mu))                    # the stokes output has the window call's bits
        sig, x = rc.signal(ref['vlos'], bar['vlos']), rc.ratio(rf['vlos'], ref['vlos'], bar['vlos'])
        print('Ns %d %s vlos %s zero %s mu %.1f: deviation / bar %.3g, largest response / largest bar %.3g' % (Ns, pats, vlos, lower_zero, mu, x, sig))
        assert sig >= vc.SIGNAL and x <= 1.0, (mu, sig, x)
        alone, S1 = host.response_v(col, mu, parameters=['vlos'])
        assert same(alone['vlos'], rf['vlos']) and same(S1, S)
        for ks in ([0], [Ns - 1], [1, 2], [0, Ns - 2]):
            sub, _ = host.response_v(col, mu, parameters=names, ks=ks)
            assert all(same(sub[p], rf[p][..., ks]) for p in names), ks


def test_the_field_rows_are_the_old_entrys(host):
    """handed the column's own velocity, the rows of B, gammaB, chiB have the bits of lsx_stokes_host_response, whether vlos is
    requested or not; and they are the brute force's with a velocity that is not the column's"""
    for Ns, mu in ((5, 0.6), (13, 1.0)):
        col = _col(Ns, 'all', True, False, given=False)
        old, S0 = host.response(col, mu)
        for names in (rc.PARAMS, vc.PARAMS):
            new, S = host.response_v(col, mu, parameters=names)
            assert same(S, S0) and all(same(new[p], old[p]) for p in rc.PARAMS)
    col = _col(5, 'blend')
    ref, bar = rc.brute(host, col, 0.6)
    rf, _ = host.response_v(col, 0.6)
    for p in rc.PARAMS:
        assert rc.signal(ref[p], bar[p]) >= vc.SIGNAL and rc.ratio(rf[p], ref[p], bar[p]) <= 1.0, p


def test_every_refusal_with_its_code(host):
    col = _col(5, 'all')
    code = lambda c=col, **kw: host.response_v_rc(c, 0.6, **kw)[0]
    OK, EINVAL = sc.LSX_OK, sc.LSX_EINVAL
    assert code() == OK and code(want_stokes=False) == OK and code(parameters=['vlos']) == OK
    assert code(params_bits=0) == EINVAL and code(params_bits=16) == EINVAL and code(params_bits=24) == EINVAL
    assert host.response_rc(col, 0.6, params_bits=8)[0] == EINVAL              # the entry without a velocity does not know the bit
    for bad in (0.0, -100.0, np.nan, np.inf):
        a = dict(vc.amps(col.vB), vlos=bad)
        assert code(parameters=['vlos'], amplitudes=a) == EINVAL and code(amplitudes=a) == EINVAL
        assert code(parameters=rc.PARAMS, amplitudes=a) == OK               # not requested: not read
    for bad in (np.nan, np.inf, -np.inf):
        v = col.vlos.copy()
        v[3] = bad
        assert code(col.replace(vlos=v)) == EINVAL and code(col.replace(vlos=v), parameters=['B']) == EINVAL
    assert code(vlos=None) == EINVAL
    # no lower bound: any finite velocity, of either sign, and B's rule is still B's alone
    assert code(col.replace(vlos=np.full(5, -5.0e4))) == OK and code(col.replace(vlos=np.zeros(5))) == OK
    B0 = col.B.copy()
    B0[1] = 0.0
    assert code(col.replace(B=B0)) == EINVAL and code(col.replace(B=B0), parameters=['gammaB', 'chiB', 'vlos']) == OK


# ---- the sums with four quantities ---------------------------------------------------------------------------------------------------------
def _sums_case(host, fithost, Ns, nnode, mus, instrument):
    prob, block, prof, J = sc.problem(Ns, 1, vlos=True)
    fld4 = list(sc.field(Ns, 1)) + [vc.velocity(Ns, 1)]
    pats = sc.PATTERN_SETS['blend']
    basis, base = vc.basis_of(Ns, nnode), vc.base_of(fld4, nnode, False)
    truth = vc.nodes_of(fld4, Ns, nnode, base)
    hb = vc.HostBackend(host, fithost, prob, block, prof, block.n, J, pats, LA0, NLA)
    vB = float(np.min(prof[1]))
    amps = vc.amps(prof[1])
    S_true = np.stack([np.stack([host.window(c, mu) for mu in mus], axis=-1) for c in hb._columns(fithost.expand4(Ns, nnode, basis, base, truth))])
    inst = vc.recovery_instrument(prob) if instrument else None
    obs = S_true if inst is None else vc.smear(inst, S_true)
    nodes = vc.off_truth(truth, nnode, vB)
    return hb, basis, base, nodes, obs, amps, inst


@pytest.mark.parametrize('nnode', vc.NNODES)
@pytest.mark.parametrize('wkind', [None, 'given'])
def test_expand4_and_normal4_against_the_yardstick(host, fithost, nnode, wkind):
    Ns, mus = 13, np.array([1.0, 0.6])
    hb, basis, base, nodes, obs, amps, _ = _sums_case(host, fithost, Ns, nnode, mus, False)
    field = fithost.expand4(Ns, nnode, basis, base, nodes)
    o = np.cumsum([0] + list(nnode))
    for q in range(4):                                                  # the expansion, by its definition
        want = base[:, q] + (nodes[:, o[q]:o[q + 1]] @ basis[o[q]:o[q + 1]] if nnode[q] else 0.0)
        assert np.allclose(field[:, q], want, rtol=1e-14, atol=0.0)
    if sum(nnode[:3]):                                                  # the rows of the field are lsx_fit_host_expand's
        assert same(field[:, :3], fithost.expand(Ns, tuple(nnode[:3]), basis[:o[3]], base[:, :3], nodes[:, :o[3]]))
    w = fc.weights_of(wkind, obs.shape)
    ne = hb.fit_field_normal(mus, basis, nnode, nodes, obs, weight=w, base=base, amplitudes=amps)
    rf, S = hb.response(ne.field, mus, nnode, amps)
    val, bar = fc.yardstick(nnode, rf, S, obs, w, basis)
    x = fc.inside(dict(chi2=ne.chi2, grad=ne.grad, hess=ne.hess), val, bar)
    sig = fc.grad_signal(val, bar)
    print('nnode %s, weights %s: deviation / bar %s, largest |grad| / bar %.3g' % (nnode, wkind, x, sig))
    assert max(x.values()) <= 1.0 and sig >= fc.SIGNAL
    c2, f2 = hb.fit_field_chi2(mus, basis, nnode, nodes, obs, weight=w, base=base)
    assert same(c2, ne.chi2) and same(f2, ne.field)


def test_normal4_through_an_instrument(host, fithost):
    """Instrument.gaussian combined with velocity nodes: the sums are those of the smeared Jacobian and the smeared vector"""
    Ns, mus, nnode = 13, np.array([1.0]), (2, 2, 2, 2)
    hb, basis, base, nodes, obs, amps, inst = _sums_case(host, fithost, Ns, nnode, mus, True)
    ne = hb.fit_field_normal(mus, basis, nnode, nodes, obs, base=base, amplitudes=amps, instrument=inst)
    rf, S = hb.response(ne.field, mus, nnode, amps)
    val, bar = fic.yardstick(nnode, rf, S, obs, None, basis, inst)
    x = fc.inside(dict(chi2=ne.chi2, grad=ne.grad, hess=ne.hess), val, bar)
    print('through an instrument of %d pixels, width %d: deviation / bar %s' % (inst.nobs, inst.width, x))
    assert max(x.values()) <= 1.0 and fc.grad_signal(val, bar) >= fc.SIGNAL


# ---- the loop ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', range(len(vc.RECOVERY_CASES)))
def test_the_loop_recovers_field_and_velocity_on_the_host(host, fithost, case):
    """the loop of the GPU test on the host backend; its iteration count is what velocity_cases.HOST_ITERATIONS states, from which the
    GPU test's cap is taken (+ 2)"""
    Ns, nn, mus, ncol, through = vc.RECOVERY_CASES[case]
    mus = np.array(mus)
    (prob, block, prof, J), pats, fld4, nnode, basis, truth, start, vB = vc.recovery(Ns, ncol, nn)
    la0, nla = vc.RECOVERY_WINDOW
    hb = vc.HostBackend(host, fithost, prob, block, prof, block.n, J, pats, la0, nla)
    inst = vc.recovery_instrument(prob) if through else None
    S = np.stack([np.stack([host.window(c, mu) for mu in mus], axis=-1) for c in hb._columns(np.stack(fld4, axis=1))])
    obs = S if inst is None else vc.smear(inst, S)
    w = fc.recovery_weight(obs)
    kw = dict(instrument=inst) if through else {}
    r = drivers.fit_field_columns(hb, obs, mus, basis, start, nnode, weight=w, amplitudes=vc.amps(prof[1]), max_iter=30, **vc.RECOVERY_LOOP, **kw)
    o = 3 * nn
    print('case %d: chi2 %s -> %s in %s iterations, field error %.3g, velocity error / vBroad %.3g'
          % (case, r.history[0], r.chi2, r.iterations, np.max(np.abs(r.nodes[:, :o] - truth[:, :o])), np.max(np.abs(r.nodes[:, o:] - truth[:, o:])) / vB))
    vc.check_recovery(r, truth, nnode, vB, 30)
    assert int(r.iterations.max()) == vc.HOST_ITERATIONS[case], (int(r.iterations.max()), vc.HOST_ITERATIONS[case])
    assert same(r.field, fithost.expand4(Ns, nnode, basis, None, r.nodes))


# ---- the library's face --------------------------------------------------------------------------------------------------------------------
def test_the_entries_are_exported_declared_in_a_header_of_their_own_and_bound():
    lib = os.path.join(CSRC, 'liblsx_hip.so')
    assert os.path.exists(lib), 'build the HIP library first (make -C lightspinner_amd/csrc)'
    syms = subprocess.run(['nm', '-D', '--defined-only', lib], capture_output=True, text=True, check=True).stdout
    text = open(os.path.join(ROOT, 'include', 'lsx_hip_stokes_velocity.h')).read()
    assert set(re.findall(r'\b(lsx_hip_[a-z0-9_]+)\s*\(', text)) == ENTRIES
    assert set(re.findall(r'\bT (lsx_hip_velocity_[a-z0-9_]*)\b', syms)) == ENTRIES
    assert '#include "lsx_hip_stokes_velocity.h"' in open(os.path.join(ROOT, 'include', 'lsx_hip.h')).read()
    from lightspinner_amd import _capi
    hip = _capi.load_hip_library()
    assert hip.has_stokes_velocity and all(hasattr(hip.dll, n) for n in ENTRIES)


@pytest.mark.parametrize('compiler,std', [('gcc', 'c99'), ('g++', 'c++17')])
def test_the_header_compiles_alone(compiler, std):
    lang = 'c' if compiler == 'gcc' else 'c++'
    r = subprocess.run([compiler, '-std=' + std, '-Wall', '-Wextra', '-pedantic', '-Werror', '-fsyntax-only', '-x', lang,
                        os.path.join(ROOT, 'include', 'lsx_hip_stokes_velocity.h')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_stack_basis_with_and_without_a_velocity():
    b = fit.hat_basis(np.arange(5), [0.0, 4.0])
    bas, nn = fit.stack_basis(B=b, gammaB=np.ones(5), chiB=np.ones(5))
    assert nn == (2, 1, 1) and bas.shape == (4, 5)
    bas, nn = fit.stack_basis(B=b, chiB=np.ones(5), vlos=b)
    assert nn == (2, 0, 1, 2) and bas.shape == (5, 5) and np.array_equal(bas[3:], b)
    bas, nn = fit.stack_basis(vlos=np.ones(5))
    assert nn == (0, 0, 0, 1) and bas.shape == (1, 5)
    r = fit.FieldFit(np.arange(5.0)[None], None, None, None, None, None, None, (2, 0, 1, 2))
    assert np.array_equal(r.parameter('vlos'), [[3.0, 4.0]]) and np.array_equal(r.parameter('chiB'), [[2.0]])


def test_the_driver_passes_four_node_counts_through_untouched():
    seen = []

    class Backend:
        def fit_field_chi2(self, mus, basis, nnode, nodes, obs, **kw):
            seen.append(nnode)
            return np.ones(1), np.zeros((1, 4, 3))

        def fit_field_normal(self, mus, basis, nnode, nodes, obs, **kw):
            seen.append(nnode)
            return fit.FieldNormal(np.ones(1), np.zeros((1, 2)), np.eye(2)[None], np.zeros((1, 4, 3)))

        def fit_field_step(self, hess, grad, lam, nodes, lo, hi):
            return np.array(nodes), np.zeros(1), np.zeros(1, dtype=np.int32)

    nn = (1, 0, 0, 1)
    r = drivers.fit_field_columns(Backend(), np.zeros((1, 4, 1, 1)), [1.0], np.ones((2, 3)), np.zeros((1, 2)), nn, max_iter=2)
    assert all(s is nn for s in seen) and r.nnode == nn and r.field.shape == (1, 4, 3)


def test_the_kernels_with_a_velocity_use_no_scratch():
    """the compiler's resource reports: k_response_nodes<true> in its own unit, k_stokes_rays<1, true> beside <1, false>"""
    for unit, want in (('lsx_stokes_velocity', ['k_response_nodesILb1']), ('lsx_stokes', ['k_stokes_raysILi1ELb1', 'k_stokes_raysILi1ELb0'])):
        path = os.path.join(CSRC, 'build', unit + '.ru.log')
        if not os.path.exists(path):
            subprocess.check_call(['make', '-s', '-j', '8', '-C', CSRC])
        blocks = re.split(r'remark: [^\n]*Function Name: ', open(path).read())[1:]
        names = [b.split()[0] for b in blocks]
        assert len(names) == len(want) and all(any(w in n for n in names) for w in want), names
        for b, name in zip(blocks, names):
            val = lambda key: int(re.search(re.escape(key) + r':? (\d+)', b).group(1))
            assert val('ScratchSize [bytes/lane]') == 0 and val('VGPRs Spill') == 0 and re.search(r'Dynamic Stack: False', b), name


def test_the_host_twins_under_asan_ubsan():
    """3, 4 and 40 depths, every set of the four parameters, subsets, the refusals, the sums with 1 to 24 rows: in a stand-alone program"""
    subprocess.check_call(['make', '-s', '-C', CSRC, 'stokesvelsan'])
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:halt_on_error=1', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')
    out = subprocess.run([os.path.join(CSRC, 'lsx_stokes_velocity_san')], capture_output=True, text=True, timeout=600, env=env)
    tail = out.stdout[-1500:] + '\n' + out.stderr[-3000:]
    assert out.returncode == 0, tail
    assert 'STOKES VELOCITY SANITIZED RUN COMPLETE' in out.stdout, tail
