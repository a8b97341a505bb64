"""Depth-resolved final pass on the GPU (include/lsx_hip_depth.h, lsx_hip_depth_rays; Engine.depth_rays, Context.compute_depth_rays):
opacity, source function, optical depth, intensity and contribution function at every depth along arbitrary up-going rays, against
the reference's own arrays (tests/golden/depth_falc_*.npz) and the checkers of tests/depth_cases.py.

Bars (tests/depth_cases.py):
  chi, S    1e-12 relative against the numpy restatement of rh_method.py:601-632 (fed the library's own profiles at the angles);
            against the fixture that plus d_cpu, the restatement's own deviation from the reference;
  I(k)      against the oracle's unit entry fed the DEVICE's chi and S: 1e-11 |x| + 3 |x(+1) - x(-1)| entry by entry;
  tau       (Nspace + 8) u tau against np.cumsum of the device's chi;   contrib   16 u against numpy from the device's chi, S, tau;
  z_tau1    16 u max|z| against numpy from the device's tau.
Every call here is an ordinary valid call or is refused on the host."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import depth_cases as dc
import envelope
import rays_cases as rc
from conftest import golden
from helpers import build_data_fakes
from lightspinner_amd import _capi, fixtures, synth
from lightspinner_amd.problem import Engine
from lightspinner_amd.rh_method import Context

pytestmark = pytest.mark.gpu
FIXTURE = {'ca': 'falc_ca.npz', 'ca_vlos': 'falc_ca_vlos.npz', 'cah': 'falc_cah.npz'}
FIELDS = ('chi', 'S', 'tau', 'I', 'contrib', 'z_tau1')


def hip_engine(hip_lib, prob, block, prof, n=None, J=None, solver='linear', **kw):
    e = Engine(prob, block.ncol, lib=hip_lib, **kw)
    synth.load_columns(e, block, prof)
    e.set_formal_solver(solver)
    if n is not None:
        e.set(_capi.LSX_N, n)
    if J is not None:
        e.set(_capi.LSX_J, J)
    return e


def check_column(tag, oracle_lib, prob, block, col, n, J, phi, d, c, solver='linear', la0=0):
    """one column `c` of a DepthRays `d` (column `col` of the block) by every bar of the module's docstring; phi: LSX_PHI of that column
    at d.mus.  -> (chi, S of the restatement, I of the oracle's unit entry fed the device's chi and S), each [nla][nmu][Nspace]"""
    mus, z = d.mus, block.height[col]
    nla = d.chi.shape[-1]
    chi, S, I = (dc.to_lambda_major(getattr(d, f)[c]) for f in ('chi', 'S', 'I'))
    assert all(np.all(np.isfinite(getattr(d, f)[c])) for f in FIELDS[:5])
    chi_r, S_r = dc.restate_chi_S(prob, block, n, J, phi, mus.shape[0], col=col, la0=la0, nla=nla)
    dchi, dS = dc.relmax(chi, chi_r), dc.relmax(S, S_r)
    runs = dc.oracle_I_runs(oracle_lib, z, block.temperature[col], prob.wavelength[la0:la0 + nla], mus, chi, S, solver=solver)
    r, rel, renv = dc.excess_I(I, runs)
    rt = dc.check_tau(d.tau[c], d.chi[c], mus, z)
    rcn = dc.check_contrib(d.contrib[c], d.chi[c], d.S[c], d.tau[c], mus)
    rz = dc.check_z_tau1(d.z_tau1[c], d.tau[c], z)
    print('%s: chi %.2e, S %.2e against the restatement; I(k) %.2e relative against the oracle on the device chi, S (envelope up to '
          '%.2e, %.3f x the bound); tau %.2f, contrib %.2f, z_tau1 %.2f x their bounds; largest tau %.3g'
          % (tag, dchi, dS, rel, renv, r, rt, rcn, rz, float(d.tau[c].max())))
    assert dchi <= dc.BASE_CHI_S and dS <= dc.BASE_CHI_S, (tag, dchi, dS)
    assert r <= 1.0, '%s: I(k) is %.2f x the bound away from the oracle fed the device chi and S' % (tag, r)
    return chi_r, S_r, runs


def top_against_emergent_rays(tag, e, d, runs_by_col, check=True):
    """I[..., 0] against lsx_hip_emergent_rays of the same engine: inside the bound of I(k), entry by entry; bit-equal or not is reported"""
    top = e.emergent_rays(d.mus)                                     # [ncol][Nspect][nmu]
    la0, nla = d.la0, d.I.shape[-1]
    equal = True
    for c, runs in enumerate(runs_by_col):
        mine = dc.to_lambda_major(d.I[c])[:, :, 0]                   # [nla][nmu]
        other = top[c, la0:la0 + nla]
        bound = dc.BASE_I * np.abs(runs[0][:, :, 0]) + dc.K_ENVELOPE * np.abs(runs[1][:, :, 0] - runs[-1][:, :, 0])
        assert not check or np.all(np.abs(mine - other) <= bound), tag
        equal = equal and np.array_equal(mine, other)
    print('%s: I[..., 0] against lsx_hip_emergent_rays: %s (largest relative difference %.1e)'
          % (tag, 'bit-equal' if equal else 'not bit-equal', max(dc.relmax(dc.to_lambda_major(d.I[c])[:, :, 0], top[c, la0:la0 + nla])
                                                                  for c in range(len(runs_by_col)))))


def against_fixture(case, d_col):
    """chi, S of one column against the reference's recorded arrays: 1e-12 + d_cpu; I(k) is reported (its bar is the oracle's unit entry)"""
    f = dc.fixture(case)
    for name in ('chi', 'S'):
        dev = dc.relmax(dc.to_lambda_major(d_col[name]), f[name])
        print('%s %s against the reference: %.2e (bar %.1e)' % (case, name, dev, dc.BASE_CHI_S + dc.D_CPU[case][name]))
        assert dev <= dc.BASE_CHI_S + dc.D_CPU[case][name], (case, name, dev)
    print('%s I(k) against the reference: %.2e relative at worst' % (case, dc.relmax(dc.to_lambda_major(d_col['I']), f['I'])))


# ---- 1. the reference ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', dc.CASES)
def test_engine_gives_the_reference_at_every_depth(hip_lib, oracle_lib, case):
    prob, block, prof, n, J, _, _ = rc.golden_case(case)
    if prof is None:                # profiles by lsx_set_line_profiles in a phi_compact context without a velocity
        prof = fixtures.profile_inputs(prob, dict(np.load(golden(FIXTURE[case]))), with_vlos=False)
    bare = dataclasses.replace(block, phi=None, wphi=None)
    e = hip_engine(hip_lib, prob, bare, prof, n, J)
    d = e.depth_rays(dc.MUS)
    assert d.chi.shape == d.I.shape == (1, 3, prob.Nspace, prob.Nspect) and d.z_tau1.shape == (1, 3, prob.Nspect)
    assert not np.any(np.isnan(d.z_tau1))
    phi = dc.profiles_at(hip_lib, prob, bare, prof, dc.MUS)
    _, _, runs = check_column('Engine ' + case, oracle_lib, prob, block, 0, n[0], J[0], phi[0], d, 0)
    against_fixture(case, {f: getattr(d, f)[0] for f in FIELDS})
    top_against_emergent_rays('Engine ' + case, e, d, [runs])
    only = e.depth_rays(dc.MUS, what=('I', 'z_tau1'))                # any subset of the outputs
    assert only.chi is None and np.array_equal(only.I, d.I) and np.array_equal(only.z_tau1, d.z_tau1)
    e.close()


def native_context(hip_lib, case, n, J):
    d = dict(np.load(golden(FIXTURE[case])))
    s = dict(np.load(golden('setup_atoms.npz')))
    atmos, spect, eq, bg = build_data_fakes(d, s)
    ctx = Context(atmos, spect, eq, bg, lib=hip_lib)
    assert ctx.setup == 'native'
    off = 0
    for atom in ctx.activeAtoms:                   # host edits of atom.n and ctx.J are sent down first
        atom.n[...] = n[0, off:off + atom.Nlevel]
        off += atom.Nlevel
    ctx.J = J[0]
    return ctx


@pytest.mark.parametrize('case', dc.CASES)
def test_context_compute_depth_rays_gives_the_reference_at_every_depth(hip_lib, oracle_lib, case):
    """the drop-in Context with models that carry atomic data: the lsx_set_atmosphere path keeps aDamp, vBroad and vlos"""
    prob, block, prof, n, J, _, _ = rc.golden_case(case)
    ctx = native_context(hip_lib, case, n, J)
    I_before = ctx.I.copy()
    r = ctx.compute_depth_rays(dc.MUS)
    assert r.chi.shape == (3, prob.Nspace, prob.Nspect) and r.z_tau1.shape == (3, prob.Nspect) and r.la0 == 0
    against_fixture(case, {f: getattr(r, f) for f in FIELDS})
    z, T = block.height[0], block.temperature[0]
    chi, S, I = (dc.to_lambda_major(getattr(r, f)) for f in ('chi', 'S', 'I'))
    ex, rel, renv = dc.excess_I(I, dc.oracle_I_runs(oracle_lib, z, T, prob.wavelength, dc.MUS, chi, S))
    print('Context %s: I(k) %.2e relative against the oracle on the device chi, S, %.3f x the bound' % (case, rel, ex))
    assert ex <= 1.0
    dc.check_tau(r.tau, r.chi, dc.MUS, z)
    dc.check_contrib(r.contrib, r.chi, r.S, r.tau, dc.MUS)
    dc.check_z_tau1(r.z_tau1, r.tau, z)
    centre = ctx.compute_depth_rays(1.0)           # a float: no angle axis
    assert centre.I.shape == (prob.Nspace, prob.Nspect) and centre.z_tau1.shape == (prob.Nspect,)
    assert all(np.array_equal(getattr(centre, f), getattr(r, f)[-1]) for f in FIELDS)
    assert np.array_equal(ctx.I, I_before)         # ctx.I stays the quadrature's
    # behind a look-ahead formal solution: taken back first, so the answer is the accepted state's
    ctx.formal_sol_gamma_matrices()
    ctx.stat_equil()
    a = ctx.compute_depth_rays(dc.MUS, la0=40, nla=9)
    b = ctx._engine.depth_rays(dc.MUS, la0=40, nla=9)
    assert all(np.array_equal(getattr(a, f), getattr(b, f)[0]) for f in FIELDS) and not ctx._spec
    ctx.close()


# ---- 2. windows -----------------------------------------------------------------------------------------------------------------
def window_of(full, la0, nla):
    return {f: getattr(full, f)[..., la0:la0 + nla] for f in FIELDS}


@pytest.mark.parametrize('case', ['ca_vlos', 'cah'])
def test_a_window_is_a_slice_of_the_full_grid_call(hip_lib, case):
    prob, block, prof, n, J, _, _ = rc.golden_case(case)
    assert prob.Nspect == {'ca_vlos': 287, 'cah': 777}[case]
    ctx = native_context(hip_lib, case, n, J)
    full = ctx.compute_depth_rays(dc.MUS)
    Nspect = prob.Nspect
    # one wavelength; a start off every multiple of 12 and 64 that crosses a 64-lane boundary of the grid and of the window; the last
    # partial wavefront of the grid; the last wavelength alone
    for la0, nla in ((100, 1), (37, 50), (5, 100), (Nspect - Nspect % 64, Nspect % 64), (Nspect - 30, 30), (Nspect - 1, 1), (0, 64), (0, 65)):
        w = ctx.compute_depth_rays(dc.MUS, la0=la0, nla=nla)
        want = window_of(full, la0, nla)
        assert w.la0 == la0 and all(np.array_equal(getattr(w, f), want[f], equal_nan=True) for f in FIELDS), (la0, nla)
    trans = [t for a in ctx.activeAtoms for t in a.trans]
    for kr, t in enumerate(trans):
        if not t.isLine and kr > 1:
            continue                               # every line, the first continua
        la0, nla = t.Nblue, t.wavelength.shape[0]
        w = ctx.compute_depth_rays(dc.MUS, transition=t)
        x = ctx.compute_depth_rays(dc.MUS, la0=la0, nla=nla)
        k = ctx.compute_depth_rays(dc.MUS, transition=kr)
        want = window_of(full, la0, nla)
        assert w.la0 == la0 and w.I.shape[-1] == nla
        for f in FIELDS:
            assert np.array_equal(getattr(w, f), want[f], equal_nan=True) and np.array_equal(getattr(w, f), getattr(x, f), equal_nan=True)
            assert np.array_equal(getattr(w, f), getattr(k, f), equal_nan=True)
    ctx.close()


# ---- 3. angle chunking ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('solver', ['linear', 'parabolic'])
def test_every_angle_of_a_call_is_its_single_angle_call(hip_lib, solver):
    """nmu = 1, 3, 5, 9: register chunks of 1; 2 + 1; 4 + 1; 4 + 4 + 1"""
    prob, block, prof, n, J, _, _ = rc.golden_case('ca_vlos')
    e = hip_engine(hip_lib, prob, block, prof, n, J, solver=solver)
    mus9 = np.linspace(0.1, 1.0, 9)
    single = [e.depth_rays([m], la0=70, nla=90) for m in mus9]
    for nmu in (1, 3, 5, 9):
        sel = np.arange(9)[:: 8 // max(nmu - 1, 1)][:nmu] if nmu > 1 else np.array([4])
        d = e.depth_rays(mus9[sel], la0=70, nla=90)
        assert d.I.shape == (1, nmu, prob.Nspace, 90)
        for q, m in enumerate(sel):
            for f in FIELDS:
                assert np.array_equal(getattr(d, f)[:, q], getattr(single[m], f)[:, 0], equal_nan=True), (nmu, q, f)
    e.close()


# ---- 4., 5. batches with a line-of-sight velocity after MALI iterations --------------------------------------------------------
@pytest.mark.parametrize('fixture,ncol,solver', [('falc_ca.npz', 7, 'linear'), ('falc_cah.npz', 7, 'linear'), ('falc_ca.npz', 3, 'parabolic')])
def test_batches_after_mali_iterations(hip_lib, oracle_lib, fixture, ncol, solver):
    prob, block, prof = rc.batch(fixture, ncol)
    e = hip_engine(hip_lib, prob, block, prof, solver=solver)
    rc.mali(e)
    n, J = e.get(_capi.LSX_N), e.get(_capi.LSX_J)
    mus = np.concatenate([prob.muz, [0.33]])                         # the quadrature's own angles and one more: chunks of 4 + 2
    d = e.depth_rays(mus)
    phi = dc.profiles_at(hip_lib, prob, block, prof, mus)
    tag = '%s %s' % (fixture, solver)
    runs = [check_column('%s column %d' % (tag, c), oracle_lib, prob, block, c, n[c], J[c], phi[c], d, c, solver=solver)[2]
            for c in range(ncol)]
    top_against_emergent_rays(tag, e, d, runs)
    # I[..., 0] against the reference's final pass as the oracle's zero-weight context restates it, inside its envelope
    zw = rc.envelope_runs(oracle_lib, prob, block, prof, mus, n, J, solver)
    top = np.stack([dc.to_lambda_major(d.I[c])[:, :, 0] for c in range(ncol)])
    rel, renv = envelope.inside(top, zw, 0, _capi.LSX_I, base=1e-11)
    print('%s: I[..., 0] against the zero-weight oracle context: %.2e relative (envelope up to %.2e)' % (tag, rel, renv))
    # a column's result does not depend on the call: a sub-range, passes of 2 + 2 + 2 + 1 columns, the column alone in an engine
    part = e.depth_rays(mus, col0=2, ncol=min(3, ncol - 2))
    assert dc.same(part, d, slice(2, 2 + min(3, ncol - 2)))
    per_col = (5 * prob.Nspace + 1) * mus.shape[0] * prob.Nspect * 8
    assert dc.same(e.depth_rays(mus, work_cap_bytes=2 * per_col + 64), d)
    assert dc.same(e.depth_rays(mus, work_cap_bytes=1), d)           # below one column's need: one column per pass
    assert dc.same(e.depth_rays(mus, work_cap_bytes=0), d)
    e.close()
    for c in range(ncol):
        one = hip_engine(hip_lib, prob, block.slice(c, c + 1), tuple(x[c:c + 1] for x in prof), n[c:c + 1], J[c:c + 1], solver=solver)
        assert dc.same(one.depth_rays(mus), d, slice(c, c + 1)), c
        one.close()


# ---- 6. depth limits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('solver', ['linear', 'parabolic'])
def test_three_depths(hip_lib, oracle_lib, solver):
    """the smallest atmosphere lsx_create admits: the boundary value, one ordinary step (none under the parabolic rule) and the end point"""
    import instance_cases as ic
    prob, block = ic.build('two_atoms', 3, 3, True)
    e = hip_engine(hip_lib, prob, block, None, solver=solver)
    e.formal_sol_gamma()
    e.formal_sol_gamma()
    n, J = e.get(_capi.LSX_N), e.get(_capi.LSX_J)
    mus = np.array([0.2, 0.7, 1.0])
    d = e.depth_rays(mus)
    assert d.I.shape == (3, 3, 3, prob.Nspect)
    runs = [check_column('three depths %s column %d' % (solver, c), oracle_lib, prob, block, c, n[c], J[c], block.phi[c], d, c,
                         solver=solver)[2] for c in range(3)]
    # (reported, not held to the bar of I(k): on these made-up columns the end point of a ray is a cancellation of up to 2e5 between
    # w0 S of the interval below and w1 dS of its own, formal_solver.py:138-139, and the emergent-ray kernel shares one reciprocal
    # of 4e-15 between the two divisions of a step -- measured 1.9e-11 relative at one entry.  That kernel is pinned by its own tests)
    top_against_emergent_rays('three depths ' + solver, e, d, runs, check=False)
    e.close()


def test_325_depths(hip_lib, oracle_lib):
    from parabolic_cases import _refine_depth
    prob, base, raw = fixtures.load_problem_npz(golden('falc_ca.npz'))
    coarse, _ = synth.perturbed_columns(prob, base, raw, ncol=3, seed=4242, vlos_sigma=0.0)
    fine, fblock, _ = _refine_depth(prob, coarse, 4)
    assert fine.Nspace == 325
    e = hip_engine(hip_lib, fine, fblock, None)
    rc.mali(e)
    n, J = e.get(_capi.LSX_N), e.get(_capi.LSX_J)
    mus = np.array([0.15, 0.5, 1.0])
    d = e.depth_rays(mus)
    runs = [check_column('325 depths column %d' % c, oracle_lib, fine, fblock, c, n[c], J[c], fblock.phi[c], d, c)[2] for c in range(3)]
    top_against_emergent_rays('325 depths', e, d, runs)
    e.close()


# ---- 7. read-only ---------------------------------------------------------------------------------------------------------------
def snapshot(e):
    return {w: e.get(w) for w in (_capi.LSX_I, _capi.LSX_J, _capi.LSX_GAMMA, _capi.LSX_N, _capi.LSX_DJ_COL, _capi.LSX_DPOPS_COL)}


def same_state(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def test_the_call_changes_nothing(hip_lib):
    """a twin engine that never calls the entry gives bitwise the same I, J, Gamma, n and per-column monitors after the same script
    of calls -- including a call between a speculative formal solution and lsx_sync_end, and a discard afterwards"""
    ncol = 12
    prob, block, prof = rc.batch('falc_cah.npz', ncol)
    mus = [0.3, 1.0, 0.77]
    engines = [hip_engine(hip_lib, prob, block, prof) for _ in range(2)]
    probe, twin = engines
    seen = []
    for it in range(4):
        for e in engines:
            e.formal_sol_gamma()
        seen.append(probe.depth_rays(mus, la0=300, nla=200).I)
        assert same_state(snapshot(probe), snapshot(twin))
        if it >= 2:
            for e in engines:
                e.stat_equil()
            seen.append(probe.depth_rays(mus, la0=300, nla=200, col0=1, ncol=ncol - 2).I)
            assert same_state(snapshot(probe), snapshot(twin))
    # the pipelined loop: FS; SE; sync_begin; speculative FS; [the call]; sync_end; discard
    for e in engines:
        e.formal_sol_gamma_async()
        e.stat_equil_async()
        e.sync_begin()
        e.formal_sol_gamma_speculative()
    spec = probe.depth_rays(mus, la0=300, nla=200).I       # sees what lsx_get sees: the speculative call's J
    assert np.array_equal(probe.get(_capi.LSX_J), twin.get(_capi.LSX_J))
    mon = [e.sync_end() for e in engines]
    assert mon[0] == mon[1]
    assert same_state(snapshot(probe), snapshot(twin))
    for e in engines:
        e.discard_formal_sol()
    assert same_state(snapshot(probe), snapshot(twin))
    back = probe.depth_rays(mus, la0=300, nla=200).I       # the accepted call's J again
    assert not np.array_equal(back, spec)
    for e in engines:                                      # and the following calls produce the bits they would have produced
        e.formal_sol_gamma()
        e.stat_equil()
        e.formal_sol_gamma()
    assert same_state(snapshot(probe), snapshot(twin))
    assert all(np.all(np.isfinite(x)) and np.all(x > 0) for x in seen + [spec, back])
    # frozen columns are computed like any other
    d = probe.depth_rays(mus, la0=300, nla=200)
    probe.set_active_columns(np.arange(ncol) % 3 != 0)
    assert dc.same(probe.depth_rays(mus, la0=300, nla=200), d)
    for e in engines:
        e.close()


# ---- 8. errors are found on the host ---------------------------------------------------------------------------------------------
def test_errors(hip_lib):
    prob, block, prof = rc.batch('falc_ca.npz', 4)
    e = Engine(prob, 4, lib=hip_lib)
    e.set_columns(0, block)                       # profiles not set yet
    with pytest.raises(_capi.LsxError) as err:
        e.depth_rays([1.0])
    assert err.value.code == _capi.LSX_EINVAL and 'no line profiles' in str(err.value)
    e.set_line_profiles(0, *prof)
    e.formal_sol_gamma()
    before = snapshot(e)
    f = hip_lib.dll.lsx_hip_depth_rays
    LA0, NLA = 40, 20
    outs = [np.zeros((4, 2, prob.Nspace, NLA)) for _ in range(5)] + [np.zeros((4, 2, NLA))]
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))

    def call(mus, col0=0, ncol=4, la0=LA0, nla=NLA, nbytes=None, nbytes_z=None, nmu=None, arrays=outs):
        mu = np.asarray(mus, dtype=np.float64)
        return f(e._h, len(mu) if nmu is None else nmu, dp(mu), col0, ncol, la0, nla, *[dp(a) for a in arrays],
                 outs[0].nbytes if nbytes is None else nbytes, outs[5].nbytes if nbytes_z is None else nbytes_z)
    assert call([0.5, 1.0]) == 0
    good = [a.copy() for a in outs]
    for bad in ([0.5, 0.0], [0.5, -0.2], [1.0000001, 0.5], [0.5, np.nan], [np.inf, 0.5]):
        assert call(bad) == _capi.LSX_EINVAL, bad
    assert call([0.5, 1.0], nmu=0) == _capi.LSX_EINVAL
    assert call([0.5, 1.0], nmu=-1) == _capi.LSX_EINVAL
    assert call([0.5, 1.0], col0=-1) == _capi.LSX_EINVAL
    assert call([0.5, 1.0], col0=1, ncol=4) == _capi.LSX_EINVAL
    assert call([0.5, 1.0], ncol=0) == _capi.LSX_EINVAL
    assert call([0.5, 1.0], ncol=3) == _capi.LSX_EINVAL          # the byte counts are those of four columns
    assert call([0.5, 1.0], nla=0) == _capi.LSX_EINVAL
    assert call([0.5, 1.0], nla=-3) == _capi.LSX_EINVAL
    assert call([0.5, 1.0], la0=-1) == _capi.LSX_EINVAL
    assert call([0.5, 1.0], la0=prob.Nspect - NLA + 1) == _capi.LSX_EINVAL
    assert call([0.5, 1.0], la0=prob.Nspect) == _capi.LSX_EINVAL
    assert call([0.5, 1.0], nla=NLA + 1) == _capi.LSX_EINVAL     # the byte counts are those of NLA wavelengths
    assert call([0.5, 1.0], nbytes=outs[0].nbytes - 8) == _capi.LSX_EINVAL
    assert call([0.5, 1.0], nbytes_z=outs[5].nbytes + 8) == _capi.LSX_EINVAL
    assert call([0.5, 1.0], arrays=[None] * 6) == _capi.LSX_EINVAL
    assert f(e._h, 2, None, 0, 4, LA0, NLA, *[dp(a) for a in outs], outs[0].nbytes, outs[5].nbytes) == _capi.LSX_EINVAL
    assert all(np.array_equal(a, g) for a, g in zip(outs, good)) and same_state(snapshot(e), before)      # nothing launched or written
    # a byte count is looked at where an array it describes is asked for
    assert call([0.5, 1.0], arrays=outs[:5] + [None], nbytes_z=0) == 0
    assert call([0.5, 1.0], arrays=[None] * 5 + outs[5:], nbytes=0) == 0
    assert all(np.array_equal(a, g) for a, g in zip(outs, good))
    with pytest.raises(ValueError):
        e.depth_rays([1.0], what=('chi', 'J'))
    e.close()
    # ray-dependent profiles handed over as arrays: the library cannot know them at another angle
    prob, base, raw = fixtures.load_problem_npz(golden('falc_ca.npz'), phi_compact=False)
    e = Engine(prob, 1, lib=hip_lib)
    e.set_columns(0, base)
    with pytest.raises(_capi.LsxError) as err:
        e.depth_rays([1.0])
    assert err.value.code == _capi.LSX_EUNSUPPORTED
    assert 'lsx_set_line_profiles' in str(err.value) and 'lsx_set_atmosphere' in str(err.value)
    assert np.all(e.get(_capi.LSX_N) > 0)                          # nothing was launched: a following lsx_get works
    e.set_line_profiles(0, *fixtures.profile_inputs(prob, raw, with_vlos=False))     # ... and can once it has built them itself
    assert np.all(e.depth_rays([1.0], la0=10, nla=5).I > 0)
    e.close()
    # a phi_compact context's arrays are ray independent: served
    prob, base, raw = fixtures.load_problem_npz(golden('falc_ca.npz'))
    assert prob.phi_compact
    e = Engine(prob, 1, lib=hip_lib)
    e.set_columns(0, base)
    assert np.all(e.depth_rays([0.2, 1.0], la0=10, nla=5).I > 0)
    e.close()
